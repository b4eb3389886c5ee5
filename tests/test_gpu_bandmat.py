"""The banded LD matrix (twk_hip_ld_matrix_band, `tomahawk ldmatrix --band -w`): the dense matrix's values of a windowed run in band
storage - per row only the columns inside the window.

Two references.  The oracle matrix of tests/test_gpu_matrix.py (the oracle's records with the window applied, scattered) with that
module's own bar, RTOL |want| + the cubic floor + 2^-24 |want|, for the band scattered to dense; and the engine's dense call with the
same arguments, which the band must equal BIT FOR BIT at every slot it stores, while everything it does not store must be the fill in
the dense matrix.  The layout is restated here with searchsorted over (rid, pos).  The fill is -2.0, which no statistic takes.
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import FIELD, MODES, STATS, big_plain, blob, mosaic140, oracle_records
from tests.test_gpu_matrix import FILL, assert_matrix, oracle_matrix, u32
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

FILL_BITS = np.array([FILL], dtype=np.float32).view(np.uint32)[0]
F0 = T.Filters(minR2=0.0)


def layout_of(variants, window, a0=0, n=None):
    """first, indptr of the slice by the definition: the variants on the row's contig within the window, by searchsorted over the
    (rid, pos) key of the sorted slice."""
    n = len(variants) - a0 if n is None else n
    pos = variants["pos"].astype(np.int64)[a0:a0 + n]
    rid = variants["rid"].astype(np.int64)[a0:a0 + n]
    K = np.int64(1) << 34
    key = rid * K + pos
    assert (np.diff(key) >= 0).all()
    lo = np.searchsorted(key, rid * K + np.maximum(pos - window, 0), side="left")
    hi = np.searchsorted(key, rid * K + np.minimum(pos + window, K - 1), side="right")
    return lo.astype(np.uint32), np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint64)


def rows_and_columns(first, indptr):
    lens = np.diff(indptr.astype(np.int64))
    rows = np.repeat(np.arange(len(first), dtype=np.int64), lens)
    cols = np.arange(int(indptr[-1]), dtype=np.int64) - indptr.astype(np.int64)[:-1][rows] + first.astype(np.int64)[rows]
    return rows, cols


def assert_layout(first, indptr, variants, window, a0=0, n=None):
    want_first, want_ptr = layout_of(variants, window, a0, n)
    assert first.dtype == np.uint32 and indptr.dtype == np.uint64
    assert np.array_equal(first, want_first) and np.array_equal(indptr, want_ptr)


def assert_band_equals_dense(hip, mode, window, variants, stats=(T.STAT_R,), fill=FILL, what="", **kw):
    """The band against the dense call with the same arguments, bit for bit; -> the last (values, first, indptr, n_records, n_pairs)."""
    fill_bits = np.array([fill], dtype=np.float32).view(np.uint32)[0]
    for stat in stats:
        dense, nrec_d, np_d = hip.ld_matrix(mode, F0, stat=stat, fill=fill, window=T.OPT_WINDOW, l_window=window, **kw)
        band = hip.ld_matrix_band(mode, F0, window, stat=stat, fill=fill, **kw)
        values, first, indptr, nrec, npairs = band
        n = dense.shape[0]
        assert_layout(first, indptr, variants, window, kw.get("a0", 0), n)
        assert values.dtype == np.float32 and values.shape == (int(indptr[-1]),)
        rows, cols = rows_and_columns(first, indptr)
        differ = np.nonzero(u32(values) != u32(dense)[rows, cols])[0]
        outside = np.ones((n, n), dtype=bool)
        outside[rows, cols] = False
        print(f"{what} {FIELD[stat]}: n {n}, band {len(values)} of {n * n}, {nrec} records, {len(differ)} slots differ, "
              f"{int((u32(dense)[outside] != fill_bits).sum())} dense entries outside the band are no fill")
        assert len(differ) == 0, f"{what} {FIELD[stat]}: first {[(int(rows[k]), int(cols[k])) for k in differ[:4]]}"
        assert (u32(dense)[outside] == fill_bits).all(), f"{what}: the dense matrix has a value outside the band"
        assert nrec == nrec_d and npairs == np_d
        assert np.array_equal(u32(T.band_to_dense(values, first, indptr, fill)), u32(dense))
    return band


# ---- 1: against the oracle ----------------------------------------------------------------------------------------------------------------
WINDOW = 2000


@functools.lru_cache(maxsize=None)
def random_300():
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    al.setflags(write=False)
    return al


@functools.lru_cache(maxsize=None)
def oracle_of_random_300(mode_key):
    """The oracle's windowed records of the set, once per mode: shared by the statistics."""
    al = random_300()
    data, mask = O.bitvectors_from_alleles(al)
    variants = O.variants_from_alleles(al)
    ia, ib, recs = oracle_records(data, mask, variants, al.shape[1], mode_key, 0.0, WINDOW)
    return ia, ib, recs, util.double_root_vetter(data, mask, variants, al.shape[1]).root_error


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_band_against_the_oracle(hip, mode_key):
    al = random_300()
    M = al.shape[0]
    _, _, variants = util.upload(hip, al)
    ia, ib, recs, root_error = oracle_of_random_300(mode_key)
    for stat in STATS:
        want, has, floor, nrec = oracle_matrix(ia, ib, recs, M, stat, FILL, root_error)
        values, first, indptr, n_records, n_pairs = hip.ld_matrix_band(MODES[mode_key][0], F0, WINDOW, stat=stat, fill=FILL)
        assert_layout(first, indptr, variants, WINDOW)
        assert 300 * 21 < int(indptr[-1]) <= 300 * 41 and values.shape == (int(indptr[-1]),)
        assert_matrix(T.band_to_dense(values, first, indptr, FILL), want, has, floor, stat, FILL, f"band -{mode_key} {FIELD[stat]}")
        # in-band slots without an oracle record are the fill, bit for bit (the diagonal apart)
        rows, cols = rows_and_columns(first, indptr)
        none = ~has[rows, cols] & (rows != cols)
        assert none.any() and (u32(values)[none] == FILL_BITS).all()
        assert n_records == nrec == len(recs) and nrec > 2000
    last = hip.bandmat_last()
    assert last["band_bytes"] == int(indptr[-1]) * 4 and last["copy_ms"] > 0
    f2, p2 = hip.bandmat_layout(WINDOW)
    assert np.array_equal(f2, first) and np.array_equal(p2, indptr)


# ---- 2: bit-identical to the dense call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_band_equals_dense_with_missing_data(hip, mode_key):
    """Masked planes and, in the default mode, the two passes over regrouped sets: both stores per lane at the file-order ids."""
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    _, _, variants = util.upload(hip, al)
    band = assert_band_equals_dense(hip, MODES[mode_key][0], 1500, variants, stats=STATS, what=f"missing -{mode_key}")
    assert band[3] > 500


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_band_wider_than_a_column_block_over_several_launches(hip, mode_key):
    _, _, variants = util.upload(hip, big_plain())
    hip.timing_reset()
    values, first, indptr, nrec, _ = assert_band_equals_dense(hip, MODES[mode_key][0], 30000, variants, what=f"700 x 250 -{mode_key}", tile_variants=128)
    assert hip.timing()["count_launches"] >= 10
    assert int(np.diff(indptr.astype(np.int64)).max()) == 601 and nrec > 50000


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_band_of_a_slice(hip, mode_key):
    _, _, variants = util.upload(hip, random_300())
    values, first, indptr, _, npairs = assert_band_equals_dense(hip, MODES[mode_key][0], WINDOW, variants, what=f"slice -{mode_key}", a0=37, n=203, tile_variants=128)
    assert len(first) == 203 and first[0] == 0 and int(first[-1]) == 203 - 21


def contig_variants(al):
    """Three contigs of 97, 105 and 98 variants, positions restarting per contig: clusters a base apart, duplicated positions, steps
    of 90 and gaps of 5000 - beyond the window of 1500."""
    M = al.shape[0]
    assert M == 300
    rid = np.repeat([0, 1, 2], [97, 105, 98]).astype(np.uint32)
    pos = np.zeros(M, dtype=np.uint32)
    p = 0
    for v in range(M):
        if v in (0, 97, 202):
            p = 500
        pos[v] = p
        p += 5000 if v % 50 in (48, 49) else 0 if v % 7 == 3 else 1 if v % 5 == 0 else 90          # (variants 49, 99, ..: alone in their window)
    return O.variants_from_alleles(al, pos=pos, rid=rid)


@pytest.mark.parametrize("mode_key,window", [("p", 1500), ("u", 1500), ("u", 0)])
def test_band_across_contigs_clusters_duplicates_and_gaps(hip, mode_key, window):
    al = util.random_alleles(300, 200, seed=77, low_ac=4)
    variants = contig_variants(al)
    util.upload(hip, al, variants)
    values, first, indptr, nrec, _ = assert_band_equals_dense(hip, MODES[mode_key][0], window, variants, what=f"contigs -{mode_key} w={window}", tile_variants=128)
    lens = np.diff(indptr.astype(np.int64))
    rid = variants["rid"]
    rows, cols = rows_and_columns(first, indptr)
    assert (rid[rows] == rid[cols]).all() and lens.min() == 1 and nrec > 0
    if window == 0:      # the duplicated positions alone
        assert lens.max() == 2 and int(indptr[-1]) > 300
    else:
        assert lens.max() > 30


def test_band_beyond_the_span_is_the_dense_matrix(hip):
    al = mosaic140(250)
    n = al.shape[0]
    _, _, variants = util.upload(hip, al)
    values, first, indptr, nrec, _ = assert_band_equals_dense(hip, T.MODE_UNPHASED, 10 ** 9, variants, stats=[T.STAT_R, T.STAT_D], what="whole span")
    assert int(indptr[-1]) == n * n and not first.any() and nrec > 1000
    dense, _, _ = hip.ld_matrix(T.MODE_UNPHASED, F0, stat=T.STAT_D, fill=FILL)          # (no window at all: the same matrix)
    assert np.array_equal(u32(values.reshape(n, n)), u32(dense))


# ---- 3: the caller's buffer and its capacity ------------------------------------------------------------------------------------------------
def test_band_stays_inside_the_callers_buffer_and_honours_its_capacity(hip):
    al = random_300()
    _, _, variants = util.upload(hip, al)
    a0, n = 37, 203
    values, first, indptr, nrec, npairs = hip.ld_matrix_band(T.MODE_UNPHASED, F0, WINDOW, fill=FILL, a0=a0, n=n, tile_variants=128)
    nnz = int(indptr[-1])
    SENTINEL, G = np.uint32(0xDEADBEEF), 4096
    f = F0._c()

    def raw(capacity):
        buf = np.full(nnz + 2 * G, SENTINEL, dtype=np.uint32)
        fi, ptr = np.full(n, SENTINEL, dtype=np.uint32), np.full(n + 1, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        nr, npr = C.c_uint64(0), C.c_uint64(0)
        rc = hip._lib.twk_hip_ld_matrix_band(hip._ctx, T.MODE_UNPHASED, C.byref(f), a0, n, 128, int(T.OPT_WINDOW), WINDOW, T.STAT_R, C.c_float(FILL),
                                             buf[G:].ctypes.data, capacity, fi.ctypes.data, ptr.ctypes.data, C.byref(nr), C.byref(npr))
        return rc, buf, fi, ptr, nr.value, npr.value

    rc, buf, fi, ptr, nr, npr = raw(nnz)
    assert rc == 0 and nr == nrec and npr == npairs
    assert (buf[:G] == SENTINEL).all(), "the words before values[0] were written"
    assert (buf[G + nnz:] == SENTINEL).all(), "the words from values[nnz] on were written"
    assert np.array_equal(buf[G:G + nnz], u32(values)) and np.array_equal(fi, first) and np.array_equal(ptr, indptr)
    rc, buf, fi, ptr, _, _ = raw(nnz - 1)
    assert rc == -1          # TWK_HIP_E_INVALID
    assert (buf == SENTINEL).all() and (fi == SENTINEL).all() and (ptr == np.uint64(0xDEADBEEFDEADBEEF)).all()


# ---- 4: repeatability -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["u", "auto"])
def test_band_runs_and_tilings_return_the_same_bytes(hip, mode_key):
    al = util.mosaic_alleles(600, 128, 5003, n_founders=6, switch=0.005, mut=0.0, miss_rate=0.05, miss_variants=0.3)
    util.upload(hip, al)
    mode = MODES[mode_key][0]
    a = hip.ld_matrix_band(mode, F0, 20000, fill=FILL)
    b = hip.ld_matrix_band(mode, F0, 20000, fill=FILL)
    c = hip.ld_matrix_band(mode, F0, 20000, fill=FILL, tile_variants=128)
    assert blob(a[:4]) == blob(b[:4]) == blob(c[:4]) and a[3] > 10000 and a[4] == b[4]


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_band_refuses_bad_arguments_and_leaves_the_engine_usable(hip):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    util.upload(hip, al)
    before, nrec_before, _ = hip.ld_matrix(T.MODE_AUTO, F0, fill=FILL, window=T.OPT_WINDOW, l_window=1500)
    for kw in (dict(filters=T.Filters(minR2=0.0, minP=0.5)), dict(n=0), dict(a0=100, n=21), dict(a0=120, n=1), dict(stat=4), dict(stat=-1)):
        kw.setdefault("filters", F0)
        with pytest.raises(T.HipError) as ei:
            hip.ld_matrix_band(T.MODE_AUTO, l_window=1500, **kw)
        assert ei.value.code == -1, kw          # TWK_HIP_E_INVALID
    with pytest.raises(T.HipError) as ei:
        hip.bandmat_layout(1500, a0=100, n=21)
    assert ei.value.code == -1
    # through the raw ABI: no window bit, a NULL values, first or row_ptr, n == 0
    f = F0._c()
    first, indptr = hip.bandmat_layout(1500)
    nnz = int(indptr[-1])
    SENTINEL = np.uint32(0xDEADBEEF)
    buf = np.full(nnz, SENTINEL, dtype=np.uint32)
    fi, ptr = np.zeros(120, dtype=np.uint32), np.zeros(121, dtype=np.uint64)

    def raw(window=int(T.OPT_WINDOW), values=buf.ctypes.data, first=fi.ctypes.data, row_ptr=ptr.ctypes.data, n=120):
        return hip._lib.twk_hip_ld_matrix_band(hip._ctx, T.MODE_AUTO, C.byref(f), 0, n, 0, window, 1500, T.STAT_R, C.c_float(FILL),
                                               values, nnz, first, row_ptr, None, None)

    assert raw(window=0) == -1 and raw(window=int(T.OPT_KEEP_LOW_AC)) == -1
    assert raw(values=None) == -1 and raw(first=None) == -1 and raw(row_ptr=None) == -1 and raw(n=0) == -1
    assert hip._lib.twk_hip_bandmat_layout(hip._ctx, 0, 120, 1500, None, ptr.ctypes.data) == -1
    assert (buf == SENTINEL).all() and not fi.any() and not ptr.any()
    assert raw() == 0 and (buf != SENTINEL).all() and np.array_equal(fi, first) and np.array_equal(ptr, indptr)
    after, nrec_after, _ = hip.ld_matrix(T.MODE_AUTO, F0, fill=FILL, window=T.OPT_WINDOW, l_window=1500)
    assert nrec_before > 500 and nrec_after == nrec_before and before.tobytes() == after.tobytes()


# ---- 6: the command line --------------------------------------------------------------------------------------------------------------------
def test_ldmatrix_band_cli(hip, tmp_path):
    al = mosaic140(250)
    M, N, _ = al.shape
    rid = np.repeat([0, 1], [80, 60]).astype(np.uint32)
    pos = np.concatenate([np.arange(80) * 100 + 1000, np.arange(60) * 100 + 500]).astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    prefix = str(tmp_path / "out")
    r = subprocess.run([hostlib.CLI_PATH, "ldmatrix", "-i", twk, "-o", prefix, "-u", "-w", "3000", "-s", "r2", "--band"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    util.upload(hip, al, variants)
    values, first, indptr, nrec, _ = hip.ld_matrix_band(T.MODE_UNPHASED, F0, 3000, stat=T.STAT_R2, fill=0.0)
    assert nrec > 1000
    assert_layout(first, indptr, variants, 3000)
    got = {name: np.load(f"{prefix}.{name}.npy") for name in ("values", "indptr", "first")}
    assert got["values"].dtype == np.float32 and got["values"].shape == (int(indptr[-1]),) and np.array_equal(u32(got["values"]), u32(values))
    assert got["indptr"].dtype == np.int64 and got["indptr"].shape == (M + 1,) and np.array_equal(got["indptr"], indptr.astype(np.int64))
    assert got["first"].dtype == np.int32 and got["first"].shape == (M,) and np.array_equal(got["first"], first.astype(np.int32))
    raw = open(prefix + ".values.npy", "rb").read()
    assert raw[:8] == b"\x93NUMPY\x01\x00"
    hlen = int.from_bytes(raw[8:10], "little")
    assert (10 + hlen) % 64 == 0 and f"'descr': '<f4', 'fortran_order': False, 'shape': ({int(indptr[-1])},)" in raw[10:10 + hlen].decode("latin1")
    assert not (tmp_path / "out.npy").exists() and not (tmp_path / "out.ld").exists()
    # the three files are a CSR matrix as they stand, and scattered they are the dense command's matrix
    dense, _, _ = hip.ld_matrix(T.MODE_UNPHASED, F0, stat=T.STAT_R2, fill=0.0, window=T.OPT_WINDOW, l_window=3000)
    assert np.array_equal(u32(T.band_to_dense(got["values"], got["first"], got["indptr"], 0.0)), u32(dense))
    rows = [l.split("\t") for l in open(prefix + ".variants.tsv").read().splitlines()]
    assert [x[0] for x in rows] == [str(int(x) + 1) for x in rid] and [int(x[1]) for x in rows] == [int(p) + 1 for p in pos]
