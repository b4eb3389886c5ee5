"""The dense LD matrix (twk_hip_ld_matrix, `tomahawk ldmatrix`): signed r, r2, D or D' of every pair of a region, filled on the GPU.

"Oracle matrix": the records of oracle.all_pairs (the pinned restatement of the reference) with minP = 1, the window applied here
where one is set (tests/test_gpu_ldscore.py oracle_records), scattered symmetrically into an n x n float64 array preset to the fill -
copysign(R, D) for r - with the diagonal 1 (for D: the fill).  The bar per entry that has an oracle record is the record path's own
plus float32's rounding, derived and not measured:

    |got - want| <= 1e-6 |want| + floor + 2^-24 |want|

floor: for records out of the unphased cubic the record's own floor for the field (tests/util.py cubic_floors with the record's
root error, as test_gpu_ldscore.oracle_score obtains it), zero otherwise.  Entries without an oracle record must equal the fill bit
for bit.  The fill is -2.0 - no statistic takes that value, so a pair-set disagreement cannot hide - but for one run each with the
default 0.0 and with NaN.  Every comparison also asserts exact symmetry (the same bits at (u, v) and (v, u)), the diagonal, and
n_records == the oracle's record count.  The data sets are test_gpu_ldscore's, on which existing tests show that engine and oracle
report the same pair set.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import FIELD, MODES, RTOL, STATS, mosaic140, oracle_records, stat_of
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

FILL = -2.0


def u32(m):
    return np.ascontiguousarray(m).view(np.uint32)


def oracle_matrix(ia, ib, recs, n, stat, fill, root_error=None, a0=0):
    """-> (want float64 (n, n), has bool (n, n), floor float64 (n, n)) of the records whose two variants lie in [a0, a0 + n)."""
    inside = (ia >= a0) & (ib < a0 + n)
    ia, ib, recs = ia[inside] - a0, ib[inside] - a0, recs[inside]
    want = np.full((n, n), fill, dtype=np.float64)
    has = np.zeros((n, n), dtype=bool)
    floor = np.zeros((n, n), dtype=np.float64)
    x = stat_of(recs, stat)
    want[ia, ib] = x; want[ib, ia] = x
    has[ia, ib] = True; has[ib, ia] = True
    for k in np.nonzero((recs["controller"] & 1) == 0)[0]:          # out of the unphased cubic
        w = recs[k]
        total = float(np.sum(w["cnt"]))
        dx = util.D_FLOOR
        if root_error is not None and total > 0:
            dx = min(max(dx, util.ROOT_ERROR_FACTOR * root_error(int(ia[k]) + a0, int(ib[k]) + a0, float(w["cnt"][0]) / total)[0]), util.DX_CEILING)
        f = util.cubic_floors([float(c) for c in w["cnt"]], w["R"], dx)[FIELD[stat]]
        floor[ia[k], ib[k]] = floor[ib[k], ia[k]] = f
    np.fill_diagonal(want, fill if stat == T.STAT_D else 1.0)
    return want, has, floor, len(recs)


def assert_matrix(m, want, has, floor, stat, fill, what=""):
    n = want.shape[0]
    assert m.dtype == np.float32 and m.shape == (n, n)
    bits = u32(m)
    fill_bits = np.array([fill], dtype=np.float32).view(np.uint32)[0]
    assert np.array_equal(bits, u32(m.T)), f"{what}: not symmetric"
    diag_bits = fill_bits if stat == T.STAT_D else np.array([1.0], dtype=np.float32).view(np.uint32)[0]
    assert (np.diagonal(bits) == diag_bits).all(), f"{what}: diagonal"
    off = ~np.eye(n, dtype=bool)
    none = off & ~has
    wrong = np.argwhere(none & (bits != fill_bits))
    assert len(wrong) == 0, f"{what}: {len(wrong)} entries without an oracle record are not the fill, first {wrong[:4].tolist()}"
    got = m.astype(np.float64)[has]
    w = want[has]
    err = np.abs(got - w)
    bar = RTOL * np.abs(w) + floor[has] + 2.0 ** -24 * np.abs(w)
    if len(w):
        worst = int(np.argmax(err - bar))
        print(f"{what}: {int(has.sum()) // 2} records, values {w.min():.6g}..{w.max():.6g}, largest |diff| {err.max():.3g}, "
              f"closest to the bar: diff {err[worst]:.3g} bar {bar[worst]:.3g} (value {w[worst]:.6g})")
    beyond = np.argwhere(has)[err > bar]
    assert len(beyond) == 0, f"{what}: {len(beyond)} entries beyond the bar, first {beyond[:4].tolist()}"


def check_against_oracle(hip, al, mode_key, stats=(T.STAT_R,), minR2=0.0, window=None, fill=FILL, variants=None, what="", **kw):
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al, variants)
    ia, ib, recs = oracle_records(data, mask, variants, N, mode_key, minR2, window)
    root_error = util.double_root_vetter(data, mask, variants, N).root_error
    if window is not None:
        kw.update(window=T.OPT_WINDOW, l_window=window)
    out = {}
    for stat in stats:
        want, has, floor, nrec = oracle_matrix(ia, ib, recs, M, stat, fill, root_error)
        m, n_records, n_pairs = hip.ld_matrix(MODES[mode_key][0], T.Filters(minR2=minR2), stat=stat, fill=fill, **kw)
        assert_matrix(m, want, has, floor, stat, fill, what or f"M={M} N={N} -{mode_key} {FIELD[stat]} minR2={minR2}")
        assert n_records == nrec == len(recs)
        out[stat] = (m, n_records, n_pairs, has)
    return out


# ---- 1: iid data, the smoke() set, every statistic ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_matrix_random_300x1000(hip, mode_key):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    out = check_against_oracle(hip, al, mode_key, stats=STATS)
    for stat in STATS:
        assert out[stat][2] == 300 * 299 // 2 and out[stat][1] > 44000
    last = hip.matrix_last()
    assert last["matrix_bytes"] == 300 * 300 * 4 and last["copy_ms"] > 0


# ---- 2: missing genotypes: masked planes, the default mode's two passes over regrouped sets ------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_matrix_with_missing(hip, mode_key):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    check_against_oracle(hip, al, mode_key, stats=STATS)


# ---- 3: real LD -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("N", [64, 250, 128, 1000])
def test_matrix_haplotype_blocks(hip, N, mode_key):
    m, nrec, _, has = check_against_oracle(hip, mosaic140(N), mode_key)[T.STAT_R]
    assert nrec > 1000 and (m[has] < 0).any() and (m[has] > 0.9).any()


def test_matrix_default_fill_is_zero_and_a_nan_fill_is_kept(hip):
    al = mosaic140(250)
    check_against_oracle(hip, al, "u", fill=0.0)
    out = check_against_oracle(hip, al, "u", stats=[T.STAT_R, T.STAT_D], fill=float("nan"))
    m, _, _, has = out[T.STAT_D]
    assert np.isnan(m[~has]).all() and np.isnan(np.diagonal(m)).all() and not np.isnan(m[has]).any()
    # the default arguments: signed r, fill 0
    m0, _, _ = hip.ld_matrix(T.MODE_UNPHASED, T.Filters(minR2=0.0))
    m1, _, _ = hip.ld_matrix(T.MODE_UNPHASED, T.Filters(minR2=0.0), stat=T.STAT_R, fill=0.0)
    assert np.array_equal(u32(m0), u32(m1))


# ---- 4: geometry: small tiles, a slice, a row pitch beyond n ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("a0,n", [(0, 300), (37, 203)])
def test_matrix_small_tiles_slice_and_pitch(hip, mode_key, a0, n):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    ia, ib, recs = oracle_records(data, mask, variants, N, mode_key)
    root_error = util.double_root_vetter(data, mask, variants, N).root_error
    want, has, floor, nrec = oracle_matrix(ia, ib, recs, n, T.STAT_R, FILL, root_error, a0=a0)
    hip.timing_reset()
    m, n_records, n_pairs = hip.ld_matrix(MODES[mode_key][0], T.Filters(minR2=0.0), fill=FILL, a0=a0, n=n, tile_variants=128)
    if n == 300:
        assert hip.timing()["count_launches"] >= 5          # diagonal and rectangular launches
    assert n_records == nrec and n_pairs == n * (n - 1) // 2
    assert_matrix(m, want, has, floor, T.STAT_R, FILL, f"tiles of 128, a0={a0} n={n} -{mode_key}")
    # the raw ABI with ld = n + 5 into a buffer preset to a sentinel pattern, a guard row before and after
    SENTINEL = np.uint32(0xDEADBEEF)
    ld = n + 5
    buf = np.full((n + 2, ld), SENTINEL, dtype=np.uint32)
    f = T.Filters(minR2=0.0)._c()
    nr, npairs = C.c_uint64(0), C.c_uint64(0)
    rc = hip._lib.twk_hip_ld_matrix(hip._ctx, MODES[mode_key][0], C.byref(f), a0, n, 128, 0, 0, T.STAT_R, C.c_float(FILL),
                                    buf[1:].ctypes.data, ld, C.byref(nr), C.byref(npairs))
    assert rc == 0 and nr.value == nrec and npairs.value == n_pairs
    assert (buf[0] == SENTINEL).all() and (buf[n + 1] == SENTINEL).all(), "a guard row was written"
    assert (buf[1:n + 1, n:] == SENTINEL).all(), "the padding columns were written"
    assert np.array_equal(buf[1:n + 1, :n], u32(m))


# ---- 5: window ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_matrix_window(hip, mode_key):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    m, nrec, _, has = check_against_oracle(hip, al, mode_key, window=2000)[T.STAT_R]
    assert nrec < 300 * 21 and int(has.sum(axis=1).max()) <= 40
    assert (m[~has & ~np.eye(300, dtype=bool)] == np.float32(FILL)).all()


# ---- 6: cut-off: the sparsified matrix --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minR2", [0.2, 0.8])
def test_matrix_cutoff(hip, minR2):
    al = mosaic140(250)
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    # no record of the unthresholded run lies within 1e-6 relative of the cut-off: the pair set cannot depend on the last bits of r2
    _, _, all_recs = oracle_records(data, mask, variants, N, "u", 0.0)
    assert not (np.abs(all_recs["R2"] - minR2) <= 1e-6 * minR2).any()
    m, nrec, _, has = check_against_oracle(hip, al, "u", stats=[T.STAT_R2], minR2=minR2)[T.STAT_R2]
    assert 0 < nrec == int((all_recs["R2"] >= minR2).sum())
    assert (m[has] >= np.float32(minR2 * (1 - 1e-6))).all()


# ---- 7: the engine's own records: the same d_pair, so bit for bit ------------------------------------------------------------------------
def matrix_of_records(recs, n, stat, fill):
    m = np.full((n, n), fill, dtype=np.float32)
    x = stat_of(recs, stat).astype(np.float32)          # the double rounded once, to nearest
    a, b = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64)
    m[a, b] = x; m[b, a] = x
    np.fill_diagonal(m, fill if stat == T.STAT_D else 1.0)
    return m


def assert_equals_record_path(hip, mode, M, stats, what, **kw):
    recs, npairs, _ = hip.ld_all(mode, T.Filters(minR2=0.0))
    for stat in stats:
        m, n_records, mp = hip.ld_matrix(mode, T.Filters(minR2=0.0), stat=stat, fill=FILL, **kw)
        want = matrix_of_records(recs, M, stat, FILL)
        differ = np.argwhere(u32(m) != u32(want))
        print(f"{what} {FIELD[stat]}: {len(recs)} records, {len(differ)} entries differ")
        assert n_records == len(recs) and mp == npairs
        assert len(differ) == 0, f"{what} {FIELD[stat]}: first {differ[:4].tolist()}"
        assert np.array_equal(u32(m), u32(m.T))


@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_matrix_equals_own_records_on_hostile_data(hip, mode_key):
    al = util.extreme_alleles(70, 64, 901, miss=True)
    util.upload(hip, al)
    assert_equals_record_path(hip, MODES[mode_key][0], 70, STATS, f"hostile -{mode_key}")


def test_matrix_long_rows(hip):
    """Rows of 100,003 samples: the count kernel splits tiles along K, several launches."""
    M, N = 1024, 100_003
    al = util.mosaic_alleles(M, N, seed=2, n_founders=5, switch=0.05, mut=0.01, miss_rate=0.01, miss_variants=0.3)
    util.upload(hip, al)
    for key in ("u", "auto"):
        hip.timing_reset()
        assert_equals_record_path(hip, MODES[key][0], M, [T.STAT_R], f"long rows -{key}", tile_variants=512)
        assert hip.timing()["count_launches"] >= 3


# ---- 8: against ld_score -----------------------------------------------------------------------------------------------------------------
def test_matrix_rows_add_up_to_the_scores(hip):
    al = mosaic140(250)
    M = al.shape[0]
    util.upload(hip, al)
    n_partners, sum_r2, _ = hip.ld_score(T.MODE_UNPHASED, T.Filters(minR2=0.0))
    m, nrec, _ = hip.ld_matrix(T.MODE_UNPHASED, T.Filters(minR2=0.0), stat=T.STAT_R2, fill=FILL)
    value = (u32(m) != np.array([FILL], dtype=np.float32).view(np.uint32)[0]) & ~np.eye(M, dtype=bool)
    assert np.array_equal(value.sum(axis=1).astype(np.uint64), n_partners) and int(value.sum()) == 2 * nrec
    rows = np.where(value, m.astype(np.float64), 0.0).sum(axis=1)
    assert (np.abs(rows - sum_r2) <= M * 2.0 ** -24 * sum_r2).all() and sum_r2.max() > 1.0


# ---- 9: determinism ---------------------------------------------------------------------------------------------------------------------
def test_matrix_runs_are_byte_identical(hip):
    util.upload(hip, mosaic140(250))
    a = hip.ld_matrix(T.MODE_UNPHASED, T.Filters(minR2=0.0), fill=FILL)
    b = hip.ld_matrix(T.MODE_UNPHASED, T.Filters(minR2=0.0), fill=FILL)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:] and a[1] > 1000


# ---- 10: errors -------------------------------------------------------------------------------------------------------------------------
def test_matrix_refuses_bad_arguments_and_leaves_the_engine_usable(hip):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    util.upload(hip, al)
    before, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    for kw in (dict(filters=T.Filters(minR2=0.0, minP=0.5)), dict(n=0), dict(a0=100, n=21), dict(a0=120, n=1), dict(stat=4), dict(stat=-1)):
        kw.setdefault("filters", T.Filters(minR2=0.0))
        with pytest.raises(T.HipError) as ei:
            hip.ld_matrix(T.MODE_AUTO, **kw)
        assert ei.value.code == -1, kw          # TWK_HIP_E_INVALID
    # ld < n and a NULL out, through the raw ABI
    f = T.Filters(minR2=0.0)._c()
    buf = np.zeros((120, 120), dtype=np.float32)
    assert hip._lib.twk_hip_ld_matrix(hip._ctx, T.MODE_AUTO, C.byref(f), 0, 120, 0, 0, 0, T.STAT_R, C.c_float(0.0), buf.ctypes.data, 119, None, None) == -1
    assert hip._lib.twk_hip_ld_matrix(hip._ctx, T.MODE_AUTO, C.byref(f), 0, 120, 0, 0, 0, T.STAT_R, C.c_float(0.0), None, 120, None, None) == -1
    assert not buf.any()
    after, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    assert len(before) > 1000 and before.tobytes() == after.tobytes()


# ---- 11: the command line ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,mode_key,window,stat,text", [(["-p"], "p", None, T.STAT_R, False),
                                                             (["-u", "-w", "3000", "-s", "r2", "-T"], "u", 3000, T.STAT_R2, True)])
def test_ldmatrix_cli(hip, tmp_path, flags, mode_key, window, stat, text):
    al = mosaic140(250)
    M, N, _ = al.shape
    rid = np.repeat([0, 1], [80, 60]).astype(np.uint32)
    pos = np.concatenate([np.arange(80) * 100 + 1000, np.arange(60) * 100 + 500]).astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    prefix = str(tmp_path / "out")
    r = subprocess.run([hostlib.CLI_PATH, "ldmatrix", "-i", twk, "-o", prefix] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    util.upload(hip, al, variants)
    kw = dict(window=T.OPT_WINDOW, l_window=window) if window is not None else {}
    m, nrec, _ = hip.ld_matrix(MODES[mode_key][0], T.Filters(minR2=0.0), stat=stat, fill=0.0, **kw)
    assert nrec > 1000
    if text:
        got = np.loadtxt(prefix + ".ld", dtype=np.float64)
        assert got.shape == (M, M) and (np.abs(got - m.astype(np.float64)) <= 5e-9 * np.abs(m.astype(np.float64))).all()
        assert all(len(line.split(" ")) == M for line in open(prefix + ".ld").read().splitlines())
        assert not (tmp_path / "out.npy").exists()
    else:
        raw = open(prefix + ".npy", "rb").read()
        assert raw[:8] == b"\x93NUMPY\x01\x00"
        hlen = int.from_bytes(raw[8:10], "little")
        assert (10 + hlen) % 64 == 0 and raw[10 + hlen - 1:10 + hlen] == b"\n"
        assert f"'descr': '<f4', 'fortran_order': False, 'shape': ({M}, {M})" in raw[10:10 + hlen].decode("latin1")
        got = np.load(prefix + ".npy")
        assert got.dtype == np.float32 and got.shape == (M, M) and np.array_equal(u32(got), u32(m))
        assert not (tmp_path / "out.ld").exists()
    rows = [l.split("\t") for l in open(prefix + ".variants.tsv").read().splitlines()]
    # contig / pos as `ldscore` prints them: the contig's name, the 1-based position; the selection in file order
    assert [x[0] for x in rows] == [str(int(x) + 1) for x in rid] and [int(x[1]) for x in rows] == [int(p) + 1 for p in pos]
