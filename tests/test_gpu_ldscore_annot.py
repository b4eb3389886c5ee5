"""Partitioned LD scores (twk_hip_ld_score_annot, `tomahawk ldscore --annot`): for every variant v and annotation column c the sum over
the records `calc` reports with v at either end of rint((R2 * a[w][c]) * 2^32), w the variant at the other end, summed exactly in
integers on the GPU, converted once and divided by 2^32.

"Own records": the engine's records of the same problem (ld_all, minR2 = 0); the sum above formed on the host in integers must match
the call bit for bit, and n must be the records' count.  "Oracle": the records of oracle.all_pairs; the bar is the record path's own
(1e-6 relative plus the cubic's floor per record, tests/util.py) carried through the weights, plus half a quantum per term:

    |got - want| <= sum over v's records of |a[w][c]| * (1e-6 * R2_w + floor_R2(record_w)) + n(v) * 2^-33 * max(1, max|a|)
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import MODES, RTOL, alleles, margin_holds, mosaic140, oracle_records
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

A11_NAMES = ["ones", "bernoulli", "every17", "zeros", "uniform", "normal", "big", "tiny", "negzero", "small_int", "index"]


def a11(M, seed=4711):
    """The standard annotation set: M rows of 11 columns."""
    rng = np.random.default_rng(seed)
    big = np.zeros(M)
    sel = rng.random(M) < 0.1
    big[sel] = rng.choice([-65536.0, 65536.0], int(sel.sum()))
    cols = [np.ones(M), (rng.random(M) < 0.3).astype(np.float64), (np.arange(M) % 17 == 0).astype(np.float64), np.zeros(M),
            rng.random(M), rng.standard_normal(M), big, 2.0 ** -40 * rng.random(M), np.full(M, -0.0),
            rng.integers(0, 4, M).astype(np.float64), np.arange(M) / M]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def score_of_records(recs, annot, M):
    """-> (n uint64[M], score float64[M, C], magnitude float64[M, C]) of records with fields idxA, idxB, R2: the definition, in integers."""
    ia, ib, r2 = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64), recs["R2"].astype(np.float64)
    n = np.zeros(M, dtype=np.uint64)
    np.add.at(n, ia, 1); np.add.at(n, ib, 1)
    ta = np.rint((r2[:, None] * annot[ib]) * 2.0 ** 32)          # to (A, c): exact integers below 2^49 in float64
    tb = np.rint((r2[:, None] * annot[ia]) * 2.0 ** 32)          # to (B, c)
    total = np.zeros(annot.shape, dtype=np.int64)               # (fewer than 2^14 terms a variant: no overflow)
    np.add.at(total, ia, ta.astype(np.int64)); np.add.at(total, ib, tb.astype(np.int64))
    mag = np.zeros(annot.shape, dtype=np.float64)
    np.add.at(mag, ia, np.abs(ta)); np.add.at(mag, ib, np.abs(tb))
    score = np.array([float(int(x)) / 2 ** 32 for x in total.ravel()], dtype=np.float64).reshape(annot.shape)
    return n, score, mag / 2.0 ** 32


def assert_equals_own_records(hip, mode, annot, what, filters=None, recs=None, **kw):
    """The call against the engine's own records of the same call geometry, bit for bit.  -> (n, score, n_pairs, records)"""
    M = annot.shape[0]
    filters = filters or T.Filters(minR2=0.0)
    if recs is None:
        a0, b0 = kw.get("a0", 0), kw.get("b0", 0)
        region = dict(a0=a0, nA=M - a0, b0=b0, nB=M - b0, triangle=True)
        region.update(kw)
        recs = hip.ld_region(mode, filters, **region)[0]
    wn, ws, _ = score_of_records(recs, annot, M)
    n, s, npairs = hip.ld_score_annot(mode, filters, annot, **kw)
    assert n.dtype == np.uint64 and s.dtype == np.float64 and n.shape == (M,) and s.shape == annot.shape
    bad = np.argwhere(s.view(np.uint64) != ws.view(np.uint64))
    print(f"{what}: {len(recs)} records, {annot.shape[1]} columns, {len(bad)} entries differ; largest |score| {np.abs(ws).max():.6g}")
    assert np.array_equal(n, wn), f"{what}: n differs at {np.nonzero(n != wn)[0][:8].tolist()}"
    assert len(bad) == 0, f"{what}: (variant, column) {bad[:6].tolist()}: got {[s[tuple(b)] for b in bad[:6]]} want {[ws[tuple(b)] for b in bad[:6]]}"
    return n, s, npairs, recs


# ---- 1: bit-exact against the engine's own records ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_annot_random_300x1000(hip, mode_key):
    al = alleles("random")
    util.upload(hip, al)
    n, s, npairs, recs = assert_equals_own_records(hip, MODES[mode_key][0], a11(300), f"random 300x1000 -{mode_key}")
    assert npairs == 300 * 299 // 2 and len(recs) > 44000 and (s[:, 3] == 0).all() and (s[:, 8] == 0).all()


@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_annot_with_missing(hip, mode_key):
    util.upload(hip, alleles("missing"))
    assert_equals_own_records(hip, MODES[mode_key][0], a11(120), f"missing -{mode_key}")


@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("N", [64, 250, 128, 1000])
def test_annot_haplotype_blocks(hip, N, mode_key):
    util.upload(hip, alleles(f"mosaic{N}"))
    _, s, _, recs = assert_equals_own_records(hip, MODES[mode_key][0], a11(140), f"mosaic N={N} -{mode_key}")
    assert len(recs) > 1000 and s[:, 0].max() > 1.0


@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_annot_hostile_data(hip, mode_key):
    util.upload(hip, util.extreme_alleles(70, 64, 901, miss=True))
    assert_equals_own_records(hip, MODES[mode_key][0], a11(70), f"hostile -{mode_key}")


# ---- 2: against the oracle ---------------------------------------------------------------------------------------------------------
def record_floors(ia, ib, recs, root_error=None):
    """floor_R2 of every record: 0 for a record of the phased math, the cubic's floor otherwise (as test_gpu_ldscore.py forms it)."""
    fl = np.zeros(len(recs), dtype=np.float64)
    for k in np.nonzero((recs["controller"] & 1) == 0)[0]:
        w = recs[k]
        total = float(np.sum(w["cnt"]))
        dx = util.D_FLOOR
        if root_error is not None and total > 0:
            dx = min(max(dx, util.ROOT_ERROR_FACTOR * root_error(int(ia[k]), int(ib[k]), float(w["cnt"][0]) / total)[0]), util.DX_CEILING)
        fl[k] = util.cubic_floors([float(x) for x in w["cnt"]], w["R"], dx)["R2"]
    return fl


@pytest.mark.parametrize("name,mode_key", [("random", "p"), ("random", "u"), ("missing", "p"), ("missing", "u"), ("missing", "auto"),
                                           ("mosaic250", "p"), ("mosaic250", "u"), ("mosaic250", "auto")])
def test_annot_against_oracle(hip, name, mode_key):
    al = alleles(name)
    M, N, _ = al.shape
    annot = a11(M)
    data, mask, variants = util.upload(hip, al)
    ia, ib, want = oracle_records(data, mask, variants, N, mode_key)
    fl = record_floors(ia, ib, want, util.double_root_vetter(data, mask, variants, N).root_error)
    r2 = want["R2"].astype(np.float64)
    wn = np.zeros(M, dtype=np.uint64)
    np.add.at(wn, ia, 1); np.add.at(wn, ib, 1)
    ws, bar = np.zeros(annot.shape), np.zeros(annot.shape)
    np.add.at(ws, ia, r2[:, None] * annot[ib]); np.add.at(ws, ib, r2[:, None] * annot[ia])
    slack = (RTOL * r2 + fl)[:, None]
    np.add.at(bar, ia, np.abs(annot[ib]) * slack); np.add.at(bar, ib, np.abs(annot[ia]) * slack)
    bar += wn[:, None].astype(np.float64) * 2.0 ** -33 * max(1.0, float(np.abs(annot).max()))
    n, s, _ = hip.ld_score_annot(MODES[mode_key][0], T.Filters(minR2=0.0), annot)
    err = np.abs(s - ws)
    worst = np.unravel_index(int(np.argmax(err - bar)), err.shape)
    print(f"{name} -{mode_key}: {len(want)} oracle records, largest |diff| {err.max():.3g}, closest to the bar: {worst} diff {err[worst]:.3g} bar {bar[worst]:.3g}")
    assert np.array_equal(n, wn), f"n differs at {np.nonzero(n != wn)[0][:8].tolist()}"
    assert (err <= bar).all(), f"beyond the bar at {np.argwhere(err > bar)[:8].tolist()}"


# ---- 3: category count: slabs and strides ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cycled_columns(M, C=256):
    """C columns cycled from the standard set, each from a seed of its own."""
    return np.ascontiguousarray(np.stack([a11(M, seed=9000 + k)[:, k % 11] for k in range(C)], axis=1))


_SINGLE = {}


def single_column_scores(hip, annot):
    """Column k alone, for every k: computed once (the caller has uploaded mosaic140(250))."""
    if "s" not in _SINGLE:
        _SINGLE["s"] = np.stack([hip.ld_score_annot(T.MODE_UNPHASED, T.Filters(minR2=0.0), annot[:, k])[1][:, 0] for k in range(annot.shape[1])], axis=1)
    return _SINGLE["s"]


@pytest.mark.parametrize("ncat", [1, 7, 8, 9, 65, 256])
def test_annot_category_count(hip, ncat):
    util.upload(hip, alleles("mosaic250"))
    annot = cycled_columns(140)
    single = single_column_scores(hip, annot)
    n, s, _ = hip.ld_score_annot(T.MODE_UNPHASED, T.Filters(minR2=0.0), annot[:, :ncat])
    assert s.shape == (140, ncat) and s.tobytes() == np.ascontiguousarray(single[:, :ncat]).tobytes()
    assert np.abs(s).max() > 1.0


def test_annot_padded_rows(hip):
    """ld_annot > n_annot: the padding is never read into a result."""
    util.upload(hip, alleles("mosaic250"))
    M, ncat, ld = 140, 9, 13
    annot = np.ascontiguousarray(cycled_columns(140)[:, :ncat])
    padded = np.full((M, ld), np.nan)          # (a sentinel the engine would refuse, had it looked)
    padded[:, :ncat] = annot
    want = hip.ld_score_annot(T.MODE_UNPHASED, T.Filters(minR2=0.0), annot)
    n = np.zeros(M, dtype=np.uint64)
    s = np.full((M, ncat), -7.0)
    npairs = C.c_uint64(0)
    f = T.Filters(minR2=0.0)._c()
    rc = hip._lib.twk_hip_ld_score_annot(hip._ctx, T.MODE_UNPHASED, C.byref(f), 0, M, 0, M, 1, 0, 1, 0, 0, 0, padded.ctypes.data, ncat, ld,
                                         n.ctypes.data, s.ctypes.data, C.byref(npairs))
    assert rc == 0 and npairs.value == want[2]
    assert n.tobytes() == want[0].tobytes() and s.tobytes() == want[1].tobytes()
    # one double too few a row is refused
    assert hip._lib.twk_hip_ld_score_annot(hip._ctx, T.MODE_UNPHASED, C.byref(f), 0, M, 0, M, 1, 0, 1, 0, 0, 0, padded.ctypes.data, ncat, ncat - 1,
                                           n.ctypes.data, s.ctypes.data, C.byref(npairs)) == -1


# ---- 4: geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_annot_small_tiles(hip, mode_key):
    util.upload(hip, alleles("random"))
    annot, mode = a11(300), MODES[mode_key][0]
    whole = hip.ld_score_annot(mode, T.Filters(minR2=0.0), annot)
    recs = hip.ld_all(mode, T.Filters(minR2=0.0))[0]
    hip.timing_reset()
    n, s, npairs, _ = assert_equals_own_records(hip, mode, annot, f"tile_variants=128 -{mode_key}", recs=recs, tile_variants=128)
    assert hip.timing()["count_launches"] >= 5          # diagonal and rectangular launches
    assert n.tobytes() == whole[0].tobytes() and s.tobytes() == whole[1].tobytes() and npairs == whole[2]


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_annot_rectangle(hip, mode_key):
    util.upload(hip, alleles("random"))
    n, s, npairs, recs = assert_equals_own_records(hip, MODES[mode_key][0], a11(300), f"rectangle -{mode_key}",
                                                   a0=50, nA=100, b0=150, nB=150, triangle=False)
    assert npairs == 100 * 150 and len(recs) > 5000
    assert not n[:50].any() and not s[:50].any() and (n[50:] > 0).all()


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_annot_window(hip, mode_key):
    util.upload(hip, alleles("random"))
    n, s, _, recs = assert_equals_own_records(hip, MODES[mode_key][0], a11(300), f"window 2000 -{mode_key}", window=T.OPT_WINDOW, l_window=2000)
    assert 0 < int(n.max()) <= 40 and 0 < len(recs) < 300 * 21


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_annot_shards_add_up(hip, mode_key):
    util.upload(hip, alleles("mosaic250"))
    annot, mode = a11(140), MODES[mode_key][0]
    n1, s1, p1, recs = assert_equals_own_records(hip, mode, annot, f"whole -{mode_key}")
    parts = [assert_equals_own_records(hip, mode, annot, f"shard {k}/3 -{mode_key}", part=k, n_parts=3) for k in range(3)]
    assert sum(p[2] for p in parts) == p1 and sum(len(p[3]) for p in parts) == len(recs)
    assert np.array_equal(np.sum([p[0] for p in parts], axis=0, dtype=np.uint64), n1)
    mag = score_of_records(recs, annot, 140)[2]         # the sum of the contributions' magnitudes
    assert (np.abs(parts[0][1] + parts[1][1] + parts[2][1] - s1) <= 3 * 2.0 ** -52 * mag).all()


@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("minR2", [0.2, 0.5, 0.8])
def test_annot_threshold(hip, minR2, mode_key):
    al = alleles("mosaic1000")
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    # no record of the unthresholded run lies within 1e-6 relative of the cut-off: the pair set cannot depend on the last bits of r2
    _, _, all_recs = oracle_records(data, mask, variants, N, mode_key, 0.0)
    assert margin_holds(all_recs["R2"], minR2)
    _, _, _, recs = assert_equals_own_records(hip, MODES[mode_key][0], a11(M), f"minR2={minR2} -{mode_key}", filters=T.Filters(minR2=minR2))
    assert 0 < len(recs) == int((all_recs["R2"] >= minR2).sum())


# ---- 5: ties to ld_score -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_annot_all_ones_is_the_ld_score(hip, mode_key):
    util.upload(hip, alleles("mosaic128"))
    M, mode = 140, MODES[mode_key][0]
    sn, ss, sp = hip.ld_score(mode, T.Filters(minR2=0.0))
    n, s, npairs = hip.ld_score_annot(mode, T.Filters(minR2=0.0), np.ones(M))
    assert npairs == sp and np.array_equal(n, sn) and s.shape == (M, 1) and ss.max() > 1.0
    assert (np.abs(s[:, 0] - ss) <= sn.astype(np.float64) * 2.0 ** -33 + 2 * M * 2.0 ** -53 * ss).all()


# ---- 6: long rows: the count kernel splits tiles along K, several launches ----------------------------------------------------------
def test_annot_long_rows(hip):
    M, N = 1024, 100_003
    al = util.mosaic_alleles(M, N, seed=2, n_founders=5, switch=0.05, mut=0.01, miss_rate=0.01, miss_variants=0.3)
    util.upload(hip, al)
    annot = np.ascontiguousarray(cycled_columns(M, 9))
    recs = hip.ld_all(T.MODE_PHASED, T.Filters(minR2=0.0))[0]
    hip.timing_reset()
    assert_equals_own_records(hip, T.MODE_PHASED, annot, "long rows -p", recs=recs, tile_variants=512)
    assert hip.timing()["count_launches"] >= 3


# ---- 7: determinism and state --------------------------------------------------------------------------------------------------------
def test_annot_runs_are_bit_identical(hip):
    util.upload(hip, alleles("mosaic250"))
    annot = a11(140)
    a = hip.ld_score_annot(T.MODE_UNPHASED, T.Filters(minR2=0.0), annot)
    b = hip.ld_score_annot(T.MODE_UNPHASED, T.Filters(minR2=0.0), annot)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1].max() > 1.0


def test_annot_refusals_leave_the_engine_usable(hip):
    util.upload(hip, alleles("missing"))
    M = 120
    annot = a11(M)
    before, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    first = hip.ld_score_annot(T.MODE_AUTO, T.Filters(minR2=0.0), annot)
    assert before.tobytes() == hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))[0].tobytes() and len(before) > 1000
    nan, big = annot.copy(), annot.copy()
    nan[77, 4] = np.nan
    big[5, 2] = 65537.0
    refused = [(T.Filters(minR2=0.0, minP=0.5), annot), (T.Filters(minR2=0.0), nan), (T.Filters(minR2=0.0), big),
               (T.Filters(minR2=0.0), np.zeros((M, 0))), (T.Filters(minR2=0.0), np.zeros((M, 257)))]
    for filters, a in refused:
        with pytest.raises(T.HipError) as ei:
            hip.ld_score_annot(T.MODE_AUTO, filters, a)
        assert ei.value.code == -1          # TWK_HIP_E_INVALID
    with pytest.raises(T.HipError) as ei:
        hip.ld_score_annot(T.MODE_AUTO, T.Filters(minR2=0.0), nan)
    assert "variant 77" in str(ei.value) and "column 4" in str(ei.value)
    with pytest.raises(ValueError):
        hip.ld_score_annot(T.MODE_AUTO, T.Filters(minR2=0.0), annot[:-1])
    again = hip.ld_score_annot(T.MODE_AUTO, T.Filters(minR2=0.0), annot)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert before.tobytes() == hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))[0].tobytes()


# ---- 8: the command line -------------------------------------------------------------------------------------------------------------
def _run_cli(twk, flags):
    r = subprocess.run([hostlib.CLI_PATH, "ldscore", "-i", twk] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head = [l for l in r.stdout.splitlines() if l.startswith("#")]
    rows = [l.split("\t") for l in r.stdout.splitlines() if l and not l.startswith("#")]
    return head, rows


@pytest.mark.parametrize("flags,mode_key,window", [(["-p"], "p", None), (["-u", "-w", "3000"], "u", 3000)])
def test_ldscore_annot_cli(hip, tmp_path, flags, mode_key, window):
    al = alleles("mosaic250")
    M, N, _ = al.shape
    rid = np.repeat([0, 1], [80, 60]).astype(np.uint32)
    pos = np.concatenate([np.arange(80) * 100 + 1000, np.arange(60) * 100 + 500]).astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    names = ["coding", "enhancer", "conserved", "weight", "signed"]
    annot = np.ascontiguousarray(a11(M)[:, [1, 2, 9, 4, 5]])
    left_out = np.arange(3, M, 14)[:10]
    annot[left_out] = 0.0
    path = str(tmp_path / "annot.txt")
    with open(path, "w") as fh:
        fh.write("## baseline annotations\n")
        fh.write("CHR\tBP\tSNP\tCM\t" + "\t".join(names) + "\n")
        for v in range(M):
            if v in left_out:
                continue
            fh.write(f"{int(rid[v]) + 1}\t{int(pos[v]) + 1}\trs{v}\t0.0\t" + "\t".join(repr(float(x)) for x in annot[v]) + "\n")
    # the binding on the same data
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    util.upload(hip, al, variants=variants)
    kw = dict(window=T.OPT_WINDOW, l_window=window) if window is not None else {}
    wn, ws, _ = hip.ld_score_annot(MODES[mode_key][0], T.Filters(minR2=0.0), annot, **kw)

    head, rows = _run_cli(twk, flags + ["--annot", path])
    assert head[-1].lstrip("#").split("\t") == ["contig", "pos", "n_partners"] + names
    assert "##annotations=5" in head and not any(h.startswith("##self") for h in head)
    assert len(rows) == M and all(len(r) == 3 + 5 for r in rows)
    assert [r[0] for r in rows] == [str(int(x) + 1) for x in rid] and [int(r[1]) for r in rows] == [int(p) + 1 for p in pos]
    n = np.array([int(r[2]) for r in rows], dtype=np.uint64)
    s = np.array([[float(x) for x in r[3:]] for r in rows], dtype=np.float64)
    assert np.array_equal(n, wn) and s.tobytes() == ws.tobytes() and np.abs(s).max() > 1.0
    assert all(repr(float(x)) == repr(float("%.17g" % float(x))) and x == "%.17g" % float(x) for r in rows for x in r[3:])
    # ##M and ##M_5_50 against numpy: sums over the variants in file order, the second over minor allele frequency > 0.05
    called = 2 * N - variants["an"].astype(np.int64)
    ac = variants["ac"].astype(np.int64)
    common = np.minimum(ac, called - ac) / np.maximum(called, 1) > 0.05
    def column_sums(sel):
        out = np.zeros(5)
        for v in np.nonzero(sel)[0]:
            out += annot[v]
        return out
    got = {h.split("=", 1)[0]: h.split("=", 1)[1] for h in head if h.startswith("##M")}
    assert [float(x) for x in got["##M"].split(",")] == column_sums(np.ones(M, bool)).tolist()
    assert [float(x) for x in got["##M_5_50"].split(",")] == column_sums(common).tolist()
    assert common.any()

    head2, rows2 = _run_cli(twk, flags + ["--annot", path, "--self"])
    assert "##self=1" in head2
    s2 = np.array([[float(x) for x in r[3:]] for r in rows2], dtype=np.float64)
    assert s2.tobytes() == (ws + annot).tobytes() and [r[:3] for r in rows2] == [r[:3] for r in rows]

    # without -a: the parent's format
    head0, rows0 = _run_cli(twk, flags)
    assert head0[-1].lstrip("#").split("\t") == ["contig", "pos", "n_partners", "sum_r2"] and all(len(r) == 4 for r in rows0)
    assert not any(h.startswith(("##annotations", "##M", "##self")) for h in head0)
