"""LD decay (twk_hip_ld_decay, `tomahawk lddecay`): r2 by the distance between two variants, binned and summed exactly on the GPU.

A pair COUNTS when `calc` reports a record for it, both variants lie on one contig and their positions differ; its bin is
min(|posA - posB| // (range_bp // n_bins), n_bins - 1); per bin the call returns the number of counting pairs and the sum of their R2.

"Oracle decay": the records of oracle.all_pairs (the pinned restatement of the reference) with minP = 1, binned in numpy by that
definition.  The oracle names a variant by (contig, position), so its records are taken ONCE per (data set, mode, cut-off) with the
default positions, which are unique; a record does not depend on positions, and every test bins those records with the positions it
uploads (duplicates and a second contig included).  The bar is the score test's plus the quantisation, derived and not measured:

    |sum(bin) - want(bin)| <= 1e-6 want(bin) + sum over the bin's cubic records of floor_R2(record) + n(bin) * 2^-33

(a record's R2 is held to 1e-6 relative plus, out of the unphased cubic, the record's own floor - tests/util.py cubic_floors; the
engine adds rint(R2 * 2^32), at most 2^-33 from R2, a pair) and n must be equal in every bin.

"Own records, exactly": for the same call arguments ld_region's records are binned here with q = rint(R2 * 2^32) as integers; n must be
equal and float(S) / 2^32 BIT-IDENTICAL to sum_r2 - the sums are exact in integers, whatever the tiling and the order.

The data sets are ones on which tests/test_gpu_ldscore.py shows that engine and oracle report the same pair set.
"""
import functools
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import MODES, RTOL, alleles, blob, oracle_records, positions
from tests.reduce_cases import data_set as big_data_set
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
Q_STEP = 2.0 ** -33                 # |rint(R2 * 2^32) / 2^32 - R2| of one pair
RANGE = 30000                       # the 300 variants at the default spacing of 100 span 29,900 bases

@functools.lru_cache(maxsize=None)
def oracle(name, mode_key, minR2=0.0):
    """-> (ia, ib, R2, floor) of the oracle's records of the set, each pair once (ia < ib in file order): computed once, never changed."""
    al = alleles(name)
    N = al.shape[1]
    data, mask = O.bitvectors_from_alleles(al)
    variants = O.variants_from_alleles(al)
    ia, ib, want = oracle_records(data, mask, variants, N, mode_key, minR2)
    root_error = util.double_root_vetter(data, mask, variants, N).root_error
    floor = np.zeros(len(want), dtype=np.float64)
    for k in np.nonzero((want["controller"] & 1) == 0)[0]:              # out of the cubic (tests/test_gpu_ldscore.py oracle_score)
        w = want[k]
        total = float(np.sum(w["cnt"]))
        dx = util.D_FLOOR
        if total > 0:
            dx = min(max(dx, util.ROOT_ERROR_FACTOR * root_error(int(ia[k]), int(ib[k]), float(w["cnt"][0]) / total)[0]), util.DX_CEILING)
        floor[k] = util.cubic_floors([float(x) for x in w["cnt"]], w["R"], dx)["R2"]
    out = (ia, ib, want["R2"].astype(np.float64), floor)
    for a in out:
        a.setflags(write=False)
    return out


def bins_of(ia, ib, pos, rid, range_bp, n_bins):
    """The definition -> (counts: bool per pair, bin per pair)."""
    width = range_bp // n_bins
    d = np.abs(pos[ia] - pos[ib])
    return (rid[ia] == rid[ib]) & (d != 0), np.minimum(d // width, n_bins - 1)


def oracle_decay(name, mode_key, pos, rid, range_bp, n_bins, minR2=0.0, window=None, inside=None):
    """-> (n uint64[n_bins], sum float64[n_bins], floor float64[n_bins], records that count)."""
    ia, ib, r2, floor = oracle(name, mode_key, minR2)
    counts, b = bins_of(ia, ib, pos, rid, range_bp, n_bins)
    if window is not None:
        counts &= (rid[ia] == rid[ib]) & (np.abs(pos[ia] - pos[ib]) <= window)
    if inside is not None:
        counts &= inside(ia, ib)
    n = np.bincount(b[counts], minlength=n_bins).astype(np.uint64)
    s = np.zeros(n_bins, dtype=np.float64)
    fl = np.zeros(n_bins, dtype=np.float64)
    np.add.at(s, b[counts], r2[counts])
    np.add.at(fl, b[counts], floor[counts])
    return n, s, fl, int(counts.sum())


def assert_decay(got_n, got_s, want_n, want_s, floor, what):
    assert got_n.dtype == np.uint64 and got_s.dtype == np.float64 and got_n.shape == got_s.shape == want_n.shape
    err = np.abs(got_s - want_s)
    bar = RTOL * want_s + floor + want_n.astype(np.float64) * Q_STEP
    worst = int(np.argmax(err - bar))
    print(f"{what}: {int(want_n.sum())} pairs in {int((want_n > 0).sum())} of {len(want_n)} bins, largest |diff| {err.max():.3g} (bin {int(np.argmax(err))}), "
          f"closest to the bar: bin {worst} diff {err[worst]:.3g} bar {bar[worst]:.3g} (quantisation share {float(want_n[worst]) * Q_STEP:.3g})")
    bad_n = np.nonzero(got_n != want_n)[0]
    assert len(bad_n) == 0, f"{what}: n differs at bins {bad_n[:8].tolist()}: got {got_n[bad_n[:8]].tolist()} want {want_n[bad_n[:8]].tolist()}"
    assert (err <= bar).all(), f"{what}: sum beyond the bar at bins {np.nonzero(err > bar)[0][:8].tolist()}"


def decay_of_records(recs, pos, rid, range_bp, n_bins):
    """The engine's own records binned on the host in integers -> (n uint64[n_bins], sum_r2 float64[n_bins], S as Python integers)."""
    ia, ib = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64)
    counts, b = bins_of(ia, ib, pos, rid, range_bp, n_bins)
    q = np.rint(recs["R2"].astype(np.float64) * 4294967296.0).astype(np.uint64)          # (the product is exact: a power of two)
    acc = np.zeros(n_bins, dtype=np.uint64)                                               # below 2^64: at most 2^32 a pair, far fewer than 2^31 pairs
    np.add.at(acc, b[counts], q[counts])
    S = [int(x) for x in acc]
    n = np.bincount(b[counts], minlength=n_bins).astype(np.uint64)
    return n, np.array([float(x) / 2 ** 32 for x in S], dtype=np.float64), S


def assert_equals_own_records(hip, mode, filters, pos, rid, range_bp, n_bins, got, what, a0=0, nA=None, b0=0, nB=None, triangle=True, **kw):
    M = len(pos)
    nA = M - a0 if nA is None else nA
    nB = M - b0 if nB is None else nB
    recs, npairs, _ = hip.ld_region(mode, filters, a0, nA, b0, nB, triangle, **kw)
    rn, rs, _ = decay_of_records(recs, pos, rid, range_bp, n_bins)
    n, s, sp = got
    print(f"{what}: {len(recs)} own records, {int(rn.sum())} of them count")
    assert sp == npairs
    assert np.array_equal(n, rn), f"{what}: n differs from the own records' at bins {np.nonzero(n != rn)[0][:8].tolist()}"
    assert s.tobytes() == rs.tobytes(), f"{what}: sums differ from the own records' at bins {np.nonzero(s != rs)[0][:8].tolist()}"
    return len(recs)


def check(hip, name, mode_key, range_bp, n_bins, pos=None, rid=None, minR2=0.0, window=None, own=True, **kw):
    """Upload the set with these positions; the call against the oracle and (own) against the engine's own records."""
    al = alleles(name)
    M = al.shape[0]
    p, r = positions(M, pos, rid)
    util.upload(hip, al, pos=p.astype(np.uint32), rid=r.astype(np.uint32))
    wn, ws, fl, n_counting = oracle_decay(name, mode_key, p, r, range_bp, n_bins, minR2, window)
    args = dict(kw)
    if window is not None:
        args.update(window=T.OPT_WINDOW, l_window=window)
    what = f"{name} -{mode_key} range={range_bp} bins={n_bins} minR2={minR2} window={window}"
    got = hip.ld_decay(MODES[mode_key][0], T.Filters(minR2=minR2), range_bp, n_bins, **args)
    assert_decay(got[0], got[1], wn, ws, fl, what)
    assert int(got[0].sum()) == n_counting
    if own:
        assert_equals_own_records(hip, MODES[mode_key][0], T.Filters(minR2=minR2), p, r, range_bp, n_bins, got, what, **args)
    return got, (wn, ws, fl, n_counting)


# ---- 1: iid data, the smoke() set: one LDS word for all lanes, a few bins, a bin per column, the cap -----------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("n_bins", [1, 10, 300, 4096])
def test_decay_random_300x1000(hip, n_bins, mode_key):
    got, (wn, _, _, n_counting) = check(hip, "random", mode_key, RANGE, n_bins)
    # unique positions on one contig: every record counts
    assert got[2] == 300 * 299 // 2 and int(got[0].sum()) == n_counting == len(oracle("random", mode_key)[0]) > 44000
    if n_bins == 300:
        assert (wn[1:299] > 0).all() and wn[0] == 0                  # width 100 = the spacing: a row's columns each in a bin of their own
    if n_bins == 4096:
        assert int((wn > 0).sum()) < 4096 // 4                       # width 7: most bins are empty


# ---- 2: missing genotypes: masked planes, the default mode's passes over regrouped sets, flipped pairs ----------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_decay_with_missing(hip, mode_key):
    check(hip, "missing", mode_key, 12000, 24)


# ---- 3: real LD -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("N", [64, 250, 128, 1000])
def test_decay_haplotype_blocks(hip, N, mode_key):
    got, (wn, ws, _, n_counting) = check(hip, f"mosaic{N}", mode_key, 14000, 14)
    assert n_counting > 1000
    if N == 1000:          # real decay: close pairs are in stronger LD than distant ones
        n, s, _ = got
        live = np.nonzero(n)[0]
        assert live[0] < live[-1] and s[live[0]] / n[live[0]] > s[live[-1]] / n[live[-1]]


# ---- 4: positions of the test's own: duplicates, two contigs, a populated clamp bin ------------------------------------------------
def irregular_positions(M=300, split=170):
    rng = np.random.default_rng(4)
    gaps = rng.choice([0, 1, 3, 50, 5000], size=M)
    rid = (np.arange(M) >= split).astype(np.int64)
    pos = np.zeros(M, dtype=np.int64)
    for c in (0, 1):
        sel = rid == c
        pos[sel] = 1000 + np.cumsum(gaps[sel])
    return pos, rid


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_decay_irregular_positions_and_two_contigs(hip, mode_key):
    pos, rid = irregular_positions()
    range_bp, n_bins = 20000, 40
    assert (np.diff(pos[rid == 0]) >= 0).all() and (np.diff(pos[rid == 1]) >= 0).all() and pos[169] - pos[0] > 2 * range_bp
    ia, ib, _, _ = oracle("random", mode_key)
    d = np.abs(pos[ia] - pos[ib])
    same = rid[ia] == rid[ib]
    n_dup, n_cross, n_beyond = int((same & (d == 0)).sum()), int((~same).sum()), int((same & (d >= range_bp)).sum())
    print(f"-{mode_key}: {len(ia)} oracle records, {n_dup} at one position, {n_cross} across contigs, {n_beyond} at or beyond the range")
    assert n_dup > 0 and n_cross > 0 and n_beyond > 0
    got, (wn, _, _, n_counting) = check(hip, "random", mode_key, range_bp, n_bins, pos=pos, rid=rid)
    assert n_counting == len(ia) - n_dup - n_cross
    assert wn[n_bins - 1] >= n_beyond > 0 and int(got[0][n_bins - 1]) == int(wn[n_bins - 1])


# ---- 5: thresholds and calc's window ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("minR2", [0.2, 0.8])
def test_decay_threshold(hip, minR2, mode_key):
    # no record of the unthresholded run lies within 1e-6 relative of the cut-off: the pair set cannot depend on the last bits of r2
    all_r2 = oracle("mosaic1000", mode_key)[2]
    assert not (np.abs(all_r2 - minR2) <= 1e-6 * minR2).any()
    _, (_, _, _, n_counting) = check(hip, "mosaic1000", mode_key, 14000, 14, minR2=minR2)
    assert 0 < n_counting == int((all_r2 >= minR2).sum())


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_decay_window(hip, mode_key):
    got, (wn, _, _, n_counting) = check(hip, "random", mode_key, RANGE, 300, window=2000)
    assert 0 < n_counting < 300 * 21 and not wn[21:].any() and (wn[1:21] > 0).all()


# ---- 6: geometry and determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_decay_is_the_same_bytes_for_any_tiling_and_repeat(hip, mode_key):
    mode, f = MODES[mode_key][0], T.Filters(minR2=0.0)
    check(hip, "random", mode_key, RANGE, 100, tile_variants=128)          # (uploads; the tiled call against the oracle and its own records)
    hip.timing_reset()
    tiled = hip.ld_decay(mode, f, RANGE, 100, tile_variants=128)
    assert hip.timing()["count_launches"] >= 5          # the decay call's own launches: diagonal and rectangular
    hip.timing_reset()
    single = hip.ld_decay(mode, f, RANGE, 100)
    assert hip.timing()["count_launches"] == 1
    again = hip.ld_decay(mode, f, RANGE, 100)
    for other, what in ((single, "a single launch"), (again, "a second call")):
        assert tiled[0].tobytes() == other[0].tobytes() and tiled[1].tobytes() == other[1].tobytes() and tiled[2] == other[2], what
    assert int(tiled[0].sum()) > 44000 and (tiled[1] > 0).all()


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_decay_shards_add_up(hip, mode_key):
    mode, f = MODES[mode_key][0], T.Filters(minR2=0.0)
    (n1, s1, p1), _ = check(hip, "mosaic250", mode_key, 14000, 14, own=False)
    parts = [hip.ld_decay(mode, f, 14000, 14, part=k, n_parts=3) for k in range(3)]
    assert sum(p[2] for p in parts) == p1 and sum(1 for p in parts if p[0].any()) >= 2          # (shards begin on multiples of 64 rows: one of 140 is empty)
    assert np.array_equal(np.sum([p[0] for p in parts], axis=0, dtype=np.uint64), n1)
    np.testing.assert_allclose(parts[0][1] + parts[1][1] + parts[2][1], s1, rtol=1e-12, atol=0)


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_decay_rectangle(hip, mode_key):
    al = alleles("random")
    pos, rid = positions(al.shape[0])
    util.upload(hip, al)
    mode, f = MODES[mode_key][0], T.Filters(minR2=0.0)
    geom = dict(a0=50, nA=100, b0=150, nB=150, triangle=False)
    got = hip.ld_decay(mode, f, RANGE, 60, **geom)
    assert got[2] == 100 * 150
    nrec = assert_equals_own_records(hip, mode, f, pos, rid, RANGE, 60, got, f"rectangle -{mode_key}", **geom)
    assert int(got[0].sum()) == nrec > 10000
    wn, ws, fl, _ = oracle_decay("random", mode_key, pos, rid, RANGE, 60, inside=lambda ia, ib: (ia >= 50) & (ia < 150) & (ib >= 150) & (ib < 300))
    assert_decay(got[0], got[1], wn, ws, fl, f"rectangle -{mode_key}")


# ---- 7: arguments -------------------------------------------------------------------------------------------------------------------
def test_decay_refuses_bad_arguments_and_leaves_the_engine_usable(hip):
    import ctypes as C
    with T.HipLd(0) as fresh:          # nothing uploaded yet
        with pytest.raises(T.HipError) as ei:
            fresh.ld_decay(T.MODE_AUTO, T.Filters(minR2=0.0), RANGE, 10, nA=1, nB=1)
        assert ei.value.code == E_STATE
    al = alleles("missing")
    pos, rid = positions(al.shape[0])
    util.upload(hip, al)
    f = T.Filters(minR2=0.0)
    good = hip.ld_decay(T.MODE_AUTO, f, 12000, 24)
    assert_equals_own_records(hip, T.MODE_AUTO, f, pos, rid, 12000, 24, good, "before the refused calls")

    def raw(n_ptr, s_ptr):
        fc = f._c()
        npairs = C.c_uint64(0)
        return hip._lib.twk_hip_ld_decay(hip._ctx, T.MODE_AUTO, C.byref(fc), 0, 120, 0, 120, 1, 0, 1, 0, 0, 0, 12000, 24, n_ptr, s_ptr, C.byref(npairs))

    n = np.zeros(24, dtype=np.uint64)
    s = np.zeros(24, dtype=np.float64)
    refused = [("minP < 1", lambda: hip.ld_decay(T.MODE_AUTO, T.Filters(minR2=0.0, minP=0.5), 12000, 24)),
               ("n_bins == 0", lambda: hip.ld_decay(T.MODE_AUTO, f, 12000, 0)),
               ("n_bins > 4096", lambda: hip.ld_decay(T.MODE_AUTO, f, 12000, 4097)),
               ("range_bp < n_bins", lambda: hip.ld_decay(T.MODE_AUTO, f, 23, 24)),
               ("a slice beyond the last variant", lambda: hip.ld_decay(T.MODE_AUTO, f, 12000, 24, a0=100, nA=21, b0=100, nB=21))]
    for what, call in refused:
        with pytest.raises(T.HipError) as ei:
            call()
        assert ei.value.code == E_INVALID, what
        again = hip.ld_decay(T.MODE_AUTO, f, 12000, 24)
        assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes(), what
    for what, rc in (("n NULL", raw(None, s.ctypes.data)), ("sum_r2 NULL", raw(n.ctypes.data, None))):
        assert rc == E_INVALID, what
        again = hip.ld_decay(T.MODE_AUTO, f, 12000, 24)
        assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes(), what
    assert raw(n.ctypes.data, s.ctypes.data) == 0 and n.tobytes() == good[0].tobytes() and s.tobytes() == good[1].tobytes()
    # range_bp == n_bins is the smallest range: a width of 1
    one = hip.ld_decay(T.MODE_AUTO, f, 24, 24)
    assert_equals_own_records(hip, T.MODE_AUTO, f, pos, rid, 24, 24, one, "width 1")
    assert int(one[0][:23].sum()) == 0 and int(one[0][23]) == int(good[0].sum())


# ---- 8: decay among the other kinds of the reduce path, on one context ----------------------------------------------------------------
def test_decay_between_calls_of_other_kinds_on_one_context(hip):
    """The order decay, region, score, decay, matrix, decay with tile_variants = 128 - more launches a call than the pipeline has slots,
    so every slot's argument block is reused by kinds whose parameter blocks differ in size: each call returns the bytes it returns alone."""
    al = big_data_set("missing")
    f = T.Filters(minR2=0.2)
    calls = {"decay": lambda e: e.ld_decay(T.MODE_AUTO, f, 50000, 500, tile_variants=128),
             "region": lambda e: e.ld_all(T.MODE_AUTO, f, tile_variants=128),
             "score": lambda e: e.ld_score(T.MODE_AUTO, f, tile_variants=128),
             "matrix": lambda e: e.ld_matrix(T.MODE_AUTO, f, T.STAT_R, -2.0, tile_variants=128)}
    alone = {}
    for kind, call in calls.items():
        with T.HipLd(0) as fresh:
            util.upload(fresh, al)
            fresh.timing_reset()
            alone[kind] = blob(call(fresh))
            assert fresh.timing()["count_launches"] >= 5, kind
    util.upload(hip, al)
    for step, kind in enumerate(("decay", "region", "score", "decay", "matrix", "decay")):
        assert blob(calls[kind](hip)) == alone[kind], f"step {step}: {kind}"
    n = np.frombuffer(alone["decay"][:500 * 8], dtype=np.uint64)
    assert int(n.sum()) > 1000 and int((n > 0).sum()) > 50


# ---- 9: the command line ----------------------------------------------------------------------------------------------------------------
def test_lddecay_cli(hip, tmp_path):
    al = alleles("random")
    M = al.shape[0]
    pos, rid = positions(M)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos.astype(np.uint32), rid.astype(np.uint32), phased=np.ones(M, np.uint8), n_contigs=1, block_size=50)
    r = subprocess.run([hostlib.CLI_PATH, "lddecay", "-i", twk, "-p", "-d", "30000", "-b", "10"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert any(l.startswith("##tomahawk_lddecayVersion=") for l in head) and any(l.startswith("##mode=phased") for l in head)
    assert "##range=30000,bins=10,width=3000,pairs=" in "\n".join(head)
    body = [l for l in lines if not l.startswith("#")]
    assert body[0].split("\t") == ["From", "To", "Mean", "Frequency", "Sum"]
    rows = [l.split("\t") for l in body[1:] if l]
    assert len(rows) == 10
    assert [(int(x[0]), int(x[1])) for x in rows] == [(3000 * b, 3000 * (b + 1)) for b in range(10)]
    util.upload(hip, al)
    n, s, _ = hip.ld_decay(T.MODE_PHASED, T.Filters(minR2=0.0), 30000, 10)
    assert int(n.sum()) > 44000
    freq = np.array([int(x[3]) for x in rows], dtype=np.uint64)
    total = np.array([float(x[4]) for x in rows], dtype=np.float64)
    mean = np.array([float(x[2]) for x in rows], dtype=np.float64)
    assert np.array_equal(freq, n)
    assert total.tobytes() == s.tobytes()                             # 17 significant digits: the text round-trips
    assert mean.tobytes() == (s / n.astype(np.float64)).tobytes()     # (every bin is populated here)
