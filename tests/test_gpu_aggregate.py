"""LD aggregate (twk_hip_ld_aggregate, `tomahawk ldaggregate`): the pairwise LD of a region rasterised into x-by-y cells, binned and
summed exactly on the GPU.

Every variant has a bin on the x axis and one on the y axis (0xFFFF: off the landscape on that axis).  For every pair (A, B) `calc`
reports a record for, the statistic v - signed r (copysign(R, D)), r2, D or D' - is added to cell (bin_x[A], bin_y[B]) and to cell
(bin_x[B], bin_y[A]), each orientation if both of its bins are valid.  Per cell: n, the contributions; sum, the sum of q / 2^32 with
q = rint(v * 2^32); sum_sq, the sum of q2 / 2^32 with q2 = rint((v * v) * 2^32); min and max of q / 2^32, 0.0 in an empty cell.

"Own records, exactly": ld_region's records for the same arguments are binned here in integers by that definition; all five arrays
must be BIT-IDENTICAL - the sums are exact in integers, whatever the tiling, the order and the bin layout.

"Oracle aggregate": the records of oracle.all_pairs (the pinned restatement of the reference) with minP = 1, taken ONCE per (data set,
mode, cut-off) and binned in numpy (sums in extended precision, so that the reference's own summation error is far below the bar).
The bars are derived, not measured.  A record's value is held to the record path's bar (tests/test_gpu_matrix.py, tests/util.py)

    e(record) = RTOL |v| + floor_stat(record)        RTOL = 1e-6; floor: cubic_floors of the record's root error, 0 off the cubic

and the engine adds rint(v * 2^32) / 2^32, at most Q = 2^-33 from its own v.  Hence, per cell,

    |sum - want|       <= sum over the cell of e(record) + n Q
    |sum_sq - want_sq| <= sum over the cell of (2 |v| e + e^2 + 2^-53 v^2) + n Q
                          (d(v^2) = 2 |v| dv, its second-order term, the rounding of the one double multiplication; q2 is
                          rint of that product, again at most Q away)
    |min - want_min|, |max - want_max| <= the largest e(record) + Q of the cell
                          (every value moves by at most its own e + Q, so an extreme moves by at most the largest of them)

and n must be equal in every cell.  The data sets are ones on which tests/test_gpu_ldscore.py shows that engine and oracle report the
same pair set; they are tests/test_gpu_decay.py's and tests/test_gpu_clump.py's, imported, not edited.
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import FIELD, MODES, RTOL, STATS, alleles, bins_every_seventh_random, bins_monotone, blob, monotone, oracle_records, positions, stat_of
from tests.reduce_cases import data_set as big_data_set
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5
Q_STEP = 2.0 ** -33
OFF = 0xFFFF
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
STAT_IDS = {T.STAT_R: "r", T.STAT_R2: "r2", T.STAT_D: "D", T.STAT_DPRIME: "Dprime"}


# ---- bin assignments (monotone and every-seventh-random: reduce_cases) -------------------------------------------------------------------------------------------------------------------
def bins_permuted(M, X, Y, seed=11):
    rng = np.random.default_rng(seed)
    return monotone(M, X)[rng.permutation(M)], monotone(M, Y)[rng.permutation(M)]


def bins_some_off(M, X, Y):
    bx, by = bins_monotone(M, X, Y)
    v = np.arange(M)
    bx[v % 5 == 1] = OFF          # off on x only
    by[v % 7 == 2] = OFF          # off on y only (and on both where the two meet)
    bx[v % 11 == 4] = OFF; by[v % 11 == 4] = OFF
    assert ((bx == OFF) & (by != OFF)).any() and ((bx != OFF) & (by == OFF)).any() and ((bx == OFF) & (by == OFF)).any()
    return bx, by


def bins_one_cell(M, X, Y):
    return np.full(M, X - 2, dtype=np.uint16), np.full(M, Y // 2, dtype=np.uint16)


# name -> (x_bins, y_bins, assignment)
CASES = {"a-5x5": (5, 5, bins_monotone), "a-7x13": (7, 13, bins_monotone), "a-1x1": (1, 1, bins_monotone), "a-64x64": (64, 64, bins_monotone),
         "a-4096x4096": (4096, 4096, bins_monotone),
         "b-7x13": (7, 13, bins_permuted), "b-300x300": (300, 300, bins_permuted),
         "c-5x5": (5, 5, bins_every_seventh_random), "c-7x13": (7, 13, bins_every_seventh_random), "c-1x1": (1, 1, bins_every_seventh_random),
         "c-64x64": (64, 64, bins_every_seventh_random), "c-4096x4096": (4096, 4096, bins_every_seventh_random),
         "d-off": (9, 6, bins_some_off), "e-one-cell": (5, 7, bins_one_cell)}


# ---- the definition, in integers ---------------------------------------------------------------------------------------------------------
def contributions(ia, ib, bx, by, Y):
    """Both orientations of every record -> (cell index, record index) of the contributions whose two bins are valid."""
    bx, by = bx.astype(np.int64), by.astype(np.int64)
    k = np.arange(len(ia))
    c1, ok1 = bx[ia] * Y + by[ib], (bx[ia] != OFF) & (by[ib] != OFF)
    c2, ok2 = bx[ib] * Y + by[ia], (bx[ib] != OFF) & (by[ia] != OFF)
    return np.concatenate([c1[ok1], c2[ok2]]), np.concatenate([k[ok1], k[ok2]])


def aggregate_of_records(recs, stat, bx, by, X, Y):
    """The engine's own records binned on the host in integers -> the five arrays, each (X, Y)."""
    v = stat_of(recs, stat).astype(np.float64)
    q = np.rint(v * 4294967296.0).astype(np.int64)                   # (the product is exact: a power of two)
    q2 = np.rint((v * v) * 4294967296.0).astype(np.int64)            # (one double multiplication, then exact)
    cell, k = contributions(recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64), bx, by, Y)
    n = np.bincount(cell, minlength=X * Y).astype(np.uint64)
    # |q|, q2 <= 2^32 + a few and fewer than 2^20 contributions: the int64 sums are exact
    S, S2 = np.zeros(X * Y, dtype=np.int64), np.zeros(X * Y, dtype=np.int64)
    lo, hi = np.full(X * Y, I64_MAX, dtype=np.int64), np.full(X * Y, I64_MIN, dtype=np.int64)
    np.add.at(S, cell, q[k]); np.add.at(S2, cell, q2[k])
    np.minimum.at(lo, cell, q[k]); np.maximum.at(hi, cell, q[k])
    out = [np.zeros(X * Y, dtype=np.float64) for _ in range(4)]
    for c in np.nonzero(n)[0]:                                       # Python integers: one correctly rounded conversion each
        out[0][c] = float(int(S[c])) / 2 ** 32
        out[1][c] = float(int(S2[c])) / 2 ** 32
        out[2][c] = float(int(lo[c])) / 2 ** 32
        out[3][c] = float(int(hi[c])) / 2 ** 32
    return tuple(a.reshape(X, Y) for a in [n] + out)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def assert_equals_own_records(hip, mode, filters, stat, bx, by, X, Y, got, what, recs_of=None, a0=0, nA=None, b0=0, nB=None, triangle=True, **kw):
    M = hip.n_variants
    nA = M - a0 if nA is None else nA
    nB = M - b0 if nB is None else nB
    recs, npairs = recs_of() if recs_of else hip.ld_region(mode, filters, a0, nA, b0, nB, triangle, **kw)[:2]
    want = aggregate_of_records(recs, stat, bx, by, X, Y)
    assert got[5] == npairs, what
    for name, g, w in zip(("n", "sum", "sum_sq", "min", "max"), got[:5], want):
        assert g.shape == (X, Y) and g.dtype == (np.uint64 if name == "n" else np.float64), f"{what}: {name}"
        assert same_bits(g, w), f"{what}: {name} differs from the own records' at cells {np.argwhere(g.view(np.uint64) != w.view(np.uint64))[:6].tolist()}"
    return len(recs), want


# ---- 1: own records, exactly ---------------------------------------------------------------------------------------------------------------
OWN_RECORDS = {}


def own_records(hip, name, mode_key):
    """ld_region's records of the uploaded set, once per (set, mode)."""
    key = (name, mode_key)
    if key not in OWN_RECORDS:
        M = hip.n_variants
        recs, npairs, _ = hip.ld_region(MODES[mode_key][0], T.Filters(minR2=0.0), 0, M, 0, M, True)
        recs.setflags(write=False)
        OWN_RECORDS[key] = (recs, npairs)
    return OWN_RECORDS[key]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("stat", STATS, ids=[STAT_IDS[s] for s in STATS])
@pytest.mark.parametrize("name,mode_key", [("random", "p"), ("random", "u"), ("missing", "auto")])
def test_aggregate_equals_own_records_binned_in_integers(hip, name, mode_key, stat, case):
    al = alleles(name)
    M = al.shape[0]
    X, Y, assign = CASES[case]
    bx, by = assign(M, X, Y)
    util.upload(hip, al)
    got = hip.ld_aggregate(MODES[mode_key][0], T.Filters(minR2=0.0), bx, by, X, Y, stat)
    what = f"{name} -{mode_key} {FIELD[stat]} {case}"
    nrec, (n, s, _, lo, hi) = assert_equals_own_records(hip, MODES[mode_key][0], T.Filters(minR2=0.0), stat, bx, by, X, Y, got, what,
                                                        recs_of=lambda: own_records(hip, name, mode_key))
    populated = int((n > 0).sum())
    print(f"{what}: {nrec} records, {int(n.sum())} contributions in {populated} of {X * Y} cells, sums {s.min():.6g}..{s.max():.6g}")
    assert nrec > 1000
    if case[0] in "ab" and X * Y > 1:
        assert populated > 1
    if case == "e-one-cell":
        assert populated == 1 and int(n[X - 2, Y // 2]) == 2 * nrec
    if case in ("a-1x1", "a-5x5", "b-7x13", "c-64x64"):
        assert int(n.sum()) == 2 * nrec                  # every variant on the landscape: two contributions a record
    if case == "d-off":
        assert 0 < int(n.sum()) < 2 * nrec
    if name == "random" and stat in (T.STAT_R, T.STAT_D) and populated >= 25:          # iid data: a cell's sum takes either sign
        assert (s < 0).any() and (s > 0).any() and (lo < 0).any() and (hi > 0).any()          # signed sums: through the arithmetic-shift split
    if stat == T.STAT_R2:
        assert (lo >= 0).all()


# ---- 2: against the oracle -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(name, mode_key, minR2=0.0):
    """-> (ia, ib, records, {stat: floor per record}) of the oracle's records of the set, each pair once (ia < ib in file order): computed
    once, never changed."""
    al = alleles(name)
    N = al.shape[1]
    data, mask = O.bitvectors_from_alleles(al)
    variants = O.variants_from_alleles(al)
    ia, ib, want = oracle_records(data, mask, variants, N, mode_key, minR2)
    root_error = util.double_root_vetter(data, mask, variants, N).root_error
    floors = {stat: np.zeros(len(want), dtype=np.float64) for stat in STATS}
    for k in np.nonzero((want["controller"] & 1) == 0)[0]:              # out of the cubic (tests/test_gpu_matrix.py oracle_matrix)
        w = want[k]
        total = float(np.sum(w["cnt"]))
        dx = util.D_FLOOR
        if total > 0:
            dx = min(max(dx, util.ROOT_ERROR_FACTOR * root_error(int(ia[k]), int(ib[k]), float(w["cnt"][0]) / total)[0]), util.DX_CEILING)
        fl = util.cubic_floors([float(x) for x in w["cnt"]], w["R"], dx)
        for stat in STATS:
            floors[stat][k] = fl[FIELD[stat]]
    for a in (ia, ib, want, *floors.values()):
        a.setflags(write=False)
    return ia, ib, want, floors


def oracle_aggregate(name, mode_key, stat, bx, by, X, Y, minR2=0.0, keep=None):
    """-> n, sum, sum_sq, min, max as the definition gives them from the oracle's records, and the three bars, each flat [X * Y]."""
    ia, ib, recs, floors = oracle(name, mode_key, minR2)
    v = stat_of(recs, stat).astype(np.float64)
    e = RTOL * np.abs(v) + floors[stat]
    if keep is not None:
        sel = keep(ia, ib)
        ia, ib, v, e = ia[sel], ib[sel], v[sel], e[sel]
    cell, k = contributions(ia, ib, bx, by, Y)
    n = np.bincount(cell, minlength=X * Y).astype(np.uint64)
    s, s2 = np.zeros(X * Y, dtype=np.longdouble), np.zeros(X * Y, dtype=np.longdouble)
    np.add.at(s, cell, v[k].astype(np.longdouble)); np.add.at(s2, cell, (v[k].astype(np.longdouble)) ** 2)
    lo, hi = np.full(X * Y, np.inf), np.full(X * Y, -np.inf)
    np.minimum.at(lo, cell, v[k]); np.maximum.at(hi, cell, v[k])
    lo[n == 0] = 0.0; hi[n == 0] = 0.0
    bar, bar2, bar_x = np.zeros(X * Y), np.zeros(X * Y), np.zeros(X * Y)
    np.add.at(bar, cell, e[k])
    np.add.at(bar2, cell, 2 * np.abs(v[k]) * e[k] + e[k] ** 2 + 2.0 ** -53 * v[k] ** 2)
    np.maximum.at(bar_x, cell, e[k])
    nq = n.astype(np.float64) * Q_STEP
    return (n, s.astype(np.float64), s2.astype(np.float64), lo, hi), (bar + nq, bar2 + nq, np.where(n > 0, bar_x + Q_STEP, 0.0)), len(ia)


def assert_aggregate(got, want, bars, what):
    n, s, s2, lo, hi = (a.reshape(-1) for a in got[:5])
    wn, ws, ws2, wlo, whi = want
    bad_n = np.nonzero(n != wn)[0]
    assert len(bad_n) == 0, f"{what}: n differs at cells {bad_n[:8].tolist()}: got {n[bad_n[:8]].tolist()} want {wn[bad_n[:8]].tolist()}"
    margins = []
    for name, g, w, bar in (("sum", s, ws, bars[0]), ("sum_sq", s2, ws2, bars[1]), ("min", lo, wlo, bars[2]), ("max", hi, whi, bars[2])):
        err = np.abs(g - w)
        worst = int(np.argmax(err - bar))
        margins.append(f"{name}: cell {worst} diff {err[worst]:.3g} bar {bar[worst]:.3g}")
        assert (err <= bar).all(), f"{what}: {name} beyond the bar at cells {np.nonzero(err > bar)[0][:8].tolist()} ({margins[-1]})"
    print(f"{what}: {int(wn.sum())} contributions in {int((wn > 0).sum())} of {len(wn)} cells; closest to the bar - " + "; ".join(margins))


def check(hip, name, mode_key, stat, X, Y, assign=bins_monotone, minR2=0.0, window=None, pos=None, **kw):
    """Upload the set; the call against the oracle and against the engine's own records."""
    al = alleles(name)
    M = al.shape[0]
    p, r = positions(M, pos)
    util.upload(hip, al, pos=p.astype(np.uint32), rid=r.astype(np.uint32))
    bx, by = assign(M, X, Y)
    args = dict(kw)
    keep = None
    if window is not None:
        args.update(window=T.OPT_WINDOW, l_window=window)
        keep = lambda ia, ib: np.abs(p[ia] - p[ib]) <= window
    mode, f = MODES[mode_key][0], T.Filters(minR2=minR2)
    what = f"{name} -{mode_key} {FIELD[stat]} {X}x{Y} {assign.__name__} minR2={minR2} window={window}"
    got = hip.ld_aggregate(mode, f, bx, by, X, Y, stat, **args)
    want, bars, nrec = oracle_aggregate(name, mode_key, stat, bx, by, X, Y, minR2, keep)
    assert_aggregate(got, want, bars, what)
    assert_equals_own_records(hip, mode, f, stat, bx, by, X, Y, got, what, **args)
    return got, want, nrec


@pytest.mark.parametrize("stat", STATS, ids=[STAT_IDS[s] for s in STATS])
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_aggregate_iid_against_the_oracle(hip, mode_key, stat):
    got, want, nrec = check(hip, "random", mode_key, stat, 7, 13)
    assert got[5] == 300 * 299 // 2 and nrec > 44000 and int(got[0].sum()) == 2 * nrec
    check(hip, "random", mode_key, stat, 300, 300, assign=bins_permuted)          # the direct path against the oracle too


@pytest.mark.parametrize("stat", STATS, ids=[STAT_IDS[s] for s in STATS])
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("N", [250, 1000])
def test_aggregate_haplotype_blocks_against_the_oracle(hip, N, mode_key, stat):
    got, _, nrec = check(hip, f"mosaic{N}", mode_key, stat, 14, 10)
    assert nrec > 1000
    if stat == T.STAT_R2 and N == 1000:          # LD blocks: cells on the diagonal hold stronger LD than the far corner
        n, s = got[0], got[1]
        assert n[0, 0] > 0 and n[0, 9] > 0 and s[0, 0] / n[0, 0] > s[0, 9] / n[0, 9]


@pytest.mark.parametrize("stat", STATS, ids=[STAT_IDS[s] for s in STATS])
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_aggregate_with_missing_against_the_oracle(hip, mode_key, stat):
    check(hip, "missing", mode_key, stat, 12, 5)
    check(hip, "mosaic128", mode_key, stat, 5, 12, assign=bins_every_seventh_random)


@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("minR2", [0.2, 0.8])
def test_aggregate_threshold(hip, minR2, mode_key):
    all_r2 = oracle("mosaic1000", mode_key)[2]["R2"]
    assert not (np.abs(all_r2 - minR2) <= 1e-6 * minR2).any()          # the pair set cannot depend on the last bits of r2
    for stat in (T.STAT_R, T.STAT_R2):
        got, _, nrec = check(hip, "mosaic1000", mode_key, stat, 14, 14, minR2=minR2)
        assert 0 < nrec == int((all_r2 >= minR2).sum()) and int(got[0].sum()) == 2 * nrec


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_aggregate_window(hip, mode_key):
    got, want, nrec = check(hip, "random", mode_key, T.STAT_D, 30, 30, window=2000)
    n = got[0]
    assert 0 < nrec < 300 * 21
    far = np.abs(np.arange(30)[:, None] - np.arange(30)[None, :]) > 3          # ten variants a bin, twenty a window
    assert not n[far].any() and n[~far].any()


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_aggregate_rectangle(hip, mode_key):
    geom = dict(a0=50, nA=100, b0=150, nB=150, triangle=False)
    inside = lambda ia, ib: (ia >= 50) & (ia < 150) & (ib >= 150) & (ib < 300)
    al = alleles("random")
    util.upload(hip, al)
    bx, by = bins_monotone(300, 12, 9)
    mode, f = MODES[mode_key][0], T.Filters(minR2=0.0)
    for stat in (T.STAT_R, T.STAT_DPRIME):
        got = hip.ld_aggregate(mode, f, bx, by, 12, 9, stat, **geom)
        assert got[5] == 100 * 150
        want, bars, nrec = oracle_aggregate("random", mode_key, stat, bx, by, 12, 9, keep=inside)
        assert_aggregate(got, want, bars, f"rectangle -{mode_key} {FIELD[stat]}")
        own, _ = assert_equals_own_records(hip, mode, f, stat, bx, by, 12, 9, got, f"rectangle -{mode_key}", **geom)
        assert own == nrec > 10000 and int(got[0].sum()) == 2 * nrec
        # rows 50..149 are x bins 2..5 of orientation one and y bins 1..4 of orientation two; columns 150..299 the upper halves
        assert not got[0][:2, :].any() and got[0][2:6, 4:].any() and got[0][6:, 1:5].any()


# ---- 3: no order -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_aggregate_is_the_same_bytes_for_any_tiling_and_repeat(hip, mode_key):
    # (the default mode on the larger set with missing genotypes: its regrouped sets are big enough to be cut into several tiles)
    name = "big missing" if mode_key == "auto" else "random"
    al = big_data_set("missing") if mode_key == "auto" else alleles(name)
    M = al.shape[0]
    util.upload(hip, al)
    mode, f = MODES[mode_key][0], T.Filters(minR2=0.0)
    for assign, X, Y in ((bins_monotone, 40, 25), (bins_permuted, 40, 25)):
        bx, by = assign(M, X, Y)
        hip.timing_reset()
        single = hip.ld_aggregate(mode, f, bx, by, X, Y, T.STAT_R)
        launches = hip.timing()["count_launches"]
        assert launches >= 1
        assert_equals_own_records(hip, mode, f, T.STAT_R, bx, by, X, Y, single, f"{name} -{mode_key} one launch")
        for tv in (32, 100, 128):          # 32, 100: tiles narrower than a block's 256 columns, and no multiple of its 32 rows
            hip.timing_reset()
            tiled = hip.ld_aggregate(mode, f, bx, by, X, Y, T.STAT_R, tile_variants=tv)
            assert hip.timing()["count_launches"] > launches
            assert blob(tiled) == blob(single), f"tile_variants={tv}"
        assert blob(hip.ld_aggregate(mode, f, bx, by, X, Y, T.STAT_R)) == blob(single), "a second call"
    assert int(single[0].sum()) > 1000


def test_aggregate_between_calls_of_other_kinds_on_one_context(hip):
    """aggregate, region, score, aggregate, decay, matrix, aggregate with tile_variants = 128 - more launches a call than the pipeline has
    slots, so every slot's argument block is reused by kinds whose parameter blocks differ in size: each call returns the bytes it
    returns alone."""
    al = big_data_set("missing")
    M = al.shape[0]
    f = T.Filters(minR2=0.2)
    bx, by = bins_every_seventh_random(M, 50, 31)
    calls = {"aggregate": lambda e: e.ld_aggregate(T.MODE_AUTO, f, bx, by, 50, 31, T.STAT_R, tile_variants=128),
             "region": lambda e: e.ld_all(T.MODE_AUTO, f, tile_variants=128),
             "score": lambda e: e.ld_score(T.MODE_AUTO, f, tile_variants=128),
             "decay": lambda e: e.ld_decay(T.MODE_AUTO, f, 50000, 500, tile_variants=128),
             "matrix": lambda e: e.ld_matrix(T.MODE_AUTO, f, T.STAT_R, -2.0, tile_variants=128)}
    alone = {}
    for kind, call in calls.items():
        with T.HipLd(0) as fresh:
            util.upload(fresh, al)
            fresh.timing_reset()
            alone[kind] = blob(call(fresh))
            assert fresh.timing()["count_launches"] >= 5, kind
    util.upload(hip, al)
    for step, kind in enumerate(("aggregate", "region", "score", "aggregate", "decay", "matrix", "aggregate")):
        assert blob(calls[kind](hip)) == alone[kind], f"step {step}: {kind}"
    n = np.frombuffer(alone["aggregate"][:50 * 31 * 8], dtype=np.uint64)
    assert int(n.sum()) > 1000 and int((n > 0).sum()) > 50


# ---- 4: shards -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_aggregate_shards_combine(hip, mode_key):
    """n adds exactly and the extremes combine exactly.  The sums: every part's sum is the correctly rounded double of an exact integer
    sum, |part - exact part| <= 2^-53 |part|; adding three of them in double rounds twice more, each time by at most 2^-53 of a partial
    result that is at most A = the sum of the parts' magnitudes; the whole is rounded once.  So
    |parts added - whole| <= 2^-53 (sum |part| + 2 A + |whole|) <= 4 * 2^-53 * A."""
    mode, f = MODES[mode_key][0], T.Filters(minR2=0.0)
    al = alleles("mosaic250")
    M = al.shape[0]
    util.upload(hip, al)
    bx, by = bins_monotone(M, 14, 9)
    whole = hip.ld_aggregate(mode, f, bx, by, 14, 9, T.STAT_R)
    parts = [hip.ld_aggregate(mode, f, bx, by, 14, 9, T.STAT_R, part=k, n_parts=3) for k in range(3)]
    assert sum(p[5] for p in parts) == whole[5] and sum(1 for p in parts if p[0].any()) >= 2
    assert np.array_equal(np.sum([p[0] for p in parts], axis=0, dtype=np.uint64), whole[0])
    lo = np.min([np.where(p[0] > 0, p[3], np.inf) for p in parts], axis=0)
    hi = np.max([np.where(p[0] > 0, p[4], -np.inf) for p in parts], axis=0)
    live = whole[0] > 0
    assert live.any() and (whole[1] < 0).any()
    assert same_bits(np.where(live, lo, 0.0), whole[3]) and same_bits(np.where(live, hi, 0.0), whole[4])
    for k in (1, 2):
        added = parts[0][k] + parts[1][k] + parts[2][k]
        A = np.abs(parts[0][k]) + np.abs(parts[1][k]) + np.abs(parts[2][k])
        err = np.abs(added - whole[k])
        print(f"-{mode_key} {'sum' if k == 1 else 'sum_sq'}: largest |parts - whole| {err.max():.3g}, bar there {4 * 2.0 ** -53 * A.reshape(-1)[int(np.argmax(err))]:.3g}")
        assert (err <= 4 * 2.0 ** -53 * A).all()


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_aggregate_refuses_bad_arguments_and_leaves_the_engine_usable(hip):
    with T.HipLd(0) as fresh:          # nothing uploaded yet
        with pytest.raises(T.HipError) as ei:
            fresh.ld_aggregate(T.MODE_AUTO, T.Filters(minR2=0.0), np.zeros(1, np.uint16), np.zeros(1, np.uint16), 5, 5, nA=1, nB=1)
        assert ei.value.code == E_STATE
    al = alleles("missing")
    M = al.shape[0]
    util.upload(hip, al)
    f = T.Filters(minR2=0.0)
    bx, by = bins_monotone(M, 8, 6)
    good = hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 8, 6, T.STAT_R)
    assert_equals_own_records(hip, T.MODE_AUTO, f, T.STAT_R, bx, by, 8, 6, good, "before the refused calls")
    arrays = [np.zeros((8, 6), dtype=np.uint64)] + [np.zeros((8, 6), dtype=np.float64) for _ in range(4)]

    def raw(null=None, stat=T.STAT_R):
        fc = f._c()
        npairs = C.c_uint64(0)
        ptrs = [bx.ctypes.data, by.ctypes.data] + [a.ctypes.data for a in arrays]
        if null is not None:
            ptrs[null] = None
        return hip._lib.twk_hip_ld_aggregate(hip._ctx, T.MODE_AUTO, C.byref(fc), 0, M, 0, M, 1, 0, 1, 0, 0, 0, stat, ptrs[0], ptrs[1], 8, 6, *ptrs[2:], C.byref(npairs))

    def with_bin(axis, value):
        x, y = bx.copy(), by.copy()
        (x if axis == 0 else y)[17] = value
        return lambda: hip.ld_aggregate(T.MODE_AUTO, f, x, y, 8, 6, T.STAT_R)

    refused = [("minP < 1", lambda: hip.ld_aggregate(T.MODE_AUTO, T.Filters(minR2=0.0, minP=0.5), bx, by, 8, 6, T.STAT_R)),
               ("x_bins == 0", lambda: hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 0, 6)),
               ("y_bins == 0", lambda: hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 8, 0)),
               ("x_bins == 4097", lambda: hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 4097, 6)),
               ("y_bins == 4097", lambda: hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 8, 4097)),
               ("a bin_x entry == x_bins", with_bin(0, 8)), ("a bin_y entry == y_bins", with_bin(1, 6)), ("a bin_x entry 0xFFFE", with_bin(0, 0xFFFE)),
               ("an unknown stat", lambda: hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 8, 6, 4)),
               ("a negative stat", lambda: hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 8, 6, -1)),
               ("a slice beyond the last variant", lambda: hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 8, 6, a0=100, nA=21, b0=100, nB=21))]
    for what, call in refused:
        hip.timing_reset()
        with pytest.raises(T.HipError) as ei:
            call()
        assert ei.value.code == E_INVALID, what
        assert hip.timing()["count_launches"] == 0, what          # refused before any launch
        assert blob(hip.ld_aggregate(T.MODE_AUTO, f, bx, by, 8, 6, T.STAT_R)) == blob(good), what
    for k, what in enumerate(("bin_x", "bin_y", "n", "sum", "sum_sq", "min", "max")):
        hip.timing_reset()
        assert raw(null=k) == E_INVALID, f"{what} NULL"
        assert hip.timing()["count_launches"] == 0, what
    assert raw() == 0 and blob(arrays) == blob(good[:5])
    # 0xFFFF is no error: the variant is off the landscape
    one_off = with_bin(0, OFF)()
    assert 0 < int(one_off[0].sum()) < int(good[0].sum())


# ---- 6: the command line ---------------------------------------------------------------------------------------------------------------------
def landscape(pos, rid, contig_bases, X, Y):
    """tomahawk ldaggregate's landscape restated in numpy -> (bin_x, bin_y, bpx, bpy, range)."""
    present = np.unique(rid)
    if len(present) == 1:
        coord, rng = pos - pos.min(), int(pos.max() - pos.min() + 1)
    else:
        offset = np.zeros(len(contig_bases), dtype=np.int64)
        at = 0
        for k in range(len(contig_bases)):
            offset[k] = at
            if k in present:
                at += contig_bases[k]
        coord, rng = offset[rid] + pos, at
    bpx = int(np.ceil(np.float32(rng) / np.float32(X)))
    bpy = int(np.ceil(np.float32(rng) / np.float32(Y)))
    return np.minimum(coord // bpx, X - 1).astype(np.uint16), np.minimum(coord // bpy, Y - 1).astype(np.uint16), bpx, bpy, rng


def test_ldaggregate_cli(hip, tmp_path):
    al = alleles("random")
    M = al.shape[0]
    rid = (np.arange(M) >= 150).astype(np.int64)
    pos = 1000 + 1_600_000 * (np.arange(M, dtype=np.int64) % 150)          # 150 variants across each contig's 250,000,000 bases
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos.astype(np.uint32), rid.astype(np.uint32), phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    X, Y = 7, 13
    bx, by, bpx, bpy, rng = landscape(pos, rid, [250_000_000, 250_000_000], X, Y)
    assert len(np.unique(bx)) == X and len(np.unique(by)) == Y and rng == 500_000_000
    util.upload(hip, al, pos=pos.astype(np.uint32), rid=rid.astype(np.uint32))
    n, s, s2, lo, hi, _ = hip.ld_aggregate(T.MODE_PHASED, T.Filters(minR2=0.0), bx, by, X, Y, T.STAT_R)
    cnt = n.astype(np.float64)
    m_cut = int(np.median(n[n > 0]))          # cuts some populated cells and keeps others
    assert (n[n > 0] < m_cut).any() and (n >= m_cut).any()
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / cnt
        sd = np.sqrt(np.maximum(s2 / cnt - mean * mean, 0.0))
    tables = {"mean": mean, "count": cnt, "sd": sd, "max": hi}
    for red, table in tables.items():
        for m in (1, m_cut):
            r = subprocess.run([hostlib.CLI_PATH, "ldaggregate", "-i", twk, "-p", "-x", str(X), "-y", str(Y), "-s", "r", "-R", red, "-m", str(m)],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            lines = r.stdout.splitlines()
            head = [l for l in lines if l.startswith("#")]
            assert any(l.startswith("##tomahawk_ldaggregateVersion=") for l in head) and any(l.startswith("##mode=phased") for l in head)
            assert any(l.startswith(f"#x={X},y={Y},bpx={bpx},bpy={bpy},range={rng},stat=r,reduce={red},min_count={m},") for l in head), head
            assert any(l.startswith("#contig=1,rid=0,offset=0") for l in head) and any(l.startswith("#contig=2,rid=1,offset=250000000") for l in head)
            rows = [l.split("\t") for l in lines if l and not l.startswith("#")]
            assert len(rows) == X and all(len(x) == Y for x in rows)
            got = np.array([[float(x) for x in row] for row in rows], dtype=np.float64)
            want = np.where((n >= m) & (n > 0), table, 0.0)
            assert same_bits(got, want), f"-R {red} -m {m}"          # 17 significant digits: the text round-trips
            if m == m_cut:
                assert (got[(n > 0) & (n < m_cut)] == 0).all() and (want != 0).any()
