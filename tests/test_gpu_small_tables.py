"""Every genotype table of a small sample count through the engine (tests/util.small_table_alleles; the oracle's side is pinned
in tests/test_small_tables.py): one variant pair per table, a 1 bp window that holds exactly those pairs, rows of one word.
Whether a table gets a record at all is decided by edge rules on small integers - fewer than 5 alleles, ac_A + ac_B <= 2,
D == 0 (in doubles: 8 tables of 20 haplotypes have D = 0 exactly and still get a record), the cubic's admissible roots,
round() in front of Fisher's test - in d_pair, d_phased_math, d_unphased_math and the Fisher kernels (ld_math.hip.h), and by
the screens in front of them (ScreenCounts, ScreenCountsUnphased with four and three products, k_screen3_pairs: ld_count.hip.h,
ld_three.hip.h), whose zero and fixed-variant branches only degenerate tables reach.  Every form of the engine and every
consumer of its record set must give the same answer on every table."""
import functools
import time

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
WIN = dict(window=T.OPT_WINDOW, l_window=1)
KEEP = dict(window=T.OPT_WINDOW | T.OPT_KEEP_LOW_AC, l_window=1)
SETTINGS = {T.MODE_PHASED: dict(phased=True), T.MODE_UNPHASED: dict(unphased=True), T.MODE_AUTO: dict()}
# (kind, n, missing) -> the modes the set runs in, the largest share of ill-conditioned tables, of tables with an exactly known root
SETS = {("unphased", 6, False): ((T.MODE_UNPHASED, T.MODE_AUTO), 0.012, 0.031),
        ("unphased", 8, False): ((T.MODE_UNPHASED, T.MODE_AUTO), 0.006, 0.036),
        ("phased", 20, False): ((T.MODE_PHASED,), 0.0, 0.0),
        ("phased", 24, False): ((T.MODE_PHASED,), 0.0, 0.0),
        ("unphased", 6, True): ((T.MODE_PHASED, T.MODE_UNPHASED, T.MODE_AUTO), 0.012, 0.031)}
CASES = [(kind, n, missing, mode) for (kind, n, missing), (modes, _, _) in SETS.items() for mode in modes]
SEED = 20
LEDGERS = []          # what each call of the parity checker in this module returned


@functools.lru_cache(maxsize=None)
def table_set(kind, n, missing, seed):
    al, variants, tables = util.small_table_alleles(kind, n, seed=seed, missing=missing)
    data, mask = O.bitvectors_from_alleles(al)
    return dict(al=al, variants=variants, tables=tables, data=data, mask=mask, N=al.shape[1], T=len(tables))


@functools.lru_cache(maxsize=None)
def oracle_records(kind, n, missing, seed, mode):
    """The oracle's record of every table's pair in `mode` at minR2 = 0 with the low-AC skip off, computed once -> oracle records."""
    s = table_set(kind, n, missing, seed)
    st = O.settings(minR2=0.0, keep_low_ac=True, **SETTINGS[mode])
    data, mask, v = s["data"], s["mask"], s["variants"]
    recs = [O.pair(data[2 * k], None if mask is None else mask[2 * k], v[2 * k],
                   data[2 * k + 1], None if mask is None else mask[2 * k + 1], v[2 * k + 1], s["N"], st) for k in range(s["T"])]
    out = np.array([r for r in recs if r is not None], dtype=O.RECORD_DTYPE)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ill_conditioned(kind, n, missing, seed):
    s = table_set(kind, n, missing, seed)
    if kind != "unphased":
        return np.zeros(s["T"], dtype=bool), None
    vet = util.double_root_vetter(s["data"], s["mask"], s["variants"], s["N"])
    return util.small_table_ill_conditioned(s["tables"], s["variants"], vet), vet


@functools.lru_cache(maxsize=None)
def exact_class(kind, n, missing, seed):
    s = table_set(kind, n, missing, seed)
    return util.small_table_exact_class(s["tables"], s["variants"]) if kind == "unphased" else {}


def send(hip, s):
    hip.set_problem(s["N"], 2 * s["T"])
    hip.upload(s["data"], util.to_hip_meta(s["variants"]), s["mask"])


def same(a, b):
    return np.sort(a, order=ORDER).tobytes() == np.sort(b, order=ORDER).tobytes()


def partner_pairs_only(recs):
    assert (recs["idxA"] % 2 == 0).all() and (recs["idxB"] == recs["idxA"] + 1).all()
    assert len(np.unique(recs["idxA"])) == len(recs)


@pytest.fixture(scope="module", autouse=True)
def module_ledger():
    """What this module alone asked of the parity checker's exemptions (tests/util.py), added up from what its calls returned
    and printed when the module is done; the session's accounting is only read."""
    del LEDGERS[:]
    yield
    total = {}
    for ledger in LEDGERS:
        for key, x in ledger.items():
            total[key] = total.get(key, 0) + x
    print(f"\nsmall tables' own ledger over {len(LEDGERS)} calls: {total}; the session's largest floor granted so far (f11 scale) "
          f"{util.LARGEST_FLOOR['dx']:.3g} of a ceiling of {util.DX_CEILING:g}, largest part of a floor used {dict(util.FLOOR_USED) or 'none'}")


# ---- a / b: the math of every table against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [None, SEED])
@pytest.mark.parametrize("kind,n,missing,mode", CASES)
def test_every_table_gets_the_oracles_record(hip, kind, n, missing, mode, seed):
    """minR2 = 0, low-AC skip off: the engine's record of every table against the oracle's.  Records out of PhasedMath (every
    table of the phased sets and of the default mode without missing data, the unphased tables without double hets): counts
    identical, statistics within 1e-6, no floors.  Records out of the cubic fall into three classes, named on the CPU from the
    tables alone before the engine is asked:
      * ill-conditioned (a double root, or a root whose floor would pass DX_CEILING: 35 of 3,003 tables at n = 6, 72 of 12,870
        at n = 8), held to what no libm decides;
      * exactly known roots where a relative bar has nothing to hold on to (util.small_table_exact_root: D = 0 exactly, or every
        expected count ends in .5 exactly; 92 tables at n = 6, 458 at n = 8, pinned in tests/test_small_tables.py), held to
        util.assert_exact_root_record: both sides report, |D| within the root's own error, P that of the record's own rounding;
      * everything else: the parity checker's bar with the floors a record's own conditioning grants, every comparison of every
        run counted in the session's ledger.
    With the low-AC skip on, exactly the records of tables with ac_A + ac_B <= 2 go."""
    t0 = time.time()
    s = table_set(kind, n, missing, seed)
    variants, n_tables = s["variants"], s["T"]
    want = oracle_records(kind, n, missing, seed, mode)
    ill, vet = ill_conditioned(kind, n, missing, seed)
    assert ill.sum() <= SETS[(kind, n, missing)][1] * n_tables
    cubic_mode = kind == "unphased" and (mode == T.MODE_UNPHASED or (mode == T.MODE_AUTO and missing))
    assert bool(((want["controller"] & 1) == 0).any()) == cubic_mode
    t1 = time.time()
    send(hip, s)
    got, npairs, nrec = hip.ld_all(mode, T.Filters(minR2=0.0), **KEEP)
    assert npairs == n_tables and nrec == len(got)
    partner_pairs_only(got)
    pos2k = {int(p): k for k, p in enumerate(variants["pos"][0::2])}
    want_k = np.array([pos2k[int(p)] for p in want["Apos"]], dtype=np.int64)
    got_k = (got["idxA"] // 2).astype(np.int64)
    if not cubic_mode:
        ledger = util.assert_records_match(got, want, variants)
        assert ledger["cubic"] == 0 and set(ledger) == {"records", "cubic"}, ledger          # PhasedMath: no floor, no tie
    else:
        # three classes, named on the CPU before the engine is asked: ill-conditioned (below), exactly known roots where the
        # relative bar has nothing to hold on to (exact: their own explicit bar, util.assert_exact_root_record, both sides must
        # report), and everything else - through the parity checker, every comparison counted in the session's ledger
        exact = exact_class(kind, n, missing, seed)
        assert len(exact) <= SETS[(kind, n, missing)][2] * n_tables
        named = ill.copy(); named[[k for k in exact]] = True
        ledger = util.assert_records_match(got[~named[got_k]], want[~named[want_k]], variants, double_root=vet)
        LEDGERS.append(dict(ledger))
        g_by_k = {int(k): g for k, g in zip(got_k, got)}
        w_by_k = {int(k): w for k, w in zip(want_k, want)}
        n_exact = n_other_round = 0
        for k, xkind in exact.items():
            if ill[k]:
                continue
            assert (k in g_by_k) and (k in w_by_k), (k, s["tables"][k], xkind, k in g_by_k, k in w_by_k)
            w = w_by_k[k]
            dx = min(max(util.D_FLOOR, util.ROOT_ERROR_FACTOR * vet.root_error(2 * k, 2 * k + 1, float(w["cnt"][0]) / float(np.sum(w["cnt"])))[0]),
                     util.DX_CEILING)
            n_other_round += util.assert_exact_root_record(g_by_k[k], w, xkind, dx)
            n_exact += 1
        ledger["exact_root"] = n_exact; ledger["exact_root_rounded_the_other_way"] = int(n_other_round)
        w_by_k = {int(k): w for k, w in zip(want_k, want)}
        n_one_sided = 0
        for g in got[ill[got_k]]:
            k = int(g["idxA"]) // 2
            assert all(np.isfinite(g[f]).all() for f in ("cnt", "D", "Dprime", "R", "R2", "P", "ChiSqFisher", "ChiSqModel")), (k, g)
            assert 0.0 <= g["R2"] <= 1.0 + 1e-9, (k, g)
            w = w_by_k.pop(k, None)
            if w is None:
                assert vet(2 * k, 2 * k + 1), (k, s["tables"][k], g)
                n_one_sided += 1
            else:
                assert not ((int(g["flags"]) ^ int(w["controller"])) & ~(1 << 5)), (k, s["tables"][k], hex(g["flags"]), hex(w["controller"]))
        for k in w_by_k:
            if ill[k]:                          # the oracle's record of an ill-conditioned table the engine did not report
                assert vet(2 * k, 2 * k + 1), (k, s["tables"][k])
                n_one_sided += 1
        ledger["ill_conditioned"] = int(ill.sum()); ledger["one_sided"] = n_one_sided
    # the low-AC skip (ac_A + ac_B <= 2, ld_engine.cpp:1918) takes exactly the records of those tables
    got2, npairs2, _ = hip.ld_all(mode, T.Filters(minR2=0.0), **WIN)
    low = (variants["ac"][got["idxA"]].astype(np.int64) + variants["ac"][got["idxB"]]) <= 2
    assert npairs2 == n_tables and same(got2, got[~low])
    assert ((variants["ac"][0::2].astype(np.int64) + variants["ac"][1::2]) <= 2).sum() > 0
    print(f"{kind} n={n} missing={missing} mode={mode} seed={seed}: {len(got)} records of {n_tables} tables, {int(low.sum())} of them low-AC; "
          f"ledger {ledger}; oracle {t1 - t0:.2f} s, engine and comparison {time.time() - t1:.2f} s")


def test_the_zero_d_records_are_the_references(hip):
    """Of the 33 polymorphic tables of 20 haplotypes with n00 n11 == n01 n10 the reference reports 8 (its pA qB - qA pB is
    rounding noise there, not 0), of the 53 of 24 haplotypes 8, of those of 12 and 16 none: the engine reports exactly those -
    a matter of operation order and of no contraction into FMAs, nothing else."""
    for n, n_want in ((12, 0), (16, 0), (20, 8), (24, 8)):
        s = table_set("phased", n, False, None)
        want = oracle_records("phased", n, False, None, T.MODE_PHASED)
        n00, n01, n10, n11 = s["tables"].T
        poly = (n10 + n11 > 0) & (n10 + n11 < n) & (n01 + n11 > 0) & (n01 + n11 < n)
        zero = poly & (n00 * n11 == n01 * n10)
        send(hip, s)
        got, _, _ = hip.ld_all(T.MODE_PHASED, T.Filters(minR2=0.0), **KEEP)
        mine = got[zero[got["idxA"] // 2]]
        pos2k = {int(p): k for k, p in enumerate(s["variants"]["pos"][0::2])}
        theirs = want[np.array([bool(zero[pos2k[int(p)]]) for p in want["Apos"]])]
        assert len(mine) == len(theirs) == n_want and zero.sum() == {12: 17, 16: 17, 20: 33, 24: 53}[n], (n, len(mine), len(theirs))
        assert np.array_equal(np.sort(s["variants"]["pos"][mine["idxA"]]), np.sort(theirs["Apos"]))
        assert ((mine["R2"] > 0) & (mine["R2"] < 1e-30) & (mine["P"] == 1.0)).all()
        print(f"{n} haplotypes: {int(zero.sum())} polymorphic tables with D = 0, {len(mine)} reported: {s['tables'][mine['idxA'] // 2].tolist()}")


# ---- c: every form of the engine gives the same records --------------------------------------------------------------------
def forms(kind):
    for fused in (0, 1):
        for three in ((0, 2) if kind == "unphased" else (None,)):
            for wopt in (0, T.OPT_R2_SCREEN):
                yield fused, three, wopt


@pytest.mark.parametrize("kind,n,mode", [("unphased", 6, T.MODE_UNPHASED), ("phased", 20, T.MODE_PHASED)])
def test_every_form_gives_the_same_records(hip, opt, kind, n, mode):
    """The plain path, the fused count -> screen form, the three-product forms (fused, and through the (HH, S) matrix and
    k_screen3_pairs) with and without the allele-count band: at a cut-off of 1, and on, one ulp below and one ulp above r2 values
    that exist, the survivors are the records of the minR2 = 0 run with R2 >= cut, byte for byte.  1e-6 is the last cut-off
    without a screen, 2e-6 has one (its candidates may overflow to the plain path)."""
    t0 = time.time()
    s = table_set(kind, n, False, None)
    send(hip, s)
    base, _, _ = hip.ld_all(mode, T.Filters(minR2=0.0), **WIN)
    assert len(base) > 1000
    r2 = np.unique(base["R2"])
    picked = r2[np.unique(np.linspace(0, len(r2) - 1, 9).round().astype(int))]
    cuts = [1.0, 1e-6, 2e-6]
    for x in picked:
        cuts += [float(np.nextafter(x, -1.0)), float(x), float(np.nextafter(x, 2.0))]
    n_runs = 0
    for cut in cuts:
        want = base[base["R2"] >= cut]
        screened = 1e-6 < cut <= 1.0
        for fused, three, wopt in forms(kind):
            opt.set("fused", fused)
            if three is not None:
                opt.set("three", three)
            hip.timing_reset()
            got, npairs, nrec = hip.ld_all(mode, T.Filters(minR2=cut), window=T.OPT_WINDOW | wopt, l_window=1)
            tm = hip.timing()
            assert npairs == s["T"] and nrec == len(got)
            assert same(got, want), (cut, fused, three, wopt, len(got), len(want))
            # the forms asked for really ran (a cut-off the screen cannot use - 0 < cut <= 1e-6, or above 1 - leaves the plain path)
            assert (tm["fused_launches"] > 0) == (screened and fused == 1), (cut, fused, three, tm)
            if three is not None:
                assert (tm["three_launches"] > 0) == (screened and three == 2), (cut, fused, three, tm)
            n_runs += 1
    assert (base["R2"] >= 1.0).sum() > 0 and (kind != "phased" or (base["R2"] < 1e-6).sum() == 8)      # (the zero-D records)
    print(f"{kind} n={n}: {n_runs} runs over {len(cuts)} cut-offs, base {len(base)} records, {time.time() - t0:.2f} s")


# ---- d: the consumers see the same record set ------------------------------------------------------------------------------
@pytest.mark.parametrize("minR2", [0.0, 0.5])
@pytest.mark.parametrize("kind,n,mode", [("unphased", 6, T.MODE_UNPHASED), ("phased", 20, T.MODE_PHASED)])
def test_the_consumers_see_the_same_record_set(hip, kind, n, mode, minR2):
    """ld_score, ld_prune, ld_clump and ld_matrix form no records but decide pair by pair whether there would be one: on every
    table, the decision and the statistic are those of ld_all's own records - at minR2 = 0 with the 8 zero-D records of 20
    haplotypes in every count."""
    t0 = time.time()
    s = table_set(kind, n, False, None)
    M = 2 * s["T"]
    send(hip, s)
    f = T.Filters(minR2=minR2)
    base, _, _ = hip.ld_all(mode, f, **WIN)
    partner_pairs_only(base)
    full, _, _ = hip.ld_all(mode, T.Filters(minR2=0.0), **WIN)
    assert same(base, full[full["R2"] >= minR2]) and 100 < len(base) <= len(full)
    if kind == "phased" and minR2 == 0.0:
        assert (base["R2"] < 1e-30).sum() == 8
    has = np.zeros(s["T"], dtype=bool); has[base["idxA"] // 2] = True
    r2_of = np.zeros(M, dtype=np.float64)
    r2_of[base["idxA"]] = base["R2"]; r2_of[base["idxB"]] = base["R2"]
    # scores: one partner for the two variants of a table with a record, none otherwise; the sum is that record's R2
    n_partners, sum_r2, npairs = hip.ld_score(mode, f, **WIN)
    assert npairs == s["T"] and np.array_equal(n_partners, np.repeat(has, 2).astype(np.uint64))
    assert sum_r2.tobytes() == r2_of.tobytes()
    # pruning in file order: B goes exactly where the table has a record
    keep, n_kept, n_edges, npairs = hip.ld_prune(mode, f, **WIN)
    assert npairs == s["T"] and n_edges == len(base) and n_kept == M - len(base)
    assert (keep[0::2] == 1).all() and np.array_equal(keep[1::2] == 0, has)
    # clumping with P increasing in file order and both thresholds at 1: the same
    p = (np.arange(M) + 1.0) / (M + 1.0)
    index_of, n_clumps, n_members, c_edges, npairs = hip.ld_clump(mode, f, p, 1.0, 1.0, **WIN)
    assert npairs == s["T"] and c_edges == len(base) and n_clumps == n_kept and n_members == len(base)
    assert np.array_equal(index_of == np.arange(M), keep == 1)
    assert np.array_equal(index_of[1::2][has], np.arange(0, M, 2, dtype=np.uint32)[has])
    # the dense matrix: (float) R2 of the record in (2k, 2k + 1) and its mirror, the fill wherever there is none
    m, n_records, npairs = hip.ld_matrix(mode, f, stat=T.STAT_R2, fill=float("nan"), **WIN)
    assert npairs == s["T"] and n_records == len(base) and m.shape == (M, M)
    ka, kb = np.arange(0, M, 2), np.arange(1, M, 2)
    want = np.full(s["T"], np.nan, dtype=np.float32); want[base["idxA"] // 2] = base["R2"].astype(np.float32)
    assert m[ka, kb].tobytes() == want.tobytes() and m[kb, ka].tobytes() == want.tobytes()
    assert (np.diagonal(m) == 1.0).all() and int((~np.isnan(m)).sum()) == M + 2 * len(base)
    del m
    mr, n_records, _ = hip.ld_matrix(mode, f, stat=T.STAT_R, fill=float("nan"), **WIN)
    want = np.full(s["T"], np.nan, dtype=np.float32); want[base["idxA"] // 2] = np.copysign(base["R"], base["D"]).astype(np.float32)
    assert n_records == len(base) and mr[ka, kb].tobytes() == want.tobytes() and mr[kb, ka].tobytes() == want.tobytes()
    # (a guard on the set, not on the engine: the comparison above pins the sign only if the records carry both; D itself is held
    # to the oracle's in test_every_table_gets_the_oracles_record.  At minR2 = 0.5 the oracle keeps 133 / 92 records with D < 0 /
    # D > 0 of the unphased set and 103 / 87 of the phased one, so no count near a hundred can be asked of each sign)
    assert (base["D"] < 0).any() and (base["D"] > 0).any()
    print(f"{kind} n={n} minR2={minR2}: {len(base)} records, consumers agree, {time.time() - t0:.2f} s")


# ---- e: Fisher's kernels against exact arithmetic ---------------------------------------------------------------------------
def test_fishers_p_of_every_small_table_is_the_exact_one(hip):
    """twk_hip_fisher_exact on every 2 x 2 table of 1 .. 24, zero cells and zero margins included, against two-sided P in
    rational arithmetic (the sum of the probabilities of the tables at most as likely as the observed one) to rtol = 1e-8 - the
    bar test_fisher_pipeline_agrees_with_the_oracle_in_any_order holds against the oracle, which itself agrees with exact
    arithmetic to 2e-14 on these tables.  Binned and in the order given: the same bytes."""
    t0 = time.time()
    tabs = np.concatenate([util.compositions(n, 4) for n in range(1, 25)]).astype(np.int32)
    assert len(tabs) == 20474 and (tabs == 0).any(axis=1).sum() > 1000
    want = np.array([float(util.exact_fisher_p(*[int(x) for x in t])) for t in tabs])
    hip.set_problem(12, 8)
    binned, _ = hip.fisher_exact(tabs)
    as_given, _ = hip.fisher_exact(tabs, ordered=False)
    assert binned.tobytes() == as_given.tobytes()
    rel = np.abs(binned - want) / want
    print(f"Fisher's P, engine against exact: worst relative difference {rel.max():.3g} over {len(tabs)} tables "
          f"(table {tabs[int(np.argmax(rel))].tolist()}), {time.time() - t0:.2f} s")
    assert (want > 0).all() and (want <= 1).all() and (want == 1).sum() > 1000 and want.min() < 1e-6
    assert np.allclose(binned, want, rtol=1e-8, atol=0.0)
