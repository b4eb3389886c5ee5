"""Every genotype table of a small sample count (tests/util.small_table_alleles), on the CPU: the generator lays out the tables
it says it does, and the oracle's verdicts on them are pinned - which tables get a record at all is decided by edge rules on
small integers (fewer than 5 alleles, D == 0, the cubic's admissible roots, round() in front of Fisher's test) that cohort
data only meets by accident.  tests/test_gpu_small_tables.py holds the engine to the same verdicts."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import util

# (kind, n, missing) -> tables, records at minR2 = 0, records out of the cubic, records with the multiple-root flag (bit 5)
SETS = {("unphased", 6, False): (3003, 2574, 1194, 198),
        ("unphased", 8, False): (12870, 12237, 6337, 575),
        ("phased", 20, False): (1771, 1614, 0, 0),
        ("phased", 24, False): (2925, 2732, 0, 0),
        ("unphased", 6, True): (3003, 2574, 1194, 198)}


def oracle_counts(kind, data, mask, k, N):
    mA = None if mask is None else mask[2 * k]
    mB = None if mask is None else mask[2 * k + 1]
    if kind == "unphased":
        return O.count_unphased(data[2 * k], mA, data[2 * k + 1], mB, N)
    return O.count_phased(data[2 * k], mA, data[2 * k + 1], mB, N)[[0, 2, 1, 3]]         # [n00, n10, n01, n11] -> table order


@pytest.mark.parametrize("kind,n,missing", list(SETS))
@pytest.mark.parametrize("seed", [None, 11])
def test_generated_pairs_hold_the_designed_tables(kind, n, missing, seed):
    al, variants, tables = util.small_table_alleles(kind, n, seed=seed, missing=missing)
    T = SETS[(kind, n, missing)][0]
    N = (n if kind == "unphased" else n // 2) + (2 if missing else 0)
    assert tables.shape == (T, 9 if kind == "unphased" else 4) and al.shape == (2 * T, N, 2) and al.dtype == np.int8
    assert (tables >= 0).all() and (tables.sum(axis=1) == n).all() and len(np.unique(tables, axis=0)) == T
    assert (variants["rid"] == 0).all() and np.array_equal(variants["pos"][0::2], 1000 + 10 * np.arange(T))
    assert np.array_equal(variants["pos"][1::2], variants["pos"][0::2] + 1)
    data, mask = O.bitvectors_from_alleles(al)
    assert (mask is not None) == missing
    for k in range(T):
        assert np.array_equal(oracle_counts(kind, data, mask, k, N), tables[k]), (k, tables[k])
    if missing:          # one sample missing in A only, one in B only, every variant
        miss = (al == 2).all(axis=2)
        assert ((al == 2).any(axis=2) == miss).all() and (miss.sum(axis=1) == 1).all()
        assert not (miss[0::2] & miss[1::2]).any() and (variants["an"] == 2).all() and variants["gt_missing"].all()
    if seed is None:
        first = np.zeros(tables.shape[1], dtype=np.int64); first[-1] = n
        assert np.array_equal(tables[0], first) and np.array_equal(tables[-1], first[::-1])
    else:                # the same tables in another order, the same genotypes in other samples
        al0, _, tables0 = util.small_table_alleles(kind, n, missing=missing)
        assert not np.array_equal(tables, tables0)
        assert np.array_equal(tables[np.lexsort(tables.T[::-1])], tables0[np.lexsort(tables0.T[::-1])])
        assert not np.array_equal(al, al0) and np.array_equal(np.sort(variants["ac"]), np.sort((al0 == 1).sum(axis=(1, 2))))


def oracle_records(kind, n, missing=False, keep_low_ac=True, seed=None, minR2=0.0):
    """-> (tables, [record or None per table]) as orc_pair treats the pair of each table in the mode of its kind."""
    al, variants, tables = util.small_table_alleles(kind, n, seed=seed, missing=missing)
    data, mask = O.bitvectors_from_alleles(al)
    N = al.shape[1]
    st = O.settings(minR2=minR2, phased=(kind == "phased"), unphased=(kind == "unphased"), keep_low_ac=keep_low_ac)
    recs = [O.pair(data[2 * k], None if mask is None else mask[2 * k], variants[2 * k],
                   data[2 * k + 1], None if mask is None else mask[2 * k + 1], variants[2 * k + 1], N, st) for k in range(len(tables))]
    return tables, variants, recs


@pytest.mark.parametrize("kind,n,missing", list(SETS))
def test_the_oracles_record_counts_are_pinned(kind, n, missing):
    """How many tables get a record at minR2 = 0, how many of those come out of the cubic and how many carry the multiple-root
    flag: measured once, pinned here.  The low-AC skip (ac_A + ac_B <= 2) takes nothing that the fewer-than-5 rules leave."""
    T, n_rec, n_cubic, n_bit5 = SETS[(kind, n, missing)]
    tables, variants, recs = oracle_records(kind, n, missing)
    ctrl = np.array([int(r["controller"]) for r in recs if r is not None])
    assert (len(tables), len(ctrl), int((ctrl & 1 == 0).sum()), int((ctrl >> 5 & 1).sum())) == (T, n_rec, n_cubic, n_bit5)
    assert not (ctrl[ctrl & 1 == 1] >> 5 & 1).any()
    # the pair as the oracle treats it is the math on the table's own counts
    st = O.settings(minR2=0.0, phased=(kind == "phased"), unphased=(kind == "unphased"), keep_low_ac=True)
    for k in range(T):
        A, B = variants[2 * k], variants[2 * k + 1]
        r = O.unphased_math(tables[k], A, B, st) if kind == "unphased" else O.phased_math(tables[k][[0, 2, 1, 3]], A, B, st)
        assert (r is None) == (recs[k] is None) and (r is None or r.tobytes() == recs[k].tobytes()), k
    _, variants2, skip = oracle_records(kind, n, missing, keep_low_ac=False)
    low = (variants2["ac"][0::2] + variants2["ac"][1::2]) <= 2
    assert low.sum() > 0 and all(r is None for r, l in zip(skip, low) if l)
    assert [r is None for r in skip] == [r is None or bool(l) for r, l in zip(recs, low)]
    assert sum(r is not None for r in skip) == n_rec


@pytest.mark.parametrize("n,want", [(12, 0), (16, 0), (20, 8), (24, 8)])
def test_zero_d_tables_that_the_reference_reports(n, want):
    """Polymorphic 2 x 2 tables with n00 n11 == n01 n10 have D = 0 exactly, and PhasedMath drops a pair whose
    pA qB - qA pB is 0 (ld_engine.cpp:1194).  In doubles that difference is rounding noise for 8 such tables of 20 haplotypes
    and 8 of 24, none of 12 or 16: the reference writes a record with r2 ~ 1e-33 for them, and every consumer that counts
    records inherits it."""
    tables, variants, recs = oracle_records("phased", n)
    n00, n01, n10, n11 = tables.T
    poly = (n10 + n11 > 0) & (n10 + n11 < n) & (n01 + n11 > 0) & (n01 + n11 < n)
    zero = poly & (n00 * n11 == n01 * n10)
    assert zero.sum() == {12: 17, 16: 17, 20: 33, 24: 53}[n]
    got = [k for k in np.nonzero(zero)[0] if recs[k] is not None]
    assert len(got) == want
    for k in got:
        assert 0 < recs[k]["R2"] < 1e-30 and abs(recs[k]["D"]) < 1e-16 and recs[k]["P"] == 1.0
    # ... and a monomorphic table never gets a record
    assert all(recs[k] is None for k in np.nonzero(~poly)[0])


def all_2x2(n):
    return util.compositions(n, 4)


def test_the_oracles_fisher_p_is_the_exact_one():
    """kt_fisher_exact as the oracle restates it against exact rational arithmetic on every 2 x 2 table of 12, 16 and 20:
    measured 8.4e-15 at worst over the 3,195 tables, held to 1e-12."""
    worst, n_tables = 0.0, 0
    for n in (12, 16, 20):
        for t in all_2x2(n):
            t = [int(x) for x in t]
            want = float(util.exact_fisher_p(*t))
            got = O.fisher(*t)[2]
            worst = max(worst, abs(got - want) / want)
            n_tables += 1
    print(f"Fisher's P, oracle against exact: worst relative difference {worst:.3g} over {n_tables} tables")
    assert n_tables == 3195 and worst <= 1e-12


@pytest.mark.parametrize("n,missing,n_ill,share", [(6, False, 35, 0.012), (8, False, 72, 0.006), (6, True, 35, 0.012)])
def test_the_ill_conditioned_class_is_small(n, missing, n_ill, share):
    """The tables the GPU parity test holds to less than the 1e-6 bar - a double root of the cubic, or a root whose own
    conditioning would need a floor beyond DX_CEILING - are named from the tables alone and are few: 35 of 3,003 at n = 6,
    72 of 12,870 at n = 8.  A change to the classifier cannot widen the exclusion past these shares."""
    al, variants, tables = util.small_table_alleles("unphased", n, missing=missing)
    data, mask = O.bitvectors_from_alleles(al)
    ill = util.small_table_ill_conditioned(tables, variants, util.double_root_vetter(data, mask, variants, al.shape[1]))
    print(f"n = {n}{' + missing' if missing else ''}: {int(ill.sum())} of {len(tables)} tables ill-conditioned ({ill.mean():.4%})")
    assert ill.sum() <= share * len(tables) and not ill[tables[:, 4] == 0].any()
    assert ill.sum() == n_ill


@pytest.mark.parametrize("n,missing,want,share", [(6, False, {"zero-D": 28, "zero-D+half": 64}, 0.031),
                                                  (8, False, {"zero-D": 126, "zero-D+half": 300, "half": 32}, 0.036),
                                                  (6, True, {"zero-D": 28, "zero-D+half": 64}, 0.031)])
def test_the_exactly_known_roots_are_named_and_few(n, missing, want, share):
    """Small tables sit far more often than cohort data where parity's relative bar has nothing to hold on to: the cubic's root
    is pA pB exactly (D = 0: the record's D is rounding noise) or makes every expected count end in .5 (round() in front of
    Fisher's test is decided by the root's last bit).  Both are decided in rational arithmetic from the table alone
    (util.small_table_exact_root): 92 of 3,003 tables at n = 6 and 458 of 12,870 at n = 8 (20 of those also ill-conditioned).  The GPU
    test holds them to a bar of their own in place of the parity checker's counted exemptions; the class cannot grow past these
    shares unseen.  The oracle itself keeps |D| below D_FLOOR on every zero-D table and its counts within DX_CEILING * total of .5
    on every half table - by construction of the class, asserted here so that the construction stays that."""
    from collections import Counter
    al, variants, tables = util.small_table_alleles("unphased", n, missing=missing)
    cls = util.small_table_exact_class(tables, variants)
    assert dict(Counter(cls.values())) == want and len(cls) <= share * len(tables)
    assert all(tables[k, 4] > 0 for k in cls)
    st = O.settings(minR2=0.0, unphased=True, keep_low_ac=True)
    for k, kind in cls.items():
        r = O.unphased_math(tables[k], variants[2 * k], variants[2 * k + 1], st)
        if "zero-D" in kind:
            assert abs(r["D"]) <= util.D_FLOOR and r["R2"] <= 1e-20, (k, tables[k], r["D"])
        if "half" in kind:
            assert np.all(np.abs(r["cnt"] - np.floor(r["cnt"]) - 0.5) <= util.DX_CEILING * np.sum(r["cnt"])), (k, tables[k], r["cnt"])
    # no other table's record is that close to D = 0, the ill-conditioned ones aside: the class is all of them
    data, mask = O.bitvectors_from_alleles(al)
    ill = util.small_table_ill_conditioned(tables, variants, util.double_root_vetter(data, mask, variants, al.shape[1]))
    for k in np.nonzero((tables[:, 4] > 0) & ~ill)[0]:
        if int(k) not in cls:
            r = O.unphased_math(tables[k], variants[2 * k], variants[2 * k + 1], st)
            assert r is None or abs(r["D"]) > 1e-9, (k, tables[k], r["D"])
