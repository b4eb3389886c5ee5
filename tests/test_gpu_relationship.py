"""The sample relationship matrix (twk_hip_relationship, `tomahawk relationship`): sample by sample instead of variant by variant.

The definition, checked literally (include/twk_hip.h): over the variants in use at which both samples of a pair are non-missing, n, ibs0
({g_a, g_b} = {0, 2}), ibs2 (g_a == g_b), hethet, het_a, het_b - exact integers - and one IEEE double division of them per statistic;
`fill`, bit for bit, where the denominator is 0.  The oracle is numpy, restated here from 0/1 matrices [variants, samples] of non-missing
(V), het (H), hom-alt (Q) and hom-ref (R) genotypes:  n = V'V, hethet = H'H, ibs0 = R'Q + Q'R, ibs2 = R'R + H'H + Q'Q, het_a = H'V, het_b
its transpose.  The reference's own `relationship` is no parity target (it skips the first sample of every run, scores het/het two ways,
leaves column 0 empty and divides by the number of variants whatever is missing); its numbers are not reproduced.

Shapes (samples x variants) are the smallest that cross each boundary of the device code: the 64-lane ballot and the 16-sample raw word
(3 x 63, 17 x 64, 16 x 65), the 1024-variant chunk and two tiles of plane rows (43 x 3 = 129 rows x 1023, 44 x 1024, with missing data),
exactly one tile (64 x 2 = 128 rows), more than one chunk (129 x 1025), and a cohort-shaped set (300 x 2100 with missing data)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from tests import util
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

STATS = (T.REL_IBS, T.REL_IBS0, T.REL_KING)
FIELDS = ("n", "ibs0", "ibs2", "hethet", "het_a", "het_b")


def u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the oracle --------------------------------------------------------------------------------------------------------------------------
def oracle_counts(al):
    """alleles int8 [M, N, 2] in {0, 1, 2 = missing} -> dict of int64 [N, N]."""
    miss = (al == 2).any(axis=2)
    g = (al == 1).sum(axis=2)
    V = ~miss
    H, Q, R = V & (g == 1), V & (g == 2), V & (g == 0)
    f = lambda X: X.astype(np.float64)                                # (products below 2^53: the float matmul is exact)
    mm = lambda A, B: np.rint(f(A).T @ f(B)).astype(np.int64)
    hh = mm(H, H)
    het_a = mm(H, V)
    return dict(n=mm(V, V), ibs0=mm(R, Q) + mm(Q, R), ibs2=mm(R, R) + hh + mm(Q, Q), hethet=hh, het_a=het_a, het_b=het_a.T.copy())


def oracle_stat(c, stat, fill):
    if stat == T.REL_IBS:
        num, den = c["n"] + c["ibs2"] - c["ibs0"], 2 * c["n"]
    elif stat == T.REL_IBS0:
        num, den = c["ibs0"], c["n"]
    else:
        num, den = c["hethet"] - 2 * c["ibs0"], c["het_a"] + c["het_b"]
    out = np.full(num.shape, fill, dtype=np.float64)
    ok = den != 0
    out[ok] = num[ok] / den[ok]                                        # numpy's true division of the same integers
    return out


def assert_counts(cnt, want, where=""):
    for k in FIELDS:
        assert np.array_equal(cnt[k].astype(np.int64), want[k]), (where, k)


# ---- the data sets: made once, shared, never changed ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dataset(name):
    if name == "cohort300":
        al = util.random_alleles(2100, 300, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    elif name == "mosaic130":
        al = util.mosaic_alleles(1100, 130, 5003, miss_rate=0.05, miss_variants=0.3)
    elif name == "list70":
        al = util.random_alleles(3100, 70, 77, miss_rate=0.1, miss_variants=0.25)
    else:
        n, m, missing = name
        al = util.random_alleles(m, n, 1000 + 7 * n + m, miss_rate=0.15, miss_variants=0.4) if missing else util.random_alleles(m, n, 1000 + 7 * n + m)
    al.setflags(write=False)
    return al, oracle_counts(al)


SHAPES = [(1, 1, False), (2, 1, False), (3, 63, False), (17, 64, False), (16, 65, False), (43, 1023, True), (44, 1024, True),
          (64, 1024, False), (129, 1025, False), "cohort300"]


# ---- 1, 2: counts exact, statistics bit for bit, the plane form ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "%dx%d%s" % (s[0], s[1], "m" if s[2] else ""))
def test_counts_equal_the_oracle_and_statistics_equal_numpys_division_bit_for_bit(hip, shape):
    al, want = dataset(shape)
    M, N, _ = al.shape
    util.upload(hip, al)
    missing = bool((al == 2).any())
    assert missing == (shape == "cohort300" or (not isinstance(shape, str) and shape[2]))
    for stat in STATS:
        out, cnt = hip.relationship(stat=stat, fill=np.nan, want_counts=True)
        assert out.shape == (N, N) and cnt.shape == (N, N)
        assert_counts(cnt, want, (shape, stat))
        exp = oracle_stat(want, stat, np.nan)
        same = u64(out) == u64(exp)
        assert same.all(), (shape, stat, int((~same).sum()), out[~same][:4], exp[~same][:4])
        assert hip.relationship_last()["planes_per_sample"] == (3 if missing else 2)
    # the diagonal is a pair like any other
    d = np.arange(N)
    assert np.array_equal(cnt["ibs2"][d, d], cnt["n"][d, d]) and not cnt["ibs0"][d, d].any()
    assert np.array_equal(cnt["hethet"][d, d], cnt["het_a"][d, d]) and np.array_equal(cnt["het_a"][d, d], cnt["het_b"][d, d])
    # the matrix without the counts, and the counts without the matrix, are the same bytes
    assert u64(hip.relationship(stat=T.REL_KING)).tobytes() == u64(out).tobytes()
    buf = np.zeros((N, N), dtype=T.REL_COUNTS_DTYPE)
    rc = hip._lib.twk_hip_relationship(hip._ctx, None, 0, 0, N, 0, N, T.REL_KING, C.c_double(0.0), None, 0, buf.ctypes.data, N, None)
    assert rc == 0 and buf.tobytes() == cnt.tobytes()
    last = hip.relationship_last()
    assert last["plane_bytes"] > 0 and last["plane_bytes"] % (128 * 32 * 4) == 0 and last["transpose_ms"] >= 0


def test_the_cohort_set_is_what_the_issue_measured_on_the_cpu():
    """What the oracle gives on the two larger sets, pinned so that a change of the generators cannot hollow the tests out."""
    _, c = dataset("cohort300")
    assert len(np.unique(c["n"])) == 96 and (c["n"] > 0).all() and (c["het_a"] + c["het_b"] > 0).all()
    king = oracle_stat(c, T.REL_KING, np.nan)
    off = king[~np.eye(300, dtype=bool)]
    assert -0.095 < off.min() < -0.085 and 0.065 < off.max() < 0.075 and (np.diag(king) == 0.5).all()          # "between -0.09 and 0.07"
    # (the mosaic with the generator's default founders, switch and mutation rates: strongly structured, KING far below zero)
    _, c = dataset("mosaic130")
    king = oracle_stat(c, T.REL_KING, np.nan)
    assert c["ibs0"].min() == 0 and c["ibs0"].max() > 100 and king.min() < -0.4 and king[~np.eye(130, dtype=bool)].max() > 0.2
    assert (c["het_a"] + c["het_b"] > 0).all() and (c["n"] > 0).all()


def test_a_list_that_leaves_the_only_variant_with_missing_genotypes_out_runs_with_two_planes(hip):
    al = util.random_alleles(200, 40, 5).copy()
    al[117, [3, 17, 39], :] = 2
    util.upload(hip, al)
    out, cnt = hip.relationship(stat=T.REL_IBS, want_counts=True)
    assert hip.relationship_last()["planes_per_sample"] == 3
    assert_counts(cnt, oracle_counts(al))
    keep = np.array([v for v in range(200) if v != 117], dtype=np.uint32)
    out, cnt = hip.relationship(stat=T.REL_IBS, variants=keep, want_counts=True)
    assert hip.relationship_last()["planes_per_sample"] == 2
    want = oracle_counts(al[keep])
    assert_counts(cnt, want)
    assert (cnt["n"] == 199).all() and np.array_equal(u64(out), u64(oracle_stat(want, T.REL_IBS, np.nan)))


# ---- 3: a variant list --------------------------------------------------------------------------------------------------------------------
def test_every_third_variant_from_37_equals_the_oracle_on_those_rows(hip):
    al, _ = dataset("list70")
    util.upload(hip, al)
    ids = 37 + 3 * np.arange(1000)
    want = oracle_counts(al[ids])
    for stat in STATS:
        out, cnt = hip.relationship(stat=stat, variants=ids, want_counts=True)
        assert_counts(cnt, want, stat)
        assert np.array_equal(u64(out), u64(oracle_stat(want, stat, np.nan))), stat
    assert hip.relationship_last()["planes_per_sample"] == 3 and (al[ids] == 2).any()
    # ... and not the matrix over all of them
    assert not np.array_equal(cnt["n"].astype(np.int64), dataset("list70")[1]["n"])


# ---- 4: rectangles ------------------------------------------------------------------------------------------------------------------------
def test_rectangles_written_through_ld_give_the_bytes_of_the_square_call(hip):
    al, want = dataset("cohort300")
    N = 300
    util.upload(hip, al)
    square, sq_cnt = hip.relationship(stat=T.REL_KING, want_counts=True)
    LD, SENT = 320, -12345.678
    whole = np.full((N, LD), SENT, dtype=np.float64)
    cnts = np.zeros((N, LD), dtype=T.REL_COUNTS_DTYPE)
    cnts["n"] = 0xABCDEF
    npairs = C.c_uint64(0)
    for a0 in range(0, N, 50):
        for b0 in range(0, N, 70):
            nb = min(70, N - b0)
            rc = hip._lib.twk_hip_relationship(hip._ctx, None, 0, a0, 50, b0, nb, T.REL_KING, C.c_double(np.nan),
                                               whole[a0:, b0:].ctypes.data, LD, cnts[a0:, b0:].ctypes.data, LD, C.byref(npairs))
            assert rc == 0 and npairs.value == (50 * 51 // 2 if (a0 == b0 and nb == 50) else 50 * nb)
    assert whole[:, :N].tobytes() == square.tobytes() and cnts[:, :N].tobytes() == sq_cnt.tobytes()
    assert (whole[:, N:] == SENT).all() and (cnts["n"][:, N:] == 0xABCDEF).all()
    # one block into a fresh array: nothing outside the block is touched - the columns beyond nSB keep the sentinel
    one = np.full((N, LD), SENT, dtype=np.float64)
    rc = hip._lib.twk_hip_relationship(hip._ctx, None, 0, 100, 50, 140, 70, T.REL_IBS, C.c_double(np.nan), one[100:, 140:].ctypes.data, LD, None, 0, None)
    assert rc == 0
    inside = np.zeros((N, LD), dtype=bool)
    inside[100:150, 140:210] = True
    assert (one[~inside] == SENT).all()
    assert np.array_equal(u64(one[100:150, 140:210]), u64(oracle_stat(want, T.REL_IBS, np.nan)[100:150, 140:210]))
    # a square on the diagonal that is not the whole matrix, through the binding
    blk, bc = hip.relationship(stat=T.REL_KING, sA0=37, nSA=129, sB0=37, nSB=129, want_counts=True)
    assert blk.tobytes() == np.ascontiguousarray(square[37:166, 37:166]).tobytes() and bc.tobytes() == np.ascontiguousarray(sq_cnt[37:166, 37:166]).tobytes()


# ---- 5: zero denominators -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [np.nan, -7.0], ids=["nan", "-7"])
def test_zero_denominators_receive_the_fill_bit_for_bit_and_their_counts_are_still_right(hip, fill):
    al = util.random_alleles(500, 40, 11).copy()
    al[:, 5, :] = 2                       # sample 5: missing everywhere
    al[:, 8, :] = 0                       # samples 8 and 9: never heterozygous, never opposite homozygotes -
    al[:, 9, :] = 0                       # hom-ref at the odd variants, hom-alt at the even ones, both alike
    al[::2, 8, :] = 1
    al[::2, 9, :] = 1
    util.upload(hip, al)
    want = oracle_counts(al)
    assert (want["n"][5] == 0).all() and want["het_a"][8, 9] + want["het_b"][8, 9] == 0 and want["ibs0"][8, 9] == 0 and want["n"][8, 9] == 500
    fill_bits = u64(np.array([fill]))[0]
    for stat in STATS:
        out, cnt = hip.relationship(stat=stat, fill=fill, want_counts=True)
        assert_counts(cnt, want, stat)
        exp = oracle_stat(want, stat, fill)
        assert np.array_equal(u64(out), u64(exp)), stat
        assert (u64(out)[5, :] == fill_bits).all() and (u64(out)[:, 5] == fill_bits).all()
        if stat == T.REL_KING:
            assert u64(out)[8, 9] == fill_bits and u64(out)[9, 8] == fill_bits and u64(out)[8, 8] == fill_bits
        else:
            assert out[8, 9] == (1.0 if stat == T.REL_IBS else 0.0)
        assert np.isfinite(out[np.ix_([0, 1, 2], [0, 1, 2])]).all()
    # a NaN with a payload travels unchanged
    payload = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]
    buf = np.zeros((40, 40), dtype=np.float64)
    rc = hip._lib.twk_hip_relationship(hip._ctx, None, 0, 0, 40, 0, 40, T.REL_KING, C.c_double(payload), buf.ctypes.data, 40, None, 0, None)
    assert rc == 0 and u64(buf)[5, 0] == 0x7FF8000000ABCDEF and u64(buf)[8, 9] == 0x7FF8000000ABCDEF


# ---- 6: planted relatives -----------------------------------------------------------------------------------------------------------------
def test_planted_duplicate_and_child(hip):
    rng = np.random.default_rng(99)
    al = util.random_alleles(3000, 24, 123, maf_lo=0.2, maf_hi=0.5).copy()
    al[:, 20] = al[:, 3]                                               # 20: a duplicate of 3
    pick_a, pick_b = rng.integers(0, 2, 3000), rng.integers(0, 2, 3000)
    v = np.arange(3000)
    al[:, 21, 0] = al[v, 6, pick_a]                                    # 21: a child of 6 and 7, one haplotype of each
    al[:, 21, 1] = al[v, 7, pick_b]
    util.upload(hip, al)
    king, cnt = hip.relationship(stat=T.REL_KING, want_counts=True)
    assert_counts(cnt, oracle_counts(al))
    assert king[3, 20] == 0.5 and king[20, 3] == 0.5 and cnt["ibs0"][3, 20] == 0
    assert cnt["ibs0"][21, 6] == 0 and cnt["ibs0"][21, 7] == 0 and cnt["ibs0"][6, 21] == 0
    assert 0.2 < king[21, 6] < 0.3 and 0.2 < king[21, 7] < 0.3          # first degree: 0.25
    assert cnt["ibs0"][6, 7] > 0 and cnt["ibs0"][1, 2] > 0 and abs(king[6, 7]) < 0.06 and abs(king[1, 2]) < 0.06      # unrelated
    ibs0 = hip.relationship(stat=T.REL_IBS0)
    assert ibs0[3, 20] == 0.0 and ibs0[21, 6] == 0.0 and ibs0[1, 2] > 0.02


# ---- 7: repeats and neighbours ------------------------------------------------------------------------------------------------------------
def test_two_calls_return_the_same_bytes_and_the_record_path_is_untouched(hip):
    al, _ = dataset("mosaic130")
    util.upload(hip, al)
    f = T.Filters(minR2=0.05)
    recs0, np0, nr0 = hip.ld_region(T.MODE_AUTO, f, 0, 600, 0, 600, True)
    score0 = hip.ld_score(T.MODE_AUTO, T.Filters(minR2=0.0), 0, 400, 0, 400, True)
    opts0 = {k: hip.get_option(k) for k in ("fused", "three", "lists", "skip_pad", "count_min_chunks")}
    a, ca = hip.relationship(stat=T.REL_KING, want_counts=True)
    b, cb = hip.relationship(stat=T.REL_KING, want_counts=True)
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    ids = np.arange(5, 1100, 2)
    assert hip.relationship(stat=T.REL_IBS, variants=ids).tobytes() == hip.relationship(stat=T.REL_IBS, variants=ids).tobytes()
    recs1, np1, nr1 = hip.ld_region(T.MODE_AUTO, f, 0, 600, 0, 600, True)
    score1 = hip.ld_score(T.MODE_AUTO, T.Filters(minR2=0.0), 0, 400, 0, 400, True)
    assert nr0 > 1000 and (np0, nr0) == (np1, nr1) and recs0.tobytes() == recs1.tobytes()
    assert score0[0].tobytes() == score1[0].tobytes() and score0[1].tobytes() == score1[1].tobytes() and score0[2] == score1[2]
    assert opts0 == {k: hip.get_option(k) for k in opts0}
    # the timing counters: one count launch and one epilogue a call here (130 samples: one super-tile)
    hip.timing_reset()
    hip.relationship(stat=T.REL_KING)
    tm = hip.timing()
    assert tm["count_launches"] == 1 and tm["stats_launches"] == 1 and tm["count_ms"] > 0 and tm["stats_ms"] > 0
    assert tm["row_pairs"] == 10 * 128 * 128          # 130 x 3 = 390 plane rows: 4 x 4 tiles, the 10 on or above the diagonal


@pytest.mark.parametrize("n,missing", [(2740, True), (4100, False)], ids=["2740x3planes", "4100x2planes"])
def test_more_samples_than_one_super_tile_holds(hip, n, missing):
    """A super-tile is at most 8,192 plane rows an axis: 2,730 samples of three planes, 4,096 of two.  Ten and four samples more make
    three super-tiles of a square call - two on the diagonal and the rectangle between them, whose pairs all fill both (a, b) and (b, a) -
    and two by two of a rectangle; the count matrix is reused from one to the next."""
    al = util.random_alleles(40, n, 4242 + n, miss_rate=0.2, miss_variants=0.5) if missing else util.random_alleles(40, n, 4242 + n)
    util.upload(hip, al)
    want = oracle_counts(al)
    hip.timing_reset()
    for stat in STATS:
        out = hip.relationship(stat=stat)
        assert np.array_equal(u64(out), u64(oracle_stat(want, stat, np.nan))), stat
    assert hip.relationship_last()["planes_per_sample"] == (3 if missing else 2)
    assert hip.timing()["count_launches"] == 3 * len(STATS)
    # a rectangle across the super-tile edge, with its counts
    a0, na, b0, nb = n - 200, 150, 0, n
    hip.timing_reset()
    out, cnt = hip.relationship(stat=T.REL_KING, sA0=a0, nSA=na, sB0=b0, nSB=nb, want_counts=True)
    assert hip.timing()["count_launches"] == 2
    for k in FIELDS:
        assert np.array_equal(cnt[k].astype(np.int64), want[k][a0:a0 + na, b0:b0 + nb]), k
    assert np.array_equal(u64(out), u64(oracle_stat(want, T.REL_KING, np.nan)[a0:a0 + na, b0:b0 + nb]))


def test_the_count_kernels_work_order_changes_nothing(hip, opt):
    """The engine's own test hooks on the shared count kernel: tiles split along K into units that add into zeroed tiles
    (count_min_chunks = 1: the 3 chunks of 2,100 variants are split too) and the zero padding contracted as well (skip_pad = 0)."""
    al, want = dataset("cohort300")
    util.upload(hip, al)
    a, ca = hip.relationship(stat=T.REL_KING, want_counts=True)
    assert_counts(ca, want)
    for key, value in (("count_min_chunks", 1), ("skip_pad", 0)):
        opt.set(key, value)
        b, cb = hip.relationship(stat=T.REL_KING, want_counts=True)
        assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes(), key


# ---- 8: argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(hip):
    al = util.random_alleles(120, 50, 3, miss_rate=0.1, miss_variants=0.3)
    util.upload(hip, al)
    before = hip.relationship(stat=T.REL_KING)
    lib, ctx = hip._lib, hip._ctx
    out = np.full((50, 50), 42.0)
    cnt = np.zeros((50, 50), dtype=T.REL_COUNTS_DTYPE)
    ids = np.arange(0, 120, 2, dtype=np.uint32)

    def call(variants=None, n_use=0, sA0=0, nSA=50, sB0=0, nSB=50, stat=T.REL_KING, o=out, ld=50, c=None, ldc=0):
        return lib.twk_hip_relationship(ctx, None if variants is None else variants.ctypes.data, n_use, sA0, nSA, sB0, nSB, stat, C.c_double(0.0),
                                        None if o is None else o.ctypes.data, ld, None if c is None else c.ctypes.data, ldc, None)

    assert call(o=None, c=None) == -1                                   # both outputs NULL
    assert call(ld=49) == -1 and call(o=None, c=cnt, ldc=49) == -1 and call(c=cnt, ldc=49) == -1          # ld / ld_counts too small
    assert call(nSA=0) == -1 and call(nSB=0) == -1                      # an empty slice
    assert call(sA0=1) == -1 and call(sB0=40, nSB=11) == -1 and call(sA0=50, nSA=1) == -1 and call(sA0=0xFFFFFFFF, nSA=2) == -1      # out of range
    assert call(variants=ids, n_use=0) == -1                            # an empty list
    for bad in (np.array([3, 3, 5]), np.array([3, 7, 5]), np.array([0, 119, 120]), np.array([0xFFFFFFFF])):
        b = bad.astype(np.uint32)
        assert call(variants=b, n_use=len(b)) == -1, bad               # not strictly ascending / beyond the last variant
    assert call(stat=3) == -1 and call(stat=-1) == -1                   # an unknown statistic
    assert (out == 42.0).all() and not cnt["n"].any()
    assert call(variants=ids, n_use=len(ids)) == 0 and call(o=None, c=cnt, ldc=50) == 0          # ... and the same calls, well formed
    for kw in (dict(stat=7), dict(nSA=0), dict(sA0=10, nSA=41), dict(variants=[5, 4])):
        with pytest.raises(T.HipError) as ei:
            hip.relationship(**kw)
        assert ei.value.code == -1, kw
    # before a problem is set: TWK_HIP_E_STATE
    with T.HipLd(0) as fresh:
        assert lib.twk_hip_relationship(fresh._ctx, None, 0, 0, 50, 0, 50, T.REL_KING, C.c_double(0.0), out.ctypes.data, 50, None, 0, None) == -5
        assert fresh.relationship_last()["planes_per_sample"] == 0
    assert hip.relationship(stat=T.REL_KING).tobytes() == before.tobytes()


# ---- 9: the command -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mosaic_twk(tmp_path_factory):
    al, _ = dataset("mosaic130")
    M = al.shape[0]
    path = str(tmp_path_factory.mktemp("relationship") / "in.twk")
    hostlib.write_twk(path, np.array(al), 1000 + 100 * np.arange(M), np.zeros(M, np.uint32), phased=np.ones(M, np.uint8), n_contigs=1, block_size=50)
    return path


def _text_matrix(text):
    return np.array([[float(x) for x in line.split("\t")] for line in text.splitlines()], dtype=np.float64)


@pytest.mark.parametrize("stat_name,stat", [("king", T.REL_KING), ("ibs", T.REL_IBS), ("ibs0", T.REL_IBS0)])
def test_relationship_cli(hip, tmp_path, mosaic_twk, stat_name, stat):
    al, want = dataset("mosaic130")
    util.upload(hip, al)
    m = hip.relationship(stat=stat, fill=np.nan)
    assert np.array_equal(u64(m), u64(oracle_stat(want, stat, np.nan)))
    flags = [] if stat == T.REL_KING else ["-s", stat_name]          # king is the default
    r = subprocess.run([hostlib.CLI_PATH, "relationship", "-i", mosaic_twk] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = _text_matrix(r.stdout)
    assert got.shape == (130, 130) and np.array_equal(u64(got), u64(m))          # 17 significant digits: the text parses back to the same bits
    assert all(len(line.split("\t")) == 130 for line in r.stdout.splitlines())
    prefix = str(tmp_path / "out")
    r = subprocess.run([hostlib.CLI_PATH, "relationship", "-i", mosaic_twk, "-o", prefix] + flags, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    raw = open(prefix + ".npy", "rb").read()
    hlen = int.from_bytes(raw[8:10], "little")
    assert raw[:8] == b"\x93NUMPY\x01\x00" and (10 + hlen) % 64 == 0
    assert "'descr': '<f8', 'fortran_order': False, 'shape': (130, 130)" in raw[10:10 + hlen].decode("latin1")
    npy = np.load(prefix + ".npy")
    assert npy.dtype == np.float64 and npy.tobytes() == m.tobytes() and not os.path.exists(prefix + ".tsv")
    assert open(prefix + ".samples.tsv").read().splitlines() == ["S%d" % s for s in range(130)]          # the header's names
    prefix_t = str(tmp_path / "text")
    r = subprocess.run([hostlib.CLI_PATH, "relationship", "-i", mosaic_twk, "-o", prefix_t, "-T"] + flags, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert np.array_equal(u64(_text_matrix(open(prefix_t + ".tsv").read())), u64(m)) and not os.path.exists(prefix_t + ".npy")
    assert open(prefix_t + ".samples.tsv").read().splitlines() == ["S%d" % s for s in range(130)]


def test_relationship_cli_intervals_and_fill(hip, tmp_path, mosaic_twk):
    """-I selects whole blocks (of 50 variants here), as every command does: positions 23,500 - 48,500 are the variants 225 .. 475, the
    blocks 4 .. 9, the variants 200 .. 499; a second interval adds block 20."""
    al, _ = dataset("mosaic130")
    util.upload(hip, al)
    r = subprocess.run([hostlib.CLI_PATH, "relationship", "-i", mosaic_twk, "-I", "1:23500-48500", "-s", "ibs"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = np.arange(200, 500)
    m = hip.relationship(stat=T.REL_IBS, variants=ids)
    assert np.array_equal(u64(_text_matrix(r.stdout)), u64(m)) and np.array_equal(u64(m), u64(oracle_stat(oracle_counts(al[ids]), T.REL_IBS, np.nan)))
    r = subprocess.run([hostlib.CLI_PATH, "relationship", "-i", mosaic_twk, "-I", "1:23500-48500", "-I", "1:102500-103000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ids = np.concatenate([np.arange(200, 500), np.arange(1000, 1050)])
    assert np.array_equal(u64(_text_matrix(r.stdout)), u64(hip.relationship(stat=T.REL_KING, variants=ids)))
    # a fill: one sample missing everywhere
    al2 = np.array(al[:300])
    al2[:, 7, :] = 2
    twk = str(tmp_path / "miss.twk")
    hostlib.write_twk(twk, al2, 1000 + 100 * np.arange(300), np.zeros(300, np.uint32), phased=np.ones(300, np.uint8), n_contigs=1, block_size=50)
    prefix = str(tmp_path / "fill")
    r = subprocess.run([hostlib.CLI_PATH, "relationship", "-i", twk, "-f", "-7", "-o", prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    npy = np.load(prefix + ".npy")
    util.upload(hip, al2)
    assert npy.tobytes() == hip.relationship(stat=T.REL_KING, fill=-7.0).tobytes() and (npy[7] == -7.0).all() and (npy[:, 7] == -7.0).all()
    r = subprocess.run([hostlib.CLI_PATH, "relationship", "-i", twk], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[7].split("\t") == ["nan"] * 130, r.stderr          # the default fill
