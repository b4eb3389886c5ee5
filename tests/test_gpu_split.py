"""LD splitting (twk_hip_ld_split) against the NumPy restatement of tests/split_cases.py over the band that ld_matrix_band (r2, fill 0)
returns on the same context: total, feasible, cost and cuts EXACTLY - the call is integer arithmetic over the band's bytes, so there is no
tolerance anywhere.  Every call gets output arrays preset to a pattern, so that what the contract leaves untouched is seen to be."""
import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import split_cases as SC
from tests import util
from tests.reduce_cases import MODES, blob, data_set

pytestmark = pytest.mark.gpu

F0 = T.Filters(minR2=0.0)
PATTERN = 0xAB


def variants_of(al, two_contigs=False):
    M = al.shape[0]
    pos = np.arange(M, dtype=np.int64) * 100 + 1000
    rid = np.zeros(M, dtype=np.uint32)
    if two_contigs:
        rid[M // 2:] = 1
    return O.variants_from_alleles(al, pos=pos.astype(np.uint32), rid=rid)


def preset(k_max):
    k = max(k_max, 1)
    out = (np.zeros(1, np.uint64), np.zeros(k, np.uint8), np.zeros(k, np.uint64), np.zeros(k * (k + 1), np.uint32))
    for x in out:
        x.view(np.uint8)[:] = PATTERN
    return out


def split(hip, mode, window, min_size, max_size, k_max, filters=F0, a0=0, n=None, tile_variants=0):
    """ld_split into preset arrays -> (its result with the cost of an infeasible K as 0, the arrays' bytes); the entries the contract
    leaves untouched must still hold the pattern."""
    out = preset(k_max)
    got = hip.ld_split(mode, filters, window, min_size, max_size, k_max, a0=a0, n=n, tile_variants=tile_variants, out=out)
    total, feasible, cost, cuts = out
    word32, word64 = np.uint32(0xABABABAB), np.uint64(0xABABABABABABABAB)
    for K in range(1, k_max + 1):
        row = cuts[(K - 1) * (k_max + 1):K * (k_max + 1)]
        assert feasible[K - 1] in (0, 1)
        if feasible[K - 1]:
            assert (row[K + 1:] == word32).all()
        else:
            assert cost[K - 1] == word64 and (row == word32).all(), K
            got["cost"][K - 1] = 0
    return got, blob(out)


def check(hip, mode, window, min_size, max_size, k_max, what, filters=F0, a0=0, n=None, tile_variants=0):
    """-> (the device's result, the restatement's, the band's n_records)."""
    values, first, indptr, nrec, npairs = hip.ld_matrix_band(mode, filters, window, stat=T.STAT_R2, fill=0.0, a0=a0, n=n)
    want = SC.split_of(values, first, indptr, min_size, max_size, k_max)
    got, _ = split(hip, mode, window, min_size, max_size, k_max, filters, a0, n, tile_variants)
    print(f"{what}: n {len(first)}, band {len(values)}, sizes {min_size}..{max_size}, k_max {k_max}: feasible K {got['K']}, total {got['total'] / SC.SCALE:.6f}, "
          f"cost {[round(int(c) / SC.SCALE, 3) for c in got['cost'][:8]]}")
    SC.assert_same(got, want, what)
    assert (got["n_records"], got["n_pairs"]) == (nrec, npairs), what
    return got, want, nrec


# ---- 1: modes and data sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode_key", [("mosaic250", "p"), ("mosaic128", "u"), ("mosaic128", "auto"), ("missing", "auto"), ("missing", "u")])
def test_split_equals_the_restatement(hip, name, mode_key):
    al = data_set(name)
    util.upload(hip, al, variants_of(al))
    M = al.shape[0]
    got, _, nrec = check(hip, MODES[mode_key][0], 3000, 10, 40, 20, f"{name} -{mode_key}")
    assert nrec > 0 and got["total"] > 0 and len(got["K"]) >= 5 and min(got["K"]) == -(-M // 40)
    last = hip.split_last()
    assert last["bytes"] > 0 and last["layers_ms"] > 0 and last["sums_ms"] > 0 and last["backtrack_ms"] > 0


def test_planted_mosaic_is_cut_at_the_planted_places(hip):
    al = SC.planted_alleles()
    util.upload(hip, al, variants_of(al))
    p = SC.PLANTED
    got, _, _ = check(hip, T.MODE_PHASED, p["window"], p["min_size"], p["max_size"], p["k_max"], "planted")
    K = len(SC.PLANTED_SIZES)
    assert np.array_equal(got["cuts"][got["K"].index(K)], SC.planted_cuts())


# ---- 2: the LDS window against the workgroup, saturation, the sizes' corners ---------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 600])
def test_a_window_wider_than_a_workgroup(hip, n):
    """max_size = 300: a block of 256 b stages more than 256 entries of the layer below, and at n = 600 the layers span workgroups."""
    al = data_set("plain")
    util.upload(hip, al, variants_of(al))
    got, _, _ = check(hip, T.MODE_PHASED, 5000, 50, 300, 6, f"plain n {n}", a0=0, n=n)
    assert got["K"][0] == -(-n // 300) and len(got["K"]) >= 3


@pytest.mark.parametrize("window,what", [(1000, "saturated: +-10 variants against blocks of up to 120"), (20000, "narrower: +-200 variants")])
def test_max_size_against_the_windows_reach(hip, window, what):
    al = data_set("plain")
    util.upload(hip, al, variants_of(al))
    check(hip, T.MODE_PHASED, window, 30, 120, 10, what)


def test_more_d_than_one_lds_window_holds(hip):
    """max_size = 900 > 768: the layer kernel loops over two windows."""
    al = util.random_alleles(1000, 64, seed=77, low_ac=4)
    util.upload(hip, al, variants_of(al))
    got, _, _ = check(hip, T.MODE_PHASED, 2000, 100, 900, 4, "two windows")
    assert got["K"] == [2, 3, 4]


def test_equal_sizes_and_the_whole_slice(hip):
    al = data_set("mosaic64")                          # 140 variants
    util.upload(hip, al, variants_of(al))
    M = al.shape[0]
    got, _, _ = check(hip, T.MODE_PHASED, 3000, 7, 7, 25, "7 divides 140")
    assert got["K"] == [20] and list(got["cuts"][0]) == list(range(0, 141, 7))
    got, _, _ = check(hip, T.MODE_PHASED, 3000, 9, 9, 25, "9 does not divide 140")
    assert got["K"] == [] and not got["feasible"].any()
    got, _, _ = check(hip, T.MODE_PHASED, 3000, 1, M, 5, "1 .. n")
    assert got["K"] == [1, 2, 3, 4, 5] and got["cost"][0] == 0 and list(got["cuts"][0]) == [0, M]
    got, _, _ = check(hip, T.MODE_PHASED, 3000, 1, M, M, "every K")
    assert got["K"] == list(range(1, M + 1)) and int(got["cost"][M - 1]) == got["total"]


def test_no_record_leaves_the_tie_rule_alone(hip):
    """A cut-off no pair passes: all weights are 0, every partition is optimal, and the smallest-d rule decides every cut - the last
    blocks as small as the others allow."""
    al = data_set("mosaic64")
    util.upload(hip, al, variants_of(al))
    got, _, nrec = check(hip, T.MODE_PHASED, 3000, 10, 40, 8, "no record", filters=T.Filters(minR2=1.5))
    assert nrec == 0 and got["total"] == 0 and got["K"] == [4, 5, 6, 7, 8] and not got["cost"].any()
    assert list(got["cuts"][0]) == [0, 40, 80, 120, 140] and list(got["cuts"][1]) == [0, 40, 80, 120, 130, 140]


# ---- 3: slices and subsets -------------------------------------------------------------------------------------------------------------
def test_a_slice_and_active_subsets(hip):
    al = data_set("plain")
    variants = variants_of(al)
    util.upload(hip, al, variants)
    M, N, _ = al.shape
    check(hip, T.MODE_PHASED, 5000, 20, 90, 9, "a0 > 0", a0=33, n=M - 50)
    try:
        hip.select_samples(np.arange(0, N, 2))
        assert hip.n_samples == (N + 1) // 2
        half, _, _ = check(hip, T.MODE_PHASED, 5000, 20, 90, 9, "sample subset", a0=33, n=M - 50)
    finally:
        hip.select_samples(None)
    keep = np.nonzero(np.arange(M) % 5 != 2)[0]
    try:
        assert hip.select_variants(list=keep) == len(keep)
        check(hip, T.MODE_PHASED, 5000, 20, 90, 9, "variant subset")
    finally:
        hip.select_variants(None)
    full, _, _ = check(hip, T.MODE_PHASED, 5000, 20, 90, 9, "a0 > 0 again", a0=33, n=M - 50)
    assert half["total"] != full["total"]


@pytest.mark.parametrize("name,mode_key", [("plain", "p"), ("missing", "auto")])
def test_tilings_and_repeats_return_the_same_bytes(hip, name, mode_key):
    al = data_set(name)
    util.upload(hip, al, variants_of(al))
    mode = MODES[mode_key][0]
    a = split(hip, mode, 5000, 20, 90, 12)
    b = split(hip, mode, 5000, 20, 90, 12)
    c = split(hip, mode, 5000, 20, 90, 12, tile_variants=64)
    d = split(hip, mode, 5000, 20, 90, 12, tile_variants=128)
    assert a[1] == b[1] == c[1] == d[1] and len(a[0]["K"]) > 0


# ---- 4: refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_engine_usable(hip):
    al = data_set("mosaic64")
    M = al.shape[0]
    util.upload(hip, al, variants_of(al, two_contigs=True))
    h = M // 2
    ok = dict(mode=T.MODE_PHASED, filters=F0, l_window=3000, min_size=5, max_size=20, k_max=6, a0=0, n=h)
    before = split(hip, T.MODE_PHASED, 3000, 5, 20, 6, a0=0, n=h)
    assert len(before[0]["K"]) > 0
    untouched = blob(preset(6))
    for change in (dict(filters=T.Filters(minR2=0.0, minP=0.5)), dict(l_window=0), dict(n=0), dict(a0=M - 10, n=11), dict(mode=99),
                   dict(n=h + 1), dict(a0=h - 1, n=3), dict(n=M),                      # two contigs
                   dict(min_size=0), dict(min_size=21), dict(max_size=65536), dict(k_max=0), dict(k_max=1025)):
        out = preset(6)
        with pytest.raises(T.HipError) as ei:
            hip.ld_split(out=out, **dict(ok, **change))
        assert ei.value.code == -1, change          # TWK_HIP_E_INVALID
        assert blob(out) == untouched, change
    # the largest sizes the contract takes are taken: max_size = 65535, k_max = 1024
    assert hip.ld_split(out=preset(1024), **dict(ok, max_size=65535, k_max=1024))["K"] == list(range(1, h // 5 + 1))
    # a NULL output, through the library itself
    out = preset(6)
    f = F0._c()
    import ctypes as C
    for null in range(4):
        ptrs = [x.ctypes.data for x in out]
        ptrs[null] = None
        rc = hip._lib.twk_hip_ld_split(hip._ctx, T.MODE_PHASED, C.byref(f), 0, h, 0, 3000, 5, 20, 6, *ptrs, None, None)
        assert rc == -1 and blob(out) == untouched
    assert split(hip, T.MODE_PHASED, 3000, 5, 20, 6, a0=0, n=h)[1] == before[1]


def test_n_times_max_size_is_bounded(hip):
    """(uint64)n * max_size >= 2^32 is refused: the smallest upload that reaches it with max_size = 65535 has 65 538 variants."""
    M = 65538
    al = util.random_alleles(M, 8, seed=3, low_ac=1)
    util.upload(hip, al, variants_of(al))
    out = preset(2)
    with pytest.raises(T.HipError) as ei:
        hip.ld_split(T.MODE_PHASED, F0, 500, 1, 65535, 2, out=out)
    assert ei.value.code == -1 and blob(out) == blob(preset(2))
    # the same slice with a max_size inside the bound is taken: 65 538 * 32 769 < 2^32, and two blocks of 32 769 are the only partition
    got, _ = split(hip, T.MODE_PHASED, 500, 32769, 32769, 2)
    assert got["K"] == [2] and list(got["cuts"][0]) == [0, 32769, M]
