"""Haplotype blocks (twk_hip_ld_dprime_ci_band, twk_hip_ld_blocks): the D' confidence bounds in band storage and the blocks selected
from them on the device, against the NumPy restatement of tests/blocks_cases.py.

THE BOUNDS are compared slot for slot, with no tolerance.  The device's log and exp differ from NumPy's in the last bits, so the
comparison rests on a CONDITION ON THE INPUT instead: the restatement reports the smallest relative distance of any running sum of any
pair from its threshold, and the test asserts that it is above 1e-9 - far beyond what the last bits of 101 terms can move.  No pair is
exempt.  In -p the tables are integers and bit-exact in the oracle too, so the bounds are checked once more against the oracle's
records.  In -u the oracle's estimated haplotype counts differ from the engine's at the record path's bar, which moves the likelihood
by more than that margin: -u and the default mode are checked against the engine's own records only.

THE BLOCKS are a function of the lo / hi bytes, the positions and the parameters alone, and are compared exactly with the restatement
over the bytes the device returned.
"""
import functools

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import blocks_cases as BC
from tests import util
from tests.reduce_cases import MODES, blob, data_set, oracle_records
from tests.test_gpu_bandmat import assert_layout

pytestmark = pytest.mark.gpu

F0 = T.Filters(minR2=0.0)
WINDOW = 20000
CASES = [("mosaic250", "p"), ("mosaic64", "p"), ("plain", "p"), ("mosaic128", "auto"), ("mosaic128", "u"), ("missing", "auto"), ("missing", "u")]
TIGHT = dict(max_span_2=150, max_span_3=400)


def variants_of(al, two_contigs=False):
    M = al.shape[0]
    pos = BC.positions(M)
    rid = np.zeros(M, dtype=np.uint32)
    if two_contigs:
        h = M // 2 + 3
        rid[h:] = 1
        pos[h:] -= pos[h] - 500
    return O.variants_from_alleles(al, pos=pos.astype(np.uint32), rid=rid)


def engine_records(hip, mode, a0, n):
    recs, _, nrec = hip.ld_region(mode, F0, a0, n, a0, n, True, window=T.OPT_WINDOW, l_window=WINDOW)
    assert nrec == len(recs)
    return recs


def assert_bounds(hip, mode, variants, a0=0, n=None, what=""):
    """ld_dprime_ci_band of the slice against the restatement over the engine's own records; -> (lo, hi, first, indptr, n_pairs)."""
    n = len(variants) - a0 if n is None else n
    recs = engine_records(hip, mode, a0, n)
    lo, hi, first, indptr, nrec, npairs = hip.ld_dprime_ci_band(mode, F0, WINDOW, a0=a0, n=n)
    assert_layout(first, indptr, variants, WINDOW, a0, n)
    assert lo.dtype == np.uint8 and hi.dtype == np.uint8 and lo.shape == hi.shape == (int(indptr[-1]),)
    want_lo, want_hi, gap = BC.band_of_records(recs, first, indptr, a0)
    bad = np.nonzero((lo != want_lo) | (hi != want_hi))[0]
    print(f"{what}: n {n}, {len(lo)} slots, {nrec} records, smallest gap {gap:.3g}, {len(bad)} slots differ")
    assert gap > BC.GAP, f"{what}: a running sum within {gap:.3g} of its threshold: the input does not decide the bounds"
    assert len(bad) == 0, f"{what}: first {[(int(k), int(lo[k]), int(hi[k]), int(want_lo[k]), int(want_hi[k])) for k in bad[:4]]}"
    assert nrec == len(recs) > 0 and ((lo == BC.NONE) == (hi == BC.NONE)).all()
    assert (lo[lo != BC.NONE] <= hi[lo != BC.NONE]).all() and hi[hi != BC.NONE].max() <= 100
    for t in (64,):
        again = hip.ld_dprime_ci_band(mode, F0, WINDOW, a0=a0, n=n, tile_variants=t)
        assert blob(again[:5]) == blob((lo, hi, first, indptr, nrec)), f"{what}: tile_variants={t} returns other bytes"
    return lo, hi, first, indptr, npairs


def assert_blocks(hip, mode, variants, lo, hi, first, indptr, npairs, a0=0, n=None, what="", tile_variants=0, **kw):
    """ld_blocks of the slice against the restatement over the bytes the device returned; -> the restatement's dict."""
    M = len(variants)
    n = M - a0 if n is None else n
    got = hip.ld_blocks(mode, F0, WINDOW, params=T.BlockParams(**kw) if kw else None, a0=a0, n=n, tile_variants=tile_variants)
    block_of, b_first, b_last, b_s, b_r, n_cand, n_inf, n_pairs = got
    want = BC.blocks_of(lo, hi, first, indptr, variants["pos"][a0:a0 + n], **kw)
    want_of = np.full(M, T.NO_BLOCK, dtype=np.uint32)
    inside = want["block_of"] >= 0
    want_of[a0:a0 + n][inside] = (want["block_of"][inside] + a0).astype(np.uint32)
    sizes = want["last"] - want["first"] + 1
    print(f"{what} {kw}: {n_inf} informative, {n_cand} candidates, {len(b_first)} blocks (want {len(sizes)}), sizes {np.bincount(sizes) if len(sizes) else []}")
    assert block_of.dtype == np.uint32 and block_of.tobytes() == want_of.tobytes()
    assert np.array_equal(b_first, want["first"] + a0) and np.array_equal(b_last, want["last"] + a0)
    assert np.array_equal(b_s, want["n_strong"]) and np.array_equal(b_r, want["n_recomb"])
    assert (n_cand, n_inf, n_pairs) == (want["n_candidates"], want["n_informative"], npairs)
    rid = variants["rid"]
    assert (rid[b_first] == rid[b_last]).all(), "a block spans two contigs"
    return want, got


# ---- 1: the bounds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode_key", CASES)
def test_bounds_and_blocks_against_the_restatement(hip, name, mode_key):
    al = data_set(name)
    variants = variants_of(al)
    util.upload(hip, al, variants)
    mode = MODES[mode_key][0]
    band = assert_bounds(hip, mode, variants, what=f"{name} -{mode_key}")
    loose, got = assert_blocks(hip, mode, variants, *band, what=f"{name} -{mode_key}")
    tight, got_tight = assert_blocks(hip, mode, variants, *band, what=f"{name} -{mode_key}", tile_variants=64, **TIGHT)
    last = hip.blocks_last()
    assert last["band_bytes"] == 2 * len(band[0])
    if mode_key == "p":      # (what the restatement gives on the oracle's tables: the spans bind, and every size class occurs)
        sizes = loose["last"] - loose["first"] + 1
        assert blob(got[:5]) != blob(got_tight[:5]) and len(tight["first"]) < len(loose["first"])
        assert all((sizes == k).any() for k in (2, 3, 4)) and (sizes >= 5).any()
        assert last["walk_ms"] > 0


@functools.lru_cache(maxsize=None)
def oracle_band(name):
    al = data_set(name)
    variants = variants_of(al)
    data, mask = O.bitvectors_from_alleles(al)
    ia, ib, recs = oracle_records(data, mask, variants, al.shape[1], "p", 0.0, WINDOW)
    r = np.zeros(len(recs), dtype=[("idxA", "<i8"), ("idxB", "<i8"), ("cnt", "<f8", (4,))])
    r["idxA"], r["idxB"], r["cnt"] = ia, ib, recs["cnt"]
    return r


@pytest.mark.parametrize("name", ["mosaic250", "mosaic64", "plain"])
def test_phased_bounds_against_the_oracles_tables(hip, name):
    al = data_set(name)
    variants = variants_of(al)
    util.upload(hip, al, variants)
    lo, hi, first, indptr, nrec, _ = hip.ld_dprime_ci_band(T.MODE_PHASED, F0, WINDOW)
    want_lo, want_hi, gap = BC.band_of_records(oracle_band(name), first, indptr)
    print(f"{name}: {nrec} records, smallest gap {gap:.3g}, {int(((lo != want_lo) | (hi != want_hi)).sum())} slots differ")
    assert gap > BC.GAP and nrec == len(oracle_band(name))
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)


@pytest.mark.parametrize("name,mode_key", [("mosaic250", "p"), ("missing", "auto")])
def test_a_slice_and_two_contigs(hip, name, mode_key):
    al = data_set(name)
    mode = MODES[mode_key][0]
    variants = variants_of(al, two_contigs=True)
    util.upload(hip, al, variants)
    M = len(variants)
    band = assert_bounds(hip, mode, variants, what=f"{name} -{mode_key} two contigs")
    want, got = assert_blocks(hip, mode, variants, *band, what=f"{name} -{mode_key} two contigs")
    assert len(want["first"]) > 0 and len(set(variants["rid"][got[1]])) == 2
    a0, n = 29, M - 40
    band = assert_bounds(hip, mode, variants, a0=a0, n=n, what=f"{name} -{mode_key} slice")
    want, got = assert_blocks(hip, mode, variants, *band, a0=a0, n=n, what=f"{name} -{mode_key} slice", tile_variants=64)
    assert (got[0][:a0] == T.NO_BLOCK).all() and (got[0][a0 + n:] == T.NO_BLOCK).all() and len(want["first"]) > 0


# ---- 2: the blocks ----------------------------------------------------------------------------------------------------------------------
def test_iid_data_has_no_block(hip):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    variants = variants_of(al)
    util.upload(hip, al, variants)
    band = assert_bounds(hip, T.MODE_PHASED, variants, what="iid")
    want, got = assert_blocks(hip, T.MODE_PHASED, variants, *band, what="iid")
    assert len(got[1]) == 0 and (got[0] == T.NO_BLOCK).all() and got[6] > 1000


def test_blocks_of_a_variant_selection_equal_those_of_the_kept_rows(hip):
    al = data_set("plain")
    variants = variants_of(al)
    keep = np.nonzero(np.arange(len(variants)) % 5 != 2)[0]
    util.upload(hip, al, variants)
    try:
        assert hip.select_variants(list=keep) == len(keep)
        selected = hip.ld_blocks(T.MODE_PHASED, F0, WINDOW)
    finally:
        hip.select_variants(None)
    util.upload(hip, np.ascontiguousarray(al[keep]), variants[keep])
    uploaded = hip.ld_blocks(T.MODE_PHASED, F0, WINDOW)
    assert len(uploaded[1]) > 10 and blob(selected) == blob(uploaded)


@pytest.mark.parametrize("name,mode_key", [("plain", "p"), ("missing", "auto")])
def test_runs_and_tilings_return_the_same_bytes(hip, name, mode_key):
    al = data_set(name)
    util.upload(hip, al, variants_of(al))
    mode = MODES[mode_key][0]
    a = hip.ld_blocks(mode, F0, WINDOW)
    b = hip.ld_blocks(mode, F0, WINDOW)
    c = hip.ld_blocks(mode, F0, WINDOW, tile_variants=64)
    assert blob(a) == blob(b) == blob(c) and len(a[1]) > 0


def test_refusals_leave_the_engine_usable(hip):
    al = data_set("mosaic64")
    util.upload(hip, al, variants_of(al))
    M = al.shape[0]
    before = hip.ld_blocks(T.MODE_PHASED, F0, WINDOW)
    P = T.BlockParams
    for kw in (dict(params=P(strong_lo=101)), dict(params=P(strong_hi=101)), dict(params=P(recomb_hi=101)), dict(params=P(strong_lo_2=101)),
               dict(params=P(strong_lo_34=101)), dict(params=P(recomb_hi=99, strong_hi=98)), dict(params=P(inform_permille=1001)),
               dict(filters=T.Filters(minR2=0.0, minP=0.5)), dict(l_window=0), dict(a0=M - 10, n=11), dict(n=0)):
        kw.setdefault("filters", F0)
        kw.setdefault("l_window", WINDOW)
        with pytest.raises(T.HipError) as ei:
            hip.ld_blocks(T.MODE_PHASED, **kw)
        assert ei.value.code == -1, kw          # TWK_HIP_E_INVALID
    for kw in (dict(filters=T.Filters(minR2=0.0, minP=0.5)), dict(l_window=0), dict(a0=M - 10, n=11)):
        kw.setdefault("filters", F0)
        kw.setdefault("l_window", WINDOW)
        with pytest.raises(T.HipError) as ei:
            hip.ld_dprime_ci_band(T.MODE_PHASED, **kw)
        assert ei.value.code == -1, kw
    assert blob(hip.ld_blocks(T.MODE_PHASED, F0, WINDOW)) == blob(before) and len(before[1]) > 0
