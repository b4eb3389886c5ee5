"""LD pruning (twk_hip_ld_prune, `tomahawk prune`): greedy pruning in file order, decided and walked on the GPU.

The definition, checked literally: over a triangle of variants a pair (u, v), u < v, is an edge if `calc` would report a record for
it under the filters; walking v upwards, v is kept if and only if no kept u < v has an edge (u, v).

"Oracle prune": the records of oracle.all_pairs (the pinned restatement of the reference) with minP = 1 and minR2 = 0, those with
R2 >= thr selected here (and the window applied here where one is set), and the walk done in Python.  keep must be equal byte for
byte, n_kept and n_edges equal.

Margin condition: one borderline pair can flip a whole cascade of decisions, so every oracle case first asserts, on the oracle's
unthresholded records, that no R2 lies within 1e-6 * thr of thr - the record path's own bar on R2.  It is a condition on the input,
not a tolerance on the output.
"""
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import MODES, big_missing, big_plain, margin_holds, mosaic140, oracle_records
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

def greedy_walk(ia, ib, M, a0=0, n=None):
    """The definition: edges (ia[k], ib[k]), ia < ib, inside [a0, a0 + n) -> keep uint8[M]."""
    n = M - a0 if n is None else n
    inside = (ia >= a0) & (ib < a0 + n)
    partners = [[] for _ in range(M)]          # partners[v]: the u < v with an edge (u, v)
    for u, v in zip(ia[inside].tolist(), ib[inside].tolist()):
        partners[v].append(u)
    keep = np.zeros(M, dtype=np.uint8)
    for v in range(a0, a0 + n):
        keep[v] = 0 if any(keep[u] for u in partners[v]) else 1
    return keep, int(inside.sum())


def oracle_prune(data, mask, variants, N, mode_key, thr, window=None, a0=0, n=None):
    ia, ib, recs = oracle_records(data, mask, variants, N, mode_key, window=window)
    r2 = recs["R2"].astype(np.float64)
    assert margin_holds(r2, thr), f"an oracle R2 within 1e-6 relative of the cut-off {thr}: the input does not qualify"
    sel = r2 >= thr
    return greedy_walk(ia[sel], ib[sel], len(variants), a0, n)


def check_against_oracle(hip, al, mode_key, thr, window=None, what="", **kw):
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    a0, n = kw.get("a0", 0), kw.get("n")
    want, want_edges = oracle_prune(data, mask, variants, N, mode_key, thr, window, a0, n)
    if window is not None:
        kw.update(window=T.OPT_WINDOW, l_window=window)
    keep, n_kept, n_edges, npairs = hip.ld_prune(MODES[mode_key][0], T.Filters(minR2=thr), **kw)
    print(f"{what or f'M={M} N={N} -{mode_key}'} thr={thr}: oracle {want_edges} edges, {int(want.sum())} kept; engine {n_edges} edges, {n_kept} kept, "
          f"{int((keep != want).sum())} flags differ")
    assert keep.dtype == np.uint8 and keep.shape == (M,)
    assert n_edges == want_edges
    assert keep.tobytes() == want.tobytes(), f"keep differs at {np.nonzero(keep != want)[0][:8].tolist()}"
    assert n_kept == int(want.sum()) == int(keep.sum())
    return keep, n_kept, n_edges, npairs


# ---- 1: real LD, 140 variants: one column block, plain and (N = 128) regrouped sets ---------------------------------------------------
CASES_140 = [(N, thr) for N in (250, 128, 1000) for thr in (0.2, 0.5, 0.8)] + [(64, thr) for thr in (0.1, 0.3, 0.5, 0.8)]
#   (N = 64 without 0.2: one pair there has r2 = 0.2 exactly)


@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("N,thr", CASES_140)
def test_prune_haplotype_blocks(hip, N, thr, mode_key):
    keep, n_kept, n_edges, npairs = check_against_oracle(hip, mosaic140(N), mode_key, thr)
    assert npairs == 140 * 139 // 2 and 0 < n_kept < 140 and n_edges > 0 and keep[0] == 1


# ---- 2: several column blocks, rows that cross 64-bit words, n not a multiple of 64 ------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("thr", [0.2, 0.5, 0.8])
def test_prune_700_variants(hip, thr, mode_key):
    keep, n_kept, n_edges, npairs = check_against_oracle(hip, big_plain(), mode_key, thr)
    assert npairs == 700 * 699 // 2 and 0 < n_kept < 700


@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("thr", [0.2, 0.5, 0.8])
def test_prune_small_tiles_share_bitmap_words(hip, thr, mode_key):
    hip.timing_reset()
    check_against_oracle(hip, big_plain(), mode_key, thr, tile_variants=128)
    assert hip.timing()["count_launches"] >= 5          # diagonal and rectangular launches


# ---- 3: the regrouped sets of the default mode with missing data: bits set through ids -----------------------------------------------
@pytest.mark.parametrize("thr", [0.2, 0.5, 0.8])
def test_prune_regrouped_sets(hip, thr):
    keep, n_kept, n_edges, _ = check_against_oracle(hip, big_missing(), "auto", thr)
    assert 0 < n_kept < 600


# ---- 4: window --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_prune_window(hip, mode_key):
    al = big_plain()
    M, N, _ = al.shape
    keep, _, n_edges, _ = check_against_oracle(hip, al, mode_key, 0.2, window=300)
    data, mask, variants = util.upload(hip, al)
    unwindowed, all_edges = oracle_prune(data, mask, variants, N, mode_key, 0.2)
    assert n_edges < all_edges and keep.tobytes() != unwindowed.tobytes()          # (the window changes the answer: not vacuous)


# ---- 5: a sub-range -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key,al", [("p", "plain"), ("u", "plain"), ("auto", "missing")])
def test_prune_sub_range(hip, mode_key, al):
    al = big_plain() if al == "plain" else big_missing()
    keep, n_kept, _, npairs = check_against_oracle(hip, al, mode_key, 0.5, a0=100, n=400)
    assert npairs == 400 * 399 // 2 and not keep[:100].any() and not keep[500:].any() and keep[100] == 1


# ---- 6: against the engine's own records and scores ------------------------------------------------------------------------------------
def walk_of_own_records(hip, mode, thr, M, **kw):
    recs, npairs, _ = hip.ld_all(mode, T.Filters(minR2=thr), **kw)
    ia, ib = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64)
    assert (ia < ib).all()
    keep, _ = greedy_walk(ia, ib, M)
    return keep, len(recs), npairs


@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("data_set", ["plain", "missing", "hostile"])
def test_prune_equals_walk_over_own_records(hip, data_set, mode_key):
    al = {"plain": big_plain, "missing": big_missing, "hostile": lambda: util.extreme_alleles(70, 64, 901, miss=True)}[data_set]()
    M = al.shape[0]
    util.upload(hip, al)
    mode = MODES[mode_key][0]
    for thr in (0.2, 0.5):
        want, n_recs, rp = walk_of_own_records(hip, mode, thr, M)
        keep, n_kept, n_edges, npairs = hip.ld_prune(mode, T.Filters(minR2=thr))
        n, _, _ = hip.ld_score(mode, T.Filters(minR2=thr))
        print(f"{data_set} -{mode_key} thr={thr}: {n_recs} records, {n_edges} edges, {n_kept} kept")
        assert npairs == rp and n_edges == n_recs == int(n.sum()) // 2
        assert keep.tobytes() == want.tobytes() and n_kept == int(want.sum())


# ---- 7: long rows: the count kernel splits tiles along K, several launches -------------------------------------------------------------
def test_prune_long_rows(hip):
    M, N, thr = 1024, 100_003, 0.5
    al = util.mosaic_alleles(M, N, seed=2, n_founders=5, switch=0.05, mut=0.01, miss_rate=0.01, miss_variants=0.3)
    data, mask, variants = util.upload(hip, al)
    hip.timing_reset()
    keep, n_kept, n_edges, _ = hip.ld_prune(T.MODE_PHASED, T.Filters(minR2=thr), tile_variants=512)
    assert hip.timing()["count_launches"] >= 3
    want, n_recs, _ = walk_of_own_records(hip, T.MODE_PHASED, thr, M, tile_variants=512)
    assert n_edges == n_recs and keep.tobytes() == want.tobytes() and 0 < n_kept == int(want.sum()) < M
    ia, ib, recs = oracle_records(data, mask, variants, N, "p")
    r2 = recs["R2"].astype(np.float64)
    if margin_holds(r2, thr):
        sel = r2 >= thr
        o_keep, o_edges = greedy_walk(ia[sel], ib[sel], M)
        assert n_edges == o_edges and keep.tobytes() == o_keep.tobytes()
        print(f"long rows: margin condition holds; oracle and engine agree on {o_edges} edges, {n_kept} kept")
    else:
        print(f"long rows: an oracle R2 lies within 1e-6 relative of {thr}: compared with the engine's own records only")


# ---- 8: determinism ------------------------------------------------------------------------------------------------------------------
def test_prune_runs_are_byte_identical(hip):
    util.upload(hip, big_plain())
    a = hip.ld_prune(T.MODE_UNPHASED, T.Filters(minR2=0.2), tile_variants=128)
    b = hip.ld_prune(T.MODE_UNPHASED, T.Filters(minR2=0.2), tile_variants=128)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:] and 0 < a[1] < 700


# ---- 9: errors -----------------------------------------------------------------------------------------------------------------------
def test_prune_refuses_a_fisher_cutoff_and_leaves_the_engine_usable(hip):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    util.upload(hip, al)
    before, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    with pytest.raises(T.HipError) as ei:
        hip.ld_prune(T.MODE_AUTO, T.Filters(minR2=0.2, minP=0.5))
    assert ei.value.code == -1          # TWK_HIP_E_INVALID
    with pytest.raises(T.HipError) as ei:
        hip.ld_prune(T.MODE_AUTO, T.Filters(minR2=0.2), a0=100, n=21)          # beyond the last variant
    assert ei.value.code == -1
    after, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    assert len(before) > 1000 and before.tobytes() == after.tobytes()
    keep, n_kept, _, _ = hip.ld_prune(T.MODE_AUTO, T.Filters(minR2=0.2))
    assert 0 < n_kept == int(keep.sum()) <= 120


# ---- 10: the command line -----------------------------------------------------------------------------------------------------------
def _prune_cli(twk, flags):
    r = subprocess.run([hostlib.CLI_PATH, "prune", "-i", twk] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head = [l for l in r.stdout.splitlines() if l.startswith("#")]
    rows = [l.split("\t") for l in r.stdout.splitlines() if l and not l.startswith("#")]
    assert head and head[-1].lstrip("#").split("\t") == ["contig", "pos", "keep"]
    return head, rows, r.stderr


@pytest.mark.parametrize("flags,mode_key,thr,window", [(["-p", "-r", "0.5"], "p", 0.5, None), (["-u", "-r", "0.2", "-w", "3000"], "u", 0.2, 3000)])
def test_prune_cli(hip, tmp_path, flags, mode_key, thr, window):
    al = mosaic140(250)
    M, N, _ = al.shape
    rid = np.repeat([0, 1], [80, 60]).astype(np.uint32)
    pos = np.concatenate([np.arange(80) * 100 + 1000, np.arange(60) * 100 + 500]).astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    data, mask = O.bitvectors_from_alleles(al)
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    ia, ib, recs = oracle_records(data, mask, variants, N, mode_key, window=window)
    r2 = recs["R2"].astype(np.float64)
    assert margin_holds(r2, thr)
    sel = r2 >= thr
    if window is not None:
        assert (rid[ia[sel]] == rid[ib[sel]]).all()          # no edge crosses contigs when a window is set
    want, want_edges = greedy_walk(ia[sel], ib[sel], M)
    head, rows, log = _prune_cli(twk, flags)
    assert len(rows) == M
    assert [r[0] for r in rows] == [str(int(x) + 1) for x in rid] and [int(r[1]) for r in rows] == [int(p) + 1 for p in pos]
    assert all(r[2] in ("0", "1") for r in rows)
    keep = np.array([int(r[2]) for r in rows], dtype=np.uint8)
    assert keep.tobytes() == want.tobytes()
    assert f"##kept={int(want.sum())},total={M},edges={want_edges}" in head
    assert "Pruned: kept" in log
