"""LD clumping (twk_hip_ld_clump, `tomahawk clump`): P-ordered greedy clumps, decided and walked on the GPU.

The definition, checked literally (include/twk_hip.h): {u, v} is an edge if `calc` would report a record with the two under the
filters; the variants with a P value are visited in ascending P, ties in file order, up to p1; a visited variant that is in no clump
becomes an index variant and claims every variant with P <= p2 that has an edge to it and is in no clump yet.

"Oracle clump": the records of oracle.all_pairs (the pinned restatement of the reference) with minP = 1 and minR2 = 0, those with
R2 >= thr selected here (and the window applied here where one is set), and the walk done in Python (clump() below).  index_of must
be equal byte for byte, n_clumps, n_members and n_edges equal.

Margin condition: as for pruning (tests/test_gpu_prune.py) every oracle case first asserts that no oracle R2 lies within 1e-6 * thr
of thr.  It is a condition on the input, not a tolerance on the output.

Every oracle case with the standard P values also asserts that it is not vacuous: there are index variants, members claimed forwards
and members claimed BACKWARDS (file index below their index variant's) - the ones a fill of only the upper triangle would miss.
"""
import functools
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import MODES, data_set, margin_holds, mosaic140, oracle_records, standard_p
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
P1, P2 = 1e-4, 1e-2


def clump(ia, ib, M, p, p1, p2, a0=0, n=None):
    """The definition: edges (ia[k], ib[k]), ia < ib -> index_of uint32[M]."""
    n = M - a0 if n is None else n
    nb = [[] for _ in range(M)]
    for u, v in zip(ia.tolist(), ib.tolist()):
        if u >= a0 and v < a0 + n:
            nb[u].append(v)
            nb[v].append(u)
    out = np.full(M, NO, dtype=np.uint32)
    sl = np.arange(a0, a0 + n)
    ok = ~np.isnan(p[sl])
    for v in sl[ok][np.argsort(p[sl][ok], kind="stable")].tolist():
        if p[v] > p1:
            break
        if out[v] != NO:
            continue
        out[v] = v
        for w in nb[v]:
            if out[w] == NO and p[w] <= p2:
                out[w] = v
    return out


def tally(index_of):
    """-> (clumps, members, members claimed backwards) of an index_of array."""
    at = np.arange(len(index_of), dtype=np.int64)
    ix = index_of.astype(np.int64)
    inside = index_of != NO
    return int((inside & (ix == at)).sum()), int((inside & (ix != at)).sum()), int((inside & (at < ix)).sum())


# ---- the data sets (reduce_cases.data_set) and their oracle records: computed once per (data set, mode, window), never changed -----------------------------
@functools.lru_cache(maxsize=None)
def oracle_edges(name, mode_key, window=None):
    al = data_set(name)
    data, mask = O.bitvectors_from_alleles(al)
    variants = O.variants_from_alleles(al)
    ia, ib, recs = oracle_records(data, mask, variants, al.shape[1], mode_key, window=window)
    r2 = recs["R2"].astype(np.float64)
    for a in (ia, ib, r2):
        a.setflags(write=False)
    return ia, ib, r2


def oracle_clump(name, mode_key, thr, p, p1, p2, window=None, a0=0, n=None):
    ia, ib, r2 = oracle_edges(name, mode_key, window)
    assert margin_holds(r2, thr), f"an oracle R2 within 1e-6 relative of the cut-off {thr}: the input does not qualify"
    sel = r2 >= thr
    M = data_set(name).shape[0]
    hi = M if n is None else a0 + n
    n_edges = int(((ia[sel] >= a0) & (ib[sel] < hi)).sum())
    return clump(ia[sel], ib[sel], M, p, p1, p2, a0, n), n_edges


def check_against_oracle(hip, name, mode_key, thr, p=None, p1=P1, p2=P2, window=None, vacuity=True, **kw):
    al = data_set(name)
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    # (the oracle's records were made from the same alleles with the default positions: the upload's variants are those)
    p = standard_p(M) if p is None else p
    want, want_edges = oracle_clump(name, mode_key, thr, p, p1, p2, window, kw.get("a0", 0), kw.get("n"))
    if window is not None:
        kw.update(window=T.OPT_WINDOW, l_window=window)
    index_of, n_clumps, n_members, n_edges, npairs = hip.ld_clump(MODES[mode_key][0], T.Filters(minR2=thr), p, p1, p2, **kw)
    wc, wm, wb = tally(want)
    print(f"{name} M={M} N={N} -{mode_key} thr={thr} {kw}: oracle {want_edges} edges, {wc} clumps, {wm} members ({wb} backwards), "
          f"{int((want == NO).sum())} unclaimed; engine {n_edges} edges, {n_clumps} clumps, {n_members} members, "
          f"{int((index_of != want).sum())} entries differ")
    assert index_of.dtype == np.uint32 and index_of.shape == (M,)
    assert n_edges == want_edges
    assert index_of.tobytes() == want.tobytes(), f"index_of differs at {np.nonzero(index_of != want)[0][:8].tolist()}"
    assert (n_clumps, n_members) == (wc, wm) == tally(index_of)[:2]
    if vacuity:
        assert wc > 0 and wb > 0 and wm - wb > 0, "vacuous: the case needs index variants and members claimed in both directions"
    return index_of, n_clumps, n_members, n_edges, npairs


def test_the_oracle_positions_are_the_uploads(hip):
    """oracle_edges builds its variants without an upload: they must be the ones util.upload hands the engine."""
    al = data_set("mosaic64")
    _, _, variants = util.upload(hip, al)
    mine = O.variants_from_alleles(al)
    assert np.array_equal(np.asarray(variants["pos"]), np.asarray(mine["pos"])) and np.array_equal(np.asarray(variants["rid"]), np.asarray(mine["rid"]))


# ---- 1: real LD, 140 variants: one column block, plain and (N = 128) regrouped sets ---------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("thr", [0.5, 0.8])
@pytest.mark.parametrize("N", [250, 128, 64])
def test_clump_haplotype_blocks(hip, N, thr, mode_key):
    # (whether a case has members in both directions depends on thr and mode: asserted for the table's cases below)
    _, n_clumps, _, n_edges, npairs = check_against_oracle(hip, f"mosaic{N}", mode_key, thr, vacuity=False)
    assert npairs == 140 * 139 // 2 and n_clumps > 0 and n_edges > 0


@pytest.mark.parametrize("N,mode_key,thr", [(250, "p", 0.5), (128, "auto", 0.5), (64, "u", 0.8)])
def test_clump_haplotype_blocks_claim_in_both_directions(hip, N, mode_key, thr):
    check_against_oracle(hip, f"mosaic{N}", mode_key, thr)


# ---- 2: several column blocks, rows and mirrored words that cross 64-bit words, n not a multiple of 64 -----------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("thr", [0.2, 0.5, 0.8])
def test_clump_700_variants(hip, thr, mode_key):
    _, _, _, _, npairs = check_against_oracle(hip, "plain", mode_key, thr)
    assert npairs == 700 * 699 // 2


@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("thr", [0.2, 0.5, 0.8])
def test_clump_small_tiles_share_bitmap_words_in_both_directions(hip, thr, mode_key):
    hip.timing_reset()
    check_against_oracle(hip, "plain", mode_key, thr, tile_variants=128)
    assert hip.timing()["count_launches"] >= 5          # diagonal and rectangular launches


# ---- 3: the regrouped sets of the default mode with missing data: both bits set through ids ---------------------------------------
@pytest.mark.parametrize("thr", [0.2, 0.5, 0.8])
def test_clump_regrouped_sets(hip, thr):
    check_against_oracle(hip, "missing", "auto", thr)


# ---- 4: window --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_clump_window(hip, mode_key):
    index_of, _, _, n_edges, _ = check_against_oracle(hip, "plain", mode_key, 0.2, window=300)
    unwindowed, all_edges = oracle_clump("plain", mode_key, 0.2, standard_p(700), P1, P2)
    assert n_edges < all_edges and index_of.tobytes() != unwindowed.tobytes()          # (the window changes the answer: not vacuous)


# ---- 5: a sub-range -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile_variants", [0, 128])
@pytest.mark.parametrize("mode_key,name", [("p", "plain"), ("u", "plain"), ("auto", "missing")])
def test_clump_sub_range(hip, mode_key, name, tile_variants):
    index_of, n_clumps, _, _, npairs = check_against_oracle(hip, name, mode_key, 0.5, a0=100, n=400, tile_variants=tile_variants)
    assert npairs == 400 * 399 // 2 and n_clumps > 0
    assert (index_of[:100] == NO).all() and (index_of[500:] == NO).all()          # nothing outside the slice is set ...
    inside = index_of[index_of != NO]
    assert ((inside >= 100) & (inside < 500)).all()                               # ... or named


# ---- 6: thresholds and order ----------------------------------------------------------------------------------------------------------
def test_clump_everything_when_both_thresholds_are_1(hip):
    index_of, n_clumps, n_members, _, _ = check_against_oracle(hip, "plain", "p", 0.5, p1=1.0, p2=1.0)
    assert (index_of != NO).all() and n_clumps + n_members == 700


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_clump_in_file_order_is_prune(hip, mode_key):
    """P increasing in file order, p1 = p2 = 1: the index variants are exactly prune's kept set."""
    p = (np.arange(700) + 1) / 701.0
    index_of, n_clumps, _, n_edges, _ = check_against_oracle(hip, "plain", mode_key, 0.5, p=p, p1=1.0, p2=1.0, vacuity=False)
    keep, n_kept, p_edges, _ = hip.ld_prune(MODES[mode_key][0], T.Filters(minR2=0.5))
    assert np.array_equal(index_of == np.arange(700), keep == 1) and n_clumps == n_kept and n_edges == p_edges
    assert 0 < n_kept < 700 and tally(index_of)[2] == 0          # (in this order nobody is claimed backwards)


def tied_p(M):
    return np.array([1e-6, 1e-3, 0.5])[np.random.default_rng(78).integers(0, 3, M)]


def test_clump_ties_resolve_in_file_order(hip):
    p = tied_p(700)
    index_of, n_clumps, _, _, _ = check_against_oracle(hip, "plain", "p", 0.5, p=p)
    assert set(np.unique(p[index_of == np.arange(700)])) == {1e-6}          # only the smallest value passes p1 = 1e-4
    # the other way round is a different answer: the order among ties matters, and the engine takes the file's
    ia, ib, r2 = oracle_edges("plain", "p")
    sel = r2 >= 0.5
    assert clump(ia[sel], ib[sel], 700, p, P1, P2).tobytes() == index_of.tobytes()
    back = np.full(700, NO, dtype=np.uint32)
    back[::-1] = clump(699 - ib[sel], 699 - ia[sel], 700, p[::-1].copy(), P1, P2)
    back[back != NO] = 699 - back[back != NO]
    assert back.tobytes() != index_of.tobytes()


def test_clump_nan_is_no_p_value(hip):
    p = tied_p(700)
    p[np.random.default_rng(78).random(700) < 0.33] = np.nan
    nan = np.isnan(p)
    assert 150 < nan.sum() < 320
    index_of, n_clumps, n_members, _, _ = check_against_oracle(hip, "plain", "p", 0.5, p=p)
    assert (index_of[nan] == NO).all()                                  # no NaN variant is an index variant or a member ...
    assert not nan[index_of[index_of != NO]].any()                      # ... and none is named
    # with p2 = 1 they still are not
    index_of, _, _, _, _ = check_against_oracle(hip, "plain", "p", 0.5, p=p, p1=1.0, p2=1.0, vacuity=False)
    assert (index_of[nan] == NO).all() and (index_of[~nan] != NO).all()


# ---- 7: against the engine's own records and scores ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("which", ["plain", "missing", "hostile"])
def test_clump_equals_walk_over_own_records(hip, which, mode_key):
    al = util.extreme_alleles(70, 64, 901, miss=True) if which == "hostile" else data_set(which)
    M = al.shape[0]
    util.upload(hip, al)
    mode = MODES[mode_key][0]
    p = standard_p(M)
    for thr, (p1, p2) in ((0.2, (P1, P2)), (0.5, (P1, P2)), (0.5, (1.0, 1.0))):
        recs, rp, _ = hip.ld_all(mode, T.Filters(minR2=thr))
        ia, ib = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64)
        assert (ia < ib).all()
        want = clump(ia, ib, M, p, p1, p2)
        index_of, n_clumps, n_members, n_edges, npairs = hip.ld_clump(mode, T.Filters(minR2=thr), p, p1, p2)
        n, _, _ = hip.ld_score(mode, T.Filters(minR2=thr))
        print(f"{which} -{mode_key} thr={thr} p1={p1}: {len(recs)} records, {n_edges} edges, {n_clumps} clumps, {n_members} members")
        assert npairs == rp and n_edges == len(recs) == int(n.sum()) // 2
        assert index_of.tobytes() == want.tobytes() and (n_clumps, n_members) == tally(want)[:2]


# ---- 8: long rows: the count kernel splits tiles along K, several launches -------------------------------------------------------------
def test_clump_long_rows(hip):
    M, N, thr = 1024, 100_003, 0.5
    al = util.mosaic_alleles(M, N, seed=2, n_founders=5, switch=0.05, mut=0.01, miss_rate=0.01, miss_variants=0.3)
    data, mask, variants = util.upload(hip, al)
    p = standard_p(M)
    hip.timing_reset()
    index_of, n_clumps, n_members, n_edges, _ = hip.ld_clump(T.MODE_PHASED, T.Filters(minR2=thr), p, tile_variants=512)
    assert hip.timing()["count_launches"] >= 3
    recs, _, _ = hip.ld_all(T.MODE_PHASED, T.Filters(minR2=thr), tile_variants=512)
    ia, ib = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64)
    want = clump(ia, ib, M, p, P1, P2)
    assert n_edges == len(recs) and index_of.tobytes() == want.tobytes() and (n_clumps, n_members) == tally(want)[:2] and n_clumps > 0
    oa, ob, recs = oracle_records(data, mask, variants, N, "p")
    r2 = recs["R2"].astype(np.float64)
    if margin_holds(r2, thr):
        sel = r2 >= thr
        assert n_edges == int(sel.sum()) and index_of.tobytes() == clump(oa[sel], ob[sel], M, p, P1, P2).tobytes()
        print(f"long rows: margin condition holds; oracle and engine agree on {n_edges} edges, {n_clumps} clumps, {n_members} members")
    else:
        print(f"long rows: an oracle R2 lies within 1e-6 relative of {thr}: compared with the engine's own records only")


# ---- 9: determinism ------------------------------------------------------------------------------------------------------------------
def test_clump_runs_are_byte_identical(hip):
    util.upload(hip, data_set("plain"))
    p = standard_p(700)
    a = hip.ld_clump(T.MODE_UNPHASED, T.Filters(minR2=0.2), p, tile_variants=128)
    b = hip.ld_clump(T.MODE_UNPHASED, T.Filters(minR2=0.2), p, tile_variants=128)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:] and 0 < a[1] < 700
    last = hip.clump_last()
    assert last["bitmap_bytes"] == 700 * 11 * 8 and last["walk_ms"] > 0


# ---- 10: errors ----------------------------------------------------------------------------------------------------------------------
def test_clump_refuses_bad_arguments_and_leaves_the_engine_usable(hip):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    util.upload(hip, al)
    p = standard_p(120)
    before, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    bad_p = p.copy()
    bad_p[7] = 1.5
    nan = float("nan")
    for what, call in (("minP", lambda: hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2, minP=0.5), p)),
                       ("p1 > p2", lambda: hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), p, 1e-2, 1e-4)),
                       ("p2 > 1", lambda: hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), p, 1e-4, 1.5)),
                       ("p1 NaN", lambda: hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), p, nan, 1e-2)),
                       ("p2 NaN", lambda: hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), p, 1e-4, nan)),
                       ("a P of 1.5", lambda: hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), bad_p)),
                       ("beyond the last variant", lambda: hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), p, a0=100, n=21))):
        with pytest.raises(T.HipError) as ei:
            call()
        assert ei.value.code == -1, what          # TWK_HIP_E_INVALID
    # (a P outside [0, 1] outside the slice is nobody's business)
    hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), bad_p, a0=8, n=112)
    after, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    assert len(before) > 1000 and before.tobytes() == after.tobytes()
    index_of, n_clumps, n_members, _, _ = hip.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.2), p, 1.0, 1.0)
    assert (n_clumps, n_members) == tally(index_of)[:2] and n_clumps + n_members == 120


# ---- 11: the command line -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,mode_key,thr,window", [(["-p", "-r", "0.5"], "p", 0.5, None), (["-u", "-r", "0.2", "-w", "3000"], "u", 0.2, 3000)])
def test_clump_cli(hip, tmp_path, flags, mode_key, thr, window):
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
    # the association file: every variant but number 5 (not named: no P), number 9 as NA, one line that names no variant, one
    # with a further column, a comment; written in shuffled order
    p = standard_p(M)
    p[[5, 9]] = np.nan
    lines = [f"{int(rid[v]) + 1}\t{int(pos[v]) + 1}\t{float(p[v])!r}" for v in range(M) if v != 5 and v != 9]
    lines[3] = lines[3].replace("\t", " ") + "  0.25 extra"
    lines += [f"{int(rid[9]) + 1}\t{int(pos[9]) + 1}\tNA", "1\t7\t1e-9", "# a comment"]
    order = np.random.default_rng(5).permutation(len(lines))
    assoc = str(tmp_path / "assoc.txt")
    with open(assoc, "w") as fh:
        fh.write("#contig\tpos\tP\n" + "\n".join(lines[k] for k in order) + "\n")
    want = clump(ia[sel], ib[sel], M, p, P1, P2)
    wc, wm, wb = tally(want)
    assert wc > 0 and wm > 0
    r = subprocess.run([hostlib.CLI_PATH, "clump", "-i", twk, "-a", assoc] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head = [l for l in r.stdout.splitlines() if l.startswith("#")]
    rows = [l.split("\t") for l in r.stdout.splitlines() if l and not l.startswith("#")]
    assert head and head[-1].lstrip("#").split("\t") == ["contig", "pos", "P", "index_contig", "index_pos"]
    assert len(rows) == M
    assert [r_[0] for r_ in rows] == [str(int(x) + 1) for x in rid] and [int(r_[1]) for r_ in rows] == [int(x) + 1 for x in pos]
    for v, row in enumerate(rows):
        assert (row[2] == "NA") if np.isnan(p[v]) else (float(row[2]) == p[v]), (v, row)
        if want[v] == NO:
            assert row[3:] == [".", "."], (v, row)
        else:
            assert row[3:] == [str(int(rid[want[v]]) + 1), str(int(pos[want[v]]) + 1)], (v, row)
    assert f"##clumps={wc},members={wm},total={M},edges={int(sel.sum())}" in head
    assert f"{M} lines, 1 name no selected variant; {M - 2} of {M} variants have a P value" in r.stderr
    assert f"Clumped: {wc} index variants claimed {wm} of {M} variants" in r.stderr
