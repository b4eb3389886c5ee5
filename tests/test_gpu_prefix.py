"""The prefix contraction: the two- and three-product launches of the two-product walk contract each tile over a prefix
[0, stop) of its rows only - the stop chosen per tile by the planner (csrc/hip/ld_plan.h plan_prefix_tile_grid) - and the screen bounds what
was not read by the rows' suffix margins (csrc/hip/ld_two_screen.h, k_screen3_pairs / k_screen2_pairs).  What the wider screen keeps is
recounted over the whole rows (k_recount_unphased, which also proves the prefix counts).  The records must be those of prefix = 0, of the
four-product form (three = 0) and of the file-order walk (two = 0), byte for byte, and those of the oracle.

Inputs: tests.test_gpu_two._iid - unlinked variants, p ~ U(0.05, 0.5), copies planted among the low-frequency variants.  The form applies to
rows of more than 128 K chunks only: N = 140,000 is 137 chunks with a ragged last one (grid step 5 chunks, 28 grid points inside the row),
N = 140,000 + 32 * 18 moves the live half-slots of the last chunk.  M = 420."""
import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.test_gpu_two import _iid

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
MODE = T.MODE_UNPHASED
N0, M0, SEED = 140_000, 420, 21


def _same(a, b):
    return np.sort(a, order=ORDER).tobytes() == np.sort(b, order=ORDER).tobytes()


def _run(hip, opt, f, mode=MODE, **kw):
    """One ld_all under options given as keywords prefix / two / three / ... (None: the default) -> (records, n_pairs, timing, launch log)."""
    keys = [k for k in kw if k in ("prefix", "two", "three", "prefix_stop", "count_min_chunks", "fused")]
    call = {k: v for k, v in kw.items() if k not in keys}
    for k in keys:
        opt.set(k, kw[k])
    hip.timing_reset()
    recs, n_pairs, n_rec = hip.ld_all(mode, f, **call)
    tm = hip.timing()
    log = hip.launch_log()
    for k in keys:
        opt.unset(k)
    assert n_rec == len(recs)
    return recs, n_pairs, tm, log


def _took_the_form(tm):
    assert tm["prefix_launches"] >= 1 and 0 < tm["prefix_chunks"] < tm["prefix_chunks_full"], tm
    assert tm["two_launches"] + tm["three_launches"] == tm["count_launches"], tm


@pytest.mark.parametrize("N", [N0, N0 + 32 * 18])
@pytest.mark.parametrize("minR2", [0.1, 0.5])
def test_default_options_give_the_records_of_every_other_form(hip, opt, N, minR2):
    util.upload(hip, _iid(M0, N, SEED))
    f = T.Filters(minR2=minR2)
    got, n_pairs, tm, _ = _run(hip, opt, f)
    print(f"N={N} r2>={minR2}: prefix launches {tm['prefix_launches']} of {tm['count_launches']}, chunks {tm['prefix_chunks']} of "
          f"{tm['prefix_chunks_full']}, recount candidates {tm['recount_candidates']}, records {len(got)}")
    plain, np0, tm0, _ = _run(hip, opt, f, prefix=0)
    four, np4, tm4, _ = _run(hip, opt, f, three=0)
    file_order, np2, tm2, _ = _run(hip, opt, f, two=0)
    assert n_pairs == np0 == np4 == np2 == M0 * (M0 - 1) // 2
    assert tm0["prefix_launches"] == tm4["prefix_launches"] == tm2["prefix_launches"] == 0
    assert tm0["prefix_chunks"] == 0 and tm0["two_launches"] + tm0["three_launches"] == tm0["count_launches"]
    assert len(got) >= 3 and _same(got, plain) and _same(got, four) and _same(got, file_order)
    _took_the_form(tm)
    assert tm["recount_candidates"] >= len(got)


@pytest.mark.parametrize("min_chunks", [8, 1])
def test_last_tiles_split_along_k_inside_the_stop(hip, opt, min_chunks):
    util.upload(hip, _iid(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    got, _, tm, _ = _run(hip, opt, f, count_min_chunks=min_chunks)
    want, _, _, _ = _run(hip, opt, f, prefix=0)
    _took_the_form(tm)
    assert len(got) >= 3 and _same(got, want)


def _thinned_pair(p_w, keep, seed):
    """The _iid data with one pair planted across tiles: v is the unplanted variant whose allele frequency is nearest p_w / keep, and w - written
    over an unplanted variant of frequency near 0.45 - keeps each of v's alt alleles with probability `keep`.  r2 of (w, v) is about
    keep (1 - pv) / (1 - keep pv); their allele counts differ by a factor 1 / keep, so in allele-count order they lie far more than a tile
    apart.  The samples are then reordered so that every carrier of w comes last -> (alleles, v, w, carriers of w)."""
    al = _iid(M0, N0, SEED).copy()
    rng = np.random.default_rng(seed)
    g = al.sum(axis=2, dtype=np.int16)
    rows = {}
    for x in range(M0):
        rows.setdefault(g[x].tobytes(), []).append(x)
    lone = np.array([x[0] for x in rows.values() if len(x) == 1])              # (variants that are no copy of another)
    freq = al.reshape(M0, -1).mean(axis=1)
    v = int(min(lone, key=lambda x: abs(freq[x] - p_w / keep)))
    w = int(min((x for x in lone if x != v), key=lambda x: abs(freq[x] - 0.45)))
    al[w] = al[v] & (rng.random((N0, 2), dtype=np.float32) < keep)
    carr = al[w].any(axis=1)
    order = np.argsort(carr, kind="stable")
    return np.ascontiguousarray(al[:, order, :]), v, w, int(carr.sum())


@pytest.mark.parametrize("p_w,kind", [(0.10, 5), (0.21, 1)])
def test_ld_that_lies_wholly_in_the_unread_part_of_a_stopped_tile(hip, opt, p_w, kind):
    """The case the form can get wrong, where the device-side screen alone decides.  A thinned copy w of a variant v (r2 ~ 0.65) lies, in
    allele-count order, more than a tile away from v: at r2 >= 0.5 the rows below p ~ 0.19 (the first 128) run with two products and the
    rest with three, so w at p = 0.10 meets v in a two-product tile (kind 5) and w at p = 0.21 in a three-product tile (kind 1), neither on
    the diagonal.  prefix = 2 with prefix_stop = 16 stops EVERY tile of every launch after 80 of 137 chunks (81,920 of 140,000 samples),
    and the samples are ordered so that every carrier of w lies behind that stop: the contracted prefix of the pair holds HH = S = 0 - as
    for an unlinked pair of two rare variants, which the screen drops - and only the suffix margins (k_row_suffix_popcount, the
    [plane row][grid] table, the tile's stop from the per-launch table) keep it.  The launch log shows that every tile stopped at chunk 80;
    no list overflowed (every launch is counted as a prefix launch, none was redone); the pair survives; the records are those of
    prefix = 0.  (At r2 >= 0.5 a pair of independent variants is decided after 0.39 of the row at the latest: at 0.58 the lists stay
    all but empty.)"""
    al, v, w, n_carr = _thinned_pair(p_w, 0.7, 5)
    stop_chunks, nchunks = 16 * 5, 137
    assert n_carr <= N0 - stop_chunks * 1024 and al[w, : stop_chunks * 1024].sum() == 0
    util.upload(hip, al)
    f = T.Filters(minR2=0.5)
    want, _, tm0, _ = _run(hip, opt, f, prefix=0)
    got, _, tm, (stats, _) = _run(hip, opt, f, prefix=2, prefix_stop=16)
    print(f"p_w={p_w}: pair ({w}, {v}), {n_carr} carriers of w; launches {[(int(x['kind']), int(x['prefix_chunks']), int(x['prefix_chunks_full']), int(x['candidates'])) for x in stats]}; "
          f"recount candidates {tm['recount_candidates']}, records {len(got)}")
    assert len(stats) == tm["count_launches"] == tm0["count_launches"] == tm["prefix_launches"], tm      # every launch with stops, none redone
    assert kind in [int(x["kind"]) for x in stats]
    for x in stats:
        assert int(x["prefix_chunks_full"]) > 0 and int(x["prefix_chunks"]) * nchunks == int(x["prefix_chunks_full"]) * stop_chunks, x      # every tile: 80 of 137
    by_pair = {(int(r["idxA"]), int(r["idxB"])): r for r in got}
    rec = by_pair.get((min(v, w), max(v, w)))
    assert rec is not None and 0.5 <= rec["R2"] < 0.8, rec
    assert _same(got, want)


def test_carriers_of_planted_pairs_moved_to_the_end_of_the_sample_order(hip, opt):
    """Default options on a sample order that crowds carriers at its end: the carriers of three planted copies come last (every carrier of
    the rarest pair in the last 11 % of the samples - a variant with p >= 0.05 is carried by at least 9.75 % of them, so no reordering puts
    a planted pair wholly into the last tenth).  The planner reads the real suffix margins and the sample decides; the records stay those of
    prefix = 0.  (A copy lies next to its original in allele-count order, in a tile on the diagonal that the planner leaves whole: what a
    stopped tile does with a linked pair is the test above.)"""
    al = _iid(M0, N0, SEED)
    g = al.sum(axis=2, dtype=np.int8)
    by_rows = {}
    for v in range(M0):
        by_rows.setdefault(g[v].tobytes(), []).append(v)
    same = sorted((tuple(x) for x in by_rows.values() if len(x) == 2), key=lambda vw: int((g[vw[0]] > 0).sum()))
    assert len(same) >= 3
    chosen = same[:3]
    carr = [g[v] > 0 for v, _ in chosen]
    n_last = int(carr[0].sum())
    assert n_last <= 0.11 * N0
    order = np.lexsort((carr[2], carr[1], carr[0]))          # (last key first: the rarest pair's carriers are the last samples of all)
    moved = np.ascontiguousarray(al[:, order, :])
    assert moved[chosen[0][0], : N0 - n_last].sum() == 0 and moved[chosen[0][1], : N0 - n_last].sum() == 0
    util.upload(hip, moved)
    f = T.Filters(minR2=0.1)
    got, _, tm, _ = _run(hip, opt, f)
    want, _, _, _ = _run(hip, opt, f, prefix=0)
    _took_the_form(tm)
    pairs = {(int(r["idxA"]), int(r["idxB"])) for r in got}
    for v, w in chosen:
        assert (v, w) in pairs or (w, v) in pairs, (v, w)
    assert _same(got, want)


def test_stop_at_the_first_grid_point_floods_the_list_and_falls_back(hip, opt):
    """prefix = 2 gives every eligible launch the form, prefix_stop = 1 stops every tile after 5 of 137 chunks: nearly every pair passes the
    screen, the list overflows and the launch is redone over whole rows in the same product form - records none twice, none lost.  A
    flooded launch is not counted as a prefix launch (the log keeps its entry, with its stops).  That the call then grants no further
    prefix is held on the CPU only (`make form-check`: CallForms::gave_up): a call of 420 variants plans fewer launches than the pipeline
    holds in flight, so none is issued after the overflow is seen, and a call with more launches than that needs tens of thousands of
    variants at rows this long."""
    util.upload(hip, _iid(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    want, _, tm0, _ = _run(hip, opt, f, prefix=0)
    got, n_pairs, tm, (stats, _) = _run(hip, opt, f, prefix=2, prefix_stop=1)
    assert n_pairs == M0 * (M0 - 1) // 2
    flooded = [x for x in stats if x["prefix_chunks_full"]]
    assert len(flooded) >= 1 and all(int(x["prefix_chunks"]) * 137 == int(x["prefix_chunks_full"]) * 5 for x in flooded)
    assert tm["prefix_launches"] == 0 and tm["prefix_chunks"] == 0, tm                      # every one of them was thrown away ...
    assert tm["count_launches"] == tm0["count_launches"] + len(flooded), tm                # ... and redone, once
    assert tm["two_launches"] - tm0["two_launches"] + tm["three_launches"] - tm0["three_launches"] == len(flooded)      # ... in its own product form
    assert len(np.unique(got[ORDER])) == len(got) == len(want) and _same(got, want)


def test_cut_offs_on_and_next_to_existing_r2_values(hip, opt):
    util.upload(hip, _iid(M0, N0, SEED))
    base, _, _, _ = _run(hip, opt, T.Filters(minR2=0.05), prefix=0)
    r2 = np.unique(base["R2"]); r2 = r2[(r2 < 1) & (r2 > 0.1)]
    assert len(r2) >= 3
    for x in r2[:: max(1, len(r2) // 3)][:3]:
        for cut in (np.nextafter(x, 0.0), x, np.nextafter(x, 1.0)):
            f = T.Filters(minR2=float(cut))
            got, _, tm, _ = _run(hip, opt, f)
            want, _, _, _ = _run(hip, opt, f, prefix=0)
            assert tm["prefix_launches"] >= 1 and _same(got, want), cut


def test_shards_of_the_sorted_triangle_make_the_whole(hip, opt):
    util.upload(hip, _iid(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    whole, n_pairs, tm, _ = _run(hip, opt, f)
    _took_the_form(tm)
    parts = [_run(hip, opt, f, part=k, n_parts=3) for k in range(3)]
    assert sum(p[1] for p in parts) == n_pairs == M0 * (M0 - 1) // 2
    assert sum(p[2]["prefix_launches"] for p in parts) >= 1
    assert _same(np.concatenate([p[0] for p in parts]), whole)


def test_calls_that_never_take_the_form(hip, opt):
    al = _iid(M0, N0, SEED)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)
    def prefix_launches(mode=MODE, filters=f, **kw):
        hip.timing_reset()
        hip.ld_all(mode, filters, **kw)
        return hip.timing()["prefix_launches"]
    assert prefix_launches() >= 1                                         # (the form is there to be refused)
    assert prefix_launches(mode=T.MODE_PHASED) == 0
    assert prefix_launches(filters=T.Filters(minR2=0.0)) == 0
    assert prefix_launches(window=T.OPT_WINDOW, l_window=30_000) == 0
    assert prefix_launches(tile_variants=256) == 0
    opt.set("three", 0)
    assert prefix_launches() == 0
    opt.unset("three")
    opt.set("prefix", 0)
    assert prefix_launches() == 0
    opt.unset("prefix")
    miss = al[:200].copy()
    miss[::7, ::50, :] = 2                                                # missing genotypes: masked planes
    util.upload(hip, miss)
    assert prefix_launches() == 0
    util.upload(hip, np.ascontiguousarray(al[:, :40_000, :]))             # rows of 40 chunks through the matrix: the walk, but never a stop
    opt.set("fused", 0)
    hip.timing_reset()
    hip.ld_all(MODE, f)
    tm = hip.timing()
    assert tm["prefix_launches"] == 0 and tm["two_launches"] + tm["three_launches"] == tm["count_launches"] >= 1


def test_launch_log_and_accounting(hip, opt):
    """Kinds are still 5 (two products) then 1 (three); a prefix launch's row_pairs are full-row equivalents - plane-row pairs x chunks
    contracted / chunks per row, rounded down once per launch - and sum to the timing's, as do the chunks."""
    util.upload(hip, _iid(M0, N0, SEED))
    _, _, tm, (stats, seen) = _run(hip, opt, T.Filters(minR2=0.5))
    _took_the_form(tm)
    kinds = [int(x["kind"]) for x in stats]
    assert seen == len(stats) == tm["count_launches"]
    assert set(kinds) <= {5, 1} and kinds == sorted(kinds, reverse=True), kinds
    assert kinds.count(5) == tm["two_launches"] and kinds.count(1) == tm["three_launches"]
    assert sum(int(x["row_pairs"]) for x in stats) == tm["row_pairs"]
    assert sum(int(x["row_pairs"]) for x in stats if x["kind"] == 1) == tm["three_row_pairs"]
    assert sum(int(x["prefix_chunks"]) for x in stats) == tm["prefix_chunks"]
    assert sum(int(x["prefix_chunks_full"]) for x in stats) == tm["prefix_chunks_full"]
    assert sum(1 for x in stats if x["prefix_chunks_full"]) == tm["prefix_launches"]          # (no list flooded: every launch with stops counts)
    for x in stats:
        if x["prefix_chunks_full"]:
            tiles = int(x["prefix_chunks_full"]) // 137
            assert int(x["prefix_chunks_full"]) == tiles * 137 and int(x["row_pairs"]) == 128 * 128 * int(x["prefix_chunks"]) // 137


def test_prefix_against_the_oracle(hip, opt):
    M = 150
    al = _iid(M, N0, 23)
    data, mask, variants = util.upload(hip, al)
    want = O.all_pairs(data, None, variants, N0, O.settings(minR2=0.8, unphased=True), vector_only=False)
    got, _, tm, _ = _run(hip, opt, T.Filters(minR2=0.8))
    assert len(want) >= 2 and tm["prefix_launches"] >= 1 and tm["prefix_chunks"] < tm["prefix_chunks_full"] and tm["recount_candidates"] >= len(want)
    util.assert_records_match(got, want, variants, double_root=util.double_root_vetter(data, None, variants, N0))
