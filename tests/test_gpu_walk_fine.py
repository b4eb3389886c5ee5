"""The fine walk (option "walk_fine"): the carrier screens hold QQ to min(qA, qB, CQ), a row block's borders between the
one-, two- and three-product forms are staircases - asked per tile row of 128 variants - with a two-product launch from the diagonal to the rows'
two_reach in the blocks behind the cut, and a tile's stop is the planner's answer without the spare grid step.  Every candidate is still recounted
from whole rows, so the records must be those of walk_fine = 0 and of the four-product form (three = 0), byte for byte.

Shapes: 140,000 samples (137 chunks, ragged last chunk) and 262,144 + 40 samples (257 chunks, where the option's default begins), iid variants with
p ~ U(0.05, 0.5) and 20 planted pairs: thinned copies (w keeps each alt allele of v with probability `keep`: p_w = keep p_v, r2 = keep (1 - p_v) /
(1 - keep p_v)), whose two variants lie far apart in allele-count order - on either side of either staircase - and copies with a few alleles
flipped, which lie next to their original: in the diagonal tiles.  walk_fine = 2 is the hook that takes the walk at 137 chunks; one_rows = 128 makes
a front block one tile row (its border is then the block's own), one_rows = 384 gives the front blocks three steps; the blocks behind the cut are cut
where a tile row's last row no longer passes against the column next to it."""
import numpy as np
import pytest

import tomahawk_amd as T
from tests import util

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
MODE = T.MODE_UNPHASED
SHAPES = {137: (140_000, 1200), 257: (262_144 + 40, 900)}       # chunks -> (samples, variants)
KEYS = ("walk_fine", "one", "one_rows", "carrier", "prefix", "two", "three", "cand_cap", "prefix_sigma")
# (p of the original, keep) of the thinned copies; (p, flip probability) of the noisy ones
THINNED = [(0.30, 0.50), (0.20, 0.60), (0.35, 0.40), (0.33, 0.55), (0.45, 0.45), (0.48, 0.40), (0.42, 0.50), (0.40, 0.50),
           (0.26, 0.74), (0.29, 0.66), (0.30, 0.85), (0.29, 0.80), (0.50, 0.50), (0.27, 0.70), (0.46, 0.55), (0.28, 0.68)]
NOISY = [(0.10, 0.05), (0.25, 0.10), (0.40, 0.03), (0.23, 0.15)]
_DATA = {}


def _data(chunks):
    """-> (alleles (M, N, 2), the planted pairs as file indices (v, w)).  Built once per shape."""
    if chunks not in _DATA:
        _DATA.clear()
        N, M = SHAPES[chunks]
        rng = np.random.default_rng(1000 + chunks)
        p = rng.uniform(0.05, 0.5, size=M)
        al = np.empty((M, N, 2), dtype=np.int8)
        for v in range(M):
            al[v] = rng.random((N, 2), dtype=np.float32) < p[v]
        used, pairs = set(), []

        def pick(target):
            v = min((x for x in range(M) if x not in used), key=lambda x: abs(p[x] - target))
            used.add(v)
            return v
        for p_v, keep in THINNED:
            v, w = pick(p_v), pick(p_v * keep)
            al[w] = al[v] & (rng.random((N, 2), dtype=np.float32) < keep)
            pairs.append((v, w))
        for p_v, eps in NOISY:
            v, w = pick(p_v), pick(p_v)
            al[w] = al[v] ^ (rng.random((N, 2), dtype=np.float32) < eps)
            pairs.append((v, w))
        _DATA[chunks] = (al, pairs, _sorted_margins(al))
    return _DATA[chunks][:2]


def _sorted_margins(al):
    g = al.sum(axis=2, dtype=np.int16)
    het, hom = (g == 1).sum(axis=1).astype(np.uint32), (g == 2).sum(axis=1).astype(np.uint32)
    order = np.argsort(het + 2 * hom, kind="stable")
    return het[order], hom[order], order


def _plan(chunks, minR2, one_rows, fine):
    _data(chunks)
    N, M = SHAPES[chunks]
    het, hom, order = _DATA[chunks][2]
    meta = np.zeros(M, dtype=T.META_DTYPE)
    meta["pos"] = np.arange(M, dtype=np.uint32) * 100 + 1000
    meta["ac"] = 5
    pl = T.plan_region(meta, N, 0, M, 0, M, True, planes_per_variant=2, k_chunks=chunks, minR2=minR2, phased_math=False, het=het, hom=hom,
                       carrier=True, one=True, one_rows=one_rows, walk_fine=fine)
    return pl, order


def _same(a, b):
    return np.sort(a, order=ORDER).tobytes() == np.sort(b, order=ORDER).tobytes()


def _run(hip, opt, f, **kw):
    keys = [k for k in kw if k in KEYS]
    for k in keys:
        opt.set(k, kw[k])
    hip.timing_reset()
    recs, n_pairs, n_rec = hip.ld_all(MODE, f)
    tm = hip.timing()
    stats, _ = hip.launch_log()
    for k in keys:
        opt.unset(k)
    assert n_rec == len(recs)
    return recs, n_pairs, tm, stats


def _zones(pl, order, pairs):
    """Where the planted pairs lie in the plan: per pair (sorted row, sorted column, zone) with zone one of front-left, front-right, behind-left,
    behind-right, past (rows from two_last on) and, for a pair within 128 of the diagonal, diag."""
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    out = []
    for v, w in pairs:
        a, b = sorted((int(rank[v]), int(rank[w])))
        s = int(pl["stair"][a])
        if b - a < 128:
            zone = "diag"
        elif a < pl["two_end"]:
            zone = "front-left" if (s and b < s) else "front-right" if s else "front"
        elif a < pl["two_last"]:
            zone = "behind-left" if b < s else "behind-right"
        else:
            zone = "past"
        out.append((a, b, zone))
    return out


@pytest.mark.parametrize("chunks", [137, 257])
def test_the_plans_of_the_shapes_have_both_staircases(chunks):
    """The planner alone, on the shapes' real margins: two_end < two_last < n; with one_rows = 384 some tile row's one_end differs from its block's;
    a two-product launch behind the cut at either height of block; the planted pairs lie on both sides of each staircase and in diagonal tiles;
    and without the fine walk the plan has neither."""
    N, M = SHAPES[chunks]
    pl, order = _plan(chunks, 0.1, 384, True)
    assert 0 < pl["two_end"] < pl["two_last"] < M, (pl["two_end"], pl["two_last"])
    stepped = [t for t in pl["tiles"] if t["one"] and len(np.unique(pl["stair"][int(t["rowA0"]): int(t["rowA0"]) + int(t["nA"])])) > 1]
    assert stepped and all(int(t["rowA0"]) + int(t["nA"]) <= pl["two_end"] for t in stepped), "no front block has a step"
    assert pl["behind"].sum() >= 1 and (pl["side"] == 1).sum() >= 2 and (pl["side"] == 2).sum() >= 2
    for r in range(1, M):                                        # never rising inside a block, constant over a tile row
        if pl["stair"][r] and pl["stair"][r - 1] and pl["stair"][r] > pl["stair"][r - 1]:
            assert any(int(t["rowA0"]) == r for t in pl["tiles"]), r
    zones = [z for _, _, z in _zones(pl, order, _data(chunks)[1])]
    print(f"{chunks} chunks: two_end {pl['two_end']} two_last {pl['two_last']} launches {len(pl['tiles'])} zones {zones}")
    for z in ("front-left", "front-right", "behind-left", "behind-right", "diag"):
        assert zones.count(z) >= 1, (z, zones)
    assert _plan(chunks, 0.1, 128, True)[0]["behind"].sum() >= 1
    pl0, _ = _plan(chunks, 0.1, 384, False)
    assert not pl0["side"].any() and not pl0["behind"].any() and not pl0["stair"].any() and pl0["two_last"] == pl0["two_end"]
    assert pl0["n_pairs"] == pl["n_pairs"] == M * (M - 1) // 2


def _contracted(stats, chunks):
    """Tile chunks the launches of a call contracted: a launch with stops says so itself, a launch over whole rows contracted all of its tiles' chunks."""
    return sum(int(x["prefix_chunks"]) if x["prefix_chunks_full"] else int(x["row_pairs"]) // (128 * 128) * chunks for x in stats)


@pytest.mark.parametrize("one_rows", [128, 384])
@pytest.mark.parametrize("minR2", [0.1, 0.05])
@pytest.mark.parametrize("chunks", [137, 257])
def test_records_are_those_of_the_parent_plan_and_of_four_products(hip, opt, chunks, minR2, one_rows):
    """Records and n_pairs equal those of walk_fine = 0 and of three = 0, every planted pair is found, no launch is redone, the call runs the plan's
    two-product launches behind the cut, and fewer tile chunks are contracted than at walk_fine = 0.  The timing's prefix_chunks counts the launches
    that took stops only: it is compared as it stands where every launch took them in both calls, and with the whole-row launches' chunks added
    otherwise (140,000 samples at r2 >= 0.05: walk_fine = 0 runs 1,730 of 1,918 chunks with stops in one launch of three and the rest over whole
    rows, walk_fine = 2 runs 8,734 of 9,590 with stops in four launches of five - more chunks with stops, fewer in all)."""
    al, pairs = _data(chunks)
    N, M = SHAPES[chunks]
    util.upload(hip, al)
    f = T.Filters(minR2=minR2)
    pl, order = _plan(chunks, minR2, one_rows, True)
    got, n_pairs, tm, stats = _run(hip, opt, f, walk_fine=2, one_rows=one_rows)
    coarse, np0, tm0, stats0 = _run(hip, opt, f, walk_fine=0, one_rows=one_rows)
    four, np4, _, _ = _run(hip, opt, f, walk_fine=2, one_rows=one_rows, three=0)
    forms = [(int(x["kind"]), int(x["carrier"]), int(x["one"]), int(x["row_pairs"]), int(x["candidates"])) for x in stats]
    print(f"{chunks} chunks r2>={minR2} one_rows={one_rows}: two_end {pl['two_end']} two_last {pl['two_last']}; launches {tm['count_launches']} (walk_fine 0: {tm0['count_launches']}), "
          f"two-product {tm['two_launches']} ({tm0['two_launches']}), prefix chunks {tm['prefix_chunks']} of {tm['prefix_chunks_full']} ({tm0['prefix_chunks']} of {tm0['prefix_chunks_full']}), "
          f"recount candidates {tm['recount_candidates']} ({tm0['recount_candidates']}), records {len(got)}; {forms}")
    assert n_pairs == np0 == np4 == M * (M - 1) // 2
    assert _same(got, coarse) and _same(got, four)
    # every planted pair is found
    have = {(int(r["idxA"]), int(r["idxB"])) for r in got}
    missing = [(v, w) for v, w in pairs if (min(v, w), max(v, w)) not in have]
    assert not missing, missing
    # no launch is redone: the launches are the plan's, each in a screened form
    assert tm["count_launches"] == len(pl["tiles"]) == len(stats), (tm["count_launches"], len(pl["tiles"]))
    # (... and the only launches in no screened form are those whose sample was dense in candidates, as many as at walk_fine = 0: the commonest rows at r2 >= 0.05)
    assert tm["count_launches"] - tm["two_launches"] - tm["three_launches"] == tm0["count_launches"] - tm0["two_launches"] - tm0["three_launches"] <= 1, (tm, tm0)
    if minR2 == 0.1:
        assert tm["two_launches"] + tm["three_launches"] == tm["count_launches"], tm
    assert 0 < _contracted(stats, chunks) < _contracted(stats0, chunks), (_contracted(stats, chunks), _contracted(stats0, chunks))
    if tm["prefix_launches"] == tm["count_launches"] and tm0["prefix_launches"] == tm0["count_launches"]:
        assert 0 < tm["prefix_chunks"] < tm0["prefix_chunks"], (tm["prefix_chunks"], tm0["prefix_chunks"])
    # at least one two-product launch behind two_end: the plan has them, and the call ran that many two-product launches more than lie in front of the cut
    n_front = sum(1 for t in pl["tiles"] if int(t["rowA0"]) + int(t["nA"]) <= pl["two_end"])
    assert pl["behind"].sum() >= 1 and tm["two_launches"] == n_front + int(pl["behind"].sum()), (tm["two_launches"], n_front, int(pl["behind"].sum()))


@pytest.mark.parametrize("chunks", [137, 257])
def test_the_default_begins_at_256_chunks(hip, opt, chunks):
    """walk_fine = 1, the default: today's plan at 137 chunks, the fine walk at 257."""
    al, _ = _data(chunks)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)
    dflt, _, tm1, _ = _run(hip, opt, f, one_rows=384)
    off, _, tm0, _ = _run(hip, opt, f, one_rows=384, walk_fine=0)
    on, _, tm2, _ = _run(hip, opt, f, one_rows=384, walk_fine=2)
    assert _same(dflt, off) and _same(dflt, on)
    same_as = tm2 if chunks >= 256 else tm0
    for k in ("count_launches", "two_launches", "three_launches", "one_launches", "prefix_chunks", "prefix_chunks_full", "row_pairs"):
        assert tm1[k] == same_as[k], (k, tm1[k], same_as[k])
    assert tm2["two_launches"] > tm0["two_launches"]


@pytest.mark.parametrize("chunks", [137, 257])
def test_the_ladder_below_the_fine_walk(hip, opt, chunks):
    """cand_cap = 8: the candidate list of every screened launch holds eight pairs.  The 20 planted pairs alone leave every launch of this plan
    eight candidates or fewer, so 60 thinned copies more are planted over the whole range of p, and 12 copies with 2 % of their alleles flipped among the
    rows of the block behind the cut, next to their originals (a copy of the shape's data, the plan's margins barely moved).  Every launch with more than eight candidates is redone down the ladder - a two-product launch behind the cut with three products, then
    four - and the records are the four-product step's."""
    al, _ = _data(chunks)
    N, M = SHAPES[chunks]
    al = al.copy()
    rng = np.random.default_rng(77 + chunks)
    for v, w in rng.permutation(M)[:120].reshape(60, 2):
        al[w] = al[v] & (rng.random((N, 2), dtype=np.float32) < rng.uniform(0.5, 0.9))
    pl, order = _plan(chunks, 0.1, 384, True)
    n_front = sum(1 for t in pl["tiles"] if int(t["rowA0"]) + int(t["nA"]) <= pl["two_end"])
    for k in range(12):
        v, w = order[pl["two_end"] + 4 + 6 * k], order[pl["two_end"] + 5 + 6 * k]
        al[w] = al[v] ^ (rng.random((N, 2), dtype=np.float32) < 0.02)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)
    want, _, _, _ = _run(hip, opt, f, three=0)
    plain, _, tm1, stats1 = _run(hip, opt, f, walk_fine=2, one_rows=384)
    got, n_pairs, tm, stats = _run(hip, opt, f, walk_fine=2, one_rows=384, cand_cap=8)
    forms = [(int(x["kind"]), int(x["carrier"]), int(x["one"]), int(x["candidates"])) for x in stats]
    print(f"{chunks} chunks: launches without the cap {[(int(x['kind']), int(x['candidates'])) for x in stats1]}; with it {forms}")
    assert n_pairs == M * (M - 1) // 2 and len(want) >= 60
    rich = sum(1 for x in stats1 if int(x["candidates"]) > 8)
    assert tm1["two_launches"] + tm1["three_launches"] == tm1["count_launches"] and rich >= 3, stats1      # screened launches, some with more candidates than the cap
    assert any(int(x["kind"]) == 5 and int(x["candidates"]) > 8 for x in stats1[n_front:]), stats1      # ... the two-product launch behind the cut among them
    assert tm["count_launches"] >= tm1["count_launches"] + rich, (tm["count_launches"], tm1["count_launches"], rich)      # every one of them ran again
    assert any(x[0] == 0 for x in forms), forms                                                               # ... down to four products
    assert _same(plain, want) and len(np.unique(got[ORDER])) == len(got) == len(want) and _same(got, want)
