"""One product a pair in front of a row block's one_end: a carrier launch of the two-product walk whose pairs all pass the screen's
lower test at S >= 0 - a function of the two dosages - contracts the carrier rows H | Q of both variants, CC = CH + CQ, and its screen tests the
carrier form's upper value alone (csrc/hip/ld_two_screen.h: screen1c_keeps, k_screen1_pairs).  What passes is recounted with four products from
the whole rows (k_recount_unphased, which also proves CC), so the records must be those of one = 0, of the file-order walk (two = 0) and of the
four-product form (three = 0), byte for byte, and those of the oracle.

Inputs as in test_gpu_carrier.py: unlinked variants, p ~ U(0.05, 0.5), copies planted among the variants with p < 0.22.  N = 140,000 is 137 chunks
with a ragged last one.  M = 700 with one_rows = 128: the first row block (p up to ~ 0.13) has its one_end at 512 at r2 >= 0.1 - the diagonal
tile and three off-diagonal one-product tiles of 128 x 128 variants - and two-product tiles behind it."""
import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
MODE = T.MODE_UNPHASED
N0, M0, SEED, NCHUNKS = 140_000, 700, 31, 137
KEYS = ("one", "one_rows", "carrier", "prefix", "two", "three", "prefix_stop", "count_min_chunks", "fused", "cand_cap")
_DATA = {}


def _iid22(M, N, seed):
    """(M, N, 2) alleles: iid, p ~ U(0.05, 0.5); of the variants with p < 0.22 every fourth is followed (in file order, some places on) by a
    copy of itself - exact, with a per-mille of its alleles flipped, or with its two haplotypes swapped.  Built once per shape."""
    key = (M, N, seed)
    if key not in _DATA:
        _DATA.clear()
        rng = np.random.default_rng(seed)
        p = rng.uniform(0.05, 0.5, size=M)
        al = np.empty((M, N, 2), dtype=np.int8)
        for v in range(M):
            al[v] = (rng.random((N, 2), dtype=np.float32) < p[v])
        low = np.flatnonzero(p < 0.22)[::4]
        for k, v in enumerate(low):
            w = (v + 3 + 7 * k) % M
            if w in low or w == v:
                continue
            if k % 3 == 0:
                al[w] = al[v]
            elif k % 3 == 1:
                al[w] = al[v] ^ (rng.random((N, 2), dtype=np.float32) < 0.001)
            else:
                al[w] = al[v][:, ::-1]
        _DATA[key] = al
    return _DATA[key]


def _same(a, b):
    return np.sort(a, order=ORDER).tobytes() == np.sort(b, order=ORDER).tobytes()


def _run(hip, opt, f, mode=MODE, **kw):
    """One ld_all under options given as keywords (KEYS; absent: the default, but one_rows = 128) -> (records, n_pairs, timing, launch log)."""
    kw.setdefault("one_rows", 128)
    keys = [k for k in kw if k in KEYS]
    call = {k: v for k, v in kw.items() if k not in keys}
    for k in keys:
        opt.set(k, kw[k])
    hip.timing_reset()
    recs, n_pairs, n_rec = hip.ld_all(mode, f, **call)
    tm = hip.timing()
    stats, _ = hip.launch_log()
    for k in keys:
        opt.unset(k)
    assert n_rec == len(recs)
    return recs, n_pairs, tm, stats


def _sorted_margins(al):
    g = al.sum(axis=2, dtype=np.int16)
    het, hom = (g == 1).sum(axis=1).astype(np.uint32), (g == 2).sum(axis=1).astype(np.uint32)
    order = np.argsort(het + 2 * hom, kind="stable")
    return het[order], hom[order]


def test_the_plan_of_the_default_shape_has_both_kinds():
    """The planner on this shape's real margins (host arithmetic): the first block of 128 rows has a one-product launch of the columns [0, 512) - the
    diagonal tile and three more - and two-product launches behind it, and no one-product launch reaches a pair whose lower test fails."""
    al = _iid22(M0, N0, SEED)
    het, hom = _sorted_margins(al)
    meta = np.zeros(M0, dtype=T.META_DTYPE)
    meta["pos"] = np.arange(M0, dtype=np.uint32) * 100 + 1000
    meta["ac"] = 5
    pl = T.plan_region(meta, N0, 0, M0, 0, M0, True, planes_per_variant=2, k_chunks=NCHUNKS, minR2=0.1, phased_math=False, het=het, hom=hom,
                       carrier=True, one=True, one_rows=128)
    tiles = pl["tiles"]
    assert pl["two_end"] >= 128 and pl["n_pairs"] == M0 * (M0 - 1) // 2
    first = [t for t in tiles if int(t["rowA0"]) == 0]
    ones = [t for t in first if t["one"]]
    assert len(ones) == 1 and int(ones[0]["nA"]) == 128 and int(ones[0]["rowB0"]) == 0 and int(ones[0]["nB"]) == 512 and int(ones[0]["diag"]) == 1, first
    twos = [t for t in first if not t["one"]]
    assert twos and min(int(t["rowB0"]) for t in twos) == 512 and max(int(t["rowB0"]) + int(t["nB"]) for t in twos) == M0
    assert not any(t["one"] for t in tiles if int(t["rowA0"]) >= pl["two_end"])
    # without the form: no launch is marked, and the pairs are the same
    pl0 = T.plan_region(meta, N0, 0, M0, 0, M0, True, planes_per_variant=2, k_chunks=NCHUNKS, minR2=0.1, phased_math=False, het=het, hom=hom, carrier=True)
    assert not pl0["tiles"]["one"].any() and pl0["n_pairs"] == pl["n_pairs"] and pl0["two_end"] == pl["two_end"]
    # every pair of the launch passes the lower test: -(dA dB) - eps inside the bound (the doubles of screen1c_lower_ok)
    d = (het.astype(np.float64) + 2.0 * hom)
    two_n, cut = 2.0 * N0, 0.1 * (1.0 - 1e-6)
    da, db = d[127], d[511]
    assert (-(da * db) - 1e-5 * two_n * two_n) ** 2 < cut * da * (two_n - da) * db * (two_n - db)


@pytest.mark.parametrize("prefix,stop", [(1, 0), (0, 0), (2, 24)])
@pytest.mark.parametrize("N", [N0, N0 + 32 * 18])
@pytest.mark.parametrize("minR2", [0.1, 0.05])
def test_records_are_those_of_every_other_form(hip, opt, N, minR2, prefix, stop):
    """r2 >= 0.1, and r2 >= 0.05 - where the cut and every one_end lie earlier, and the noisy copies survive all the same.  N + 32 * 18 moves the
    live half-slots of the last chunk.  prefix 2 with prefix_stop 24: every tile stops at chunk 120 of 137."""
    util.upload(hip, _iid22(M0, N, SEED))
    f = T.Filters(minR2=minR2)
    kw = dict(prefix=prefix, prefix_stop=stop) if stop else dict(prefix=prefix)
    got, n_pairs, tm, stats = _run(hip, opt, f, **kw)
    carrier, np0, tm0, stats0 = _run(hip, opt, f, one=0, **kw)
    file_order, np2, tm2, _ = _run(hip, opt, f, two=0, **kw)
    four, np4, tm4, _ = _run(hip, opt, f, three=0, **kw)
    print(f"N={N} r2>={minR2} prefix={prefix} stop={stop}: one-product launches {tm['one_launches']} of {tm['carrier_launches']} carrier of {tm['count_launches']}; "
          f"recount candidates {tm['recount_candidates']} (one = 0: {tm0['recount_candidates']}); records {len(got)}; "
          f"launches {[(int(x['kind']), int(x['carrier']), int(x['one']), int(x['row_pairs']), int(x['candidates'])) for x in stats]}")
    assert n_pairs == np0 == np2 == np4 == M0 * (M0 - 1) // 2
    assert tm0["one_launches"] == tm2["one_launches"] == tm4["one_launches"] == 0 and not any(x["one"] for x in stats0)
    assert len(got) >= 10 and _same(got, carrier) and _same(got, file_order) and _same(got, four)
    if minR2 == 0.1:
        assert tm["one_launches"] >= 1 and tm["carrier_launches"] > tm["one_launches"], tm          # both kinds ran
        assert all((not x["one"]) or (x["carrier"] and int(x["kind"]) == 5) for x in stats)
        assert sum(1 for x in stats if x["one"]) == tm["one_launches"]
        assert tm["two_launches"] + tm["three_launches"] == tm["count_launches"], tm               # none redone
        assert tm["recount_candidates"] >= len(got)
        # accounting: a one-product launch's row_pairs are variant pairs in tiles of 128 x 128 - here the 4 tiles of the columns [0, 512)
        one = [x for x in stats if x["one"]][0]
        full = int(one["prefix_chunks_full"]) // NCHUNKS if one["prefix_chunks_full"] else int(one["row_pairs"]) // (128 * 128)
        assert full == 4, one
        if prefix:
            assert tm["prefix_launches"] >= 1 and 0 < tm["prefix_chunks"] < tm["prefix_chunks_full"], tm


def test_last_tiles_split_along_k_and_added_into_zeroed_tiles(hip, opt):
    util.upload(hip, _iid22(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    want, _, _, _ = _run(hip, opt, f, one=0)
    for prefix in (1, 0):
        got, _, tm, _ = _run(hip, opt, f, count_min_chunks=1, prefix=prefix)
        assert tm["one_launches"] >= 1 and len(got) >= 10 and _same(got, want), prefix


@pytest.mark.parametrize("M", [641, 700])
def test_partial_tiles_on_both_axes(hip, opt, M):
    """two = 2 gives every row block of the walk the form where the planner marks it; M = 641 and 700 leave partial tiles on both axes of the last
    blocks (641 = 5 x 128 + 1; 700 = 5 x 128 + 60), whose rows end in the zeroed pad behind the carrier rows.  At r2 >= 0.5 the one-product columns
    reach far, and no list floods."""
    util.upload(hip, _iid22(M, N0, SEED))
    f = T.Filters(minR2=0.5)
    got, n_pairs, tm, stats = _run(hip, opt, f, two=2, one=2)
    want, _, tm0, _ = _run(hip, opt, f, one=0)
    four, _, _, _ = _run(hip, opt, f, three=0)
    print(f"M={M}: launches {[(int(x['kind']), int(x['carrier']), int(x['one']), int(x['row_pairs']), int(x['candidates'])) for x in stats]}")
    assert n_pairs == M * (M - 1) // 2
    assert tm["one_launches"] >= 2 and tm0["one_launches"] == 0, tm
    assert len(got) >= 3 and _same(got, want) and _same(got, four)


def _thinned_pair(p_w, keep, seed):
    """The _iid22 data with one pair planted across tiles (see test_gpu_carrier.py): w keeps each of v's alt alleles with probability `keep`, and
    the samples are reordered so that every carrier of w comes last -> (alleles, v, w, carriers of w)."""
    al = _iid22(M0, N0, SEED).copy()
    rng = np.random.default_rng(seed)
    g = al.sum(axis=2, dtype=np.int16)
    rows = {}
    for x in range(M0):
        rows.setdefault(g[x].tobytes(), []).append(x)
    lone = np.array([x[0] for x in rows.values() if len(x) == 1])
    freq = al.reshape(M0, -1).mean(axis=1)
    v = int(min(lone, key=lambda x: abs(freq[x] - p_w / keep)))
    w = int(min((x for x in lone if x != v), key=lambda x: abs(freq[x] - 0.45)))
    al[w] = al[v] & (rng.random((N0, 2), dtype=np.float32) < keep)
    carr = al[w].any(axis=1)
    order = np.argsort(carr, kind="stable")
    return np.ascontiguousarray(al[:, order, :]), v, w, int(carr.sum())


def test_thinned_copy_whose_carriers_lie_behind_a_fixed_stop(hip, opt):
    """A thinned copy w (p ~ 0.07, r2 ~ 0.65 with its original v, p ~ 0.10) more than a tile from v in allele-count order, both inside the first
    block's one-product columns, the samples ordered so that every carrier of w lies behind chunk 80 of 137.  prefix = 2 with prefix_stop = 16
    stops every tile there: the prefix of the pair holds CC = 0 and only the suffix margins keep it (screen1c_prefix_keeps).  The recount compares
    HH + QH + HQ + QQ over [0, stop) with what the launch counted - a mismatch fails the call - and the records are the four-product form's."""
    al, v, w, n_carr = _thinned_pair(0.07, 0.7, 5)
    stop_chunks = 16 * 5
    assert n_carr <= al.shape[1] - stop_chunks * 1024 and al[w, : stop_chunks * 1024].sum() == 0
    util.upload(hip, al)
    f = T.Filters(minR2=0.5)
    want, _, _, _ = _run(hip, opt, f, prefix=0, three=0)
    got, _, tm, stats = _run(hip, opt, f, prefix=2, prefix_stop=16)
    print(f"pair ({w}, {v}); launches {[(int(x['kind']), int(x['one']), int(x['prefix_chunks']), int(x['prefix_chunks_full']), int(x['candidates'])) for x in stats]}")
    assert tm["one_launches"] >= 1 and tm["prefix_launches"] == tm["count_launches"] == len(stats), tm      # every launch with stops, none redone
    for x in stats:
        assert int(x["prefix_chunks"]) * NCHUNKS == int(x["prefix_chunks_full"]) * stop_chunks > 0, x
    rec = {(int(r["idxA"]), int(r["idxB"])): r for r in got}.get((min(v, w), max(v, w)))
    assert rec is not None and 0.5 <= rec["R2"] < 0.8, rec
    assert _same(got, want)


def test_a_one_product_prefix_launch_that_floods_is_redone_over_whole_rows(hip, opt):
    """A fixed stop at the first coarse point (5 chunks of 137) leaves the screen almost nothing but the suffix margins: every pair is a candidate,
    the lists of the launches overflow.  one = 2, prefix = 2: the one-product launch is redone over whole rows - still with one product, which
    then holds - and the records are those of one = 0.  With the stops gone for the call, the launches behind it run over whole rows."""
    util.upload(hip, _iid22(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    want, _, tm0, _ = _run(hip, opt, f, one=0)
    got, n_pairs, tm, stats = _run(hip, opt, f, one=2, prefix=2, prefix_stop=1)
    print(f"launches {[(int(x['kind']), int(x['carrier']), int(x['one']), int(x['prefix_chunks']), int(x['candidates'])) for x in stats]}")
    assert n_pairs == M0 * (M0 - 1) // 2
    assert tm["one_launches"] >= 2 and tm["count_launches"] > tm0["count_launches"], tm      # (what flooded ran again)
    assert len(np.unique(got[ORDER])) == len(got) == len(want) and _same(got, want)


def test_the_ladder_below_a_one_product_launch(hip, opt):
    """cand_cap = 8: the candidate list of every screened launch holds eight pairs, fewer than the planted copies of the first block.  The one-product
    launch overflows and is redone in the carrier two-product form - the next entry of the launch log, over the same rows - which overflows in its
    turn, and so on down to four products; no record is lost or doubled, and the call has given up `one` (and, here, what lies below it)."""
    util.upload(hip, _iid22(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    want, _, tm0, _ = _run(hip, opt, f, one=0)
    got, n_pairs, tm, stats = _run(hip, opt, f, one=2, prefix=0, cand_cap=8)
    forms = [(int(x["kind"]), int(x["carrier"]), int(x["one"]), int(x["candidates"])) for x in stats]
    print(f"launches {forms}")
    assert n_pairs == M0 * (M0 - 1) // 2
    k = [i for i, x in enumerate(forms) if x[2]]
    assert k and k[0] == 0 and all(forms[i][3] > 8 for i in k), forms         # the first launch took one product, and it overflowed (as did any in flight behind it)
    assert forms[k[0] + 1][:3] == (5, 1, 0) and forms[k[0] + 1][3] > 8, forms  # redone with two products on carrier rows, which overflowed as well
    assert forms[k[0] + 2][0] == 1 and forms[k[0] + 3][0] == 0, forms          # ... three products, four products
    assert len(np.unique(got[ORDER])) == len(got) == len(want) and _same(got, want)


def test_shards_of_the_sorted_triangle_make_the_whole(hip, opt):
    util.upload(hip, _iid22(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    whole, n_pairs, tm, _ = _run(hip, opt, f)
    assert tm["one_launches"] >= 1
    parts = [_run(hip, opt, f, part=k, n_parts=3) for k in range(3)]
    assert sum(p[1] for p in parts) == n_pairs == M0 * (M0 - 1) // 2
    assert sum(p[2]["one_launches"] for p in parts) >= 1
    assert _same(np.concatenate([p[0] for p in parts]), whole)


def test_one_product_against_the_oracle(hip, opt):
    M = 150
    al = _iid22(M, N0, 33)
    data, mask, variants = util.upload(hip, al)
    want = O.all_pairs(data, None, variants, N0, O.settings(minR2=0.8, unphased=True), vector_only=False)
    got, _, tm, _ = _run(hip, opt, T.Filters(minR2=0.8), two=2, one=2)
    assert len(want) >= 2 and tm["one_launches"] >= 1 and tm["recount_candidates"] >= len(want)
    util.assert_records_match(got, want, variants, double_root=util.double_root_vetter(data, None, variants, N0))


def test_calls_that_never_take_the_form(hip, opt):
    al = _iid22(M0, N0, SEED)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)
    opt.set("one_rows", 128)

    def one_launches(mode=MODE, filters=f, **kw):
        hip.timing_reset()
        hip.ld_all(mode, filters, **kw)
        return hip.timing()["one_launches"]
    assert one_launches() >= 1                                        # (the form is there to be refused)
    assert one_launches(mode=T.MODE_PHASED) == 0
    assert one_launches(filters=T.Filters(minR2=0.0)) == 0            # cut-off 0: no screen
    assert one_launches(window=T.OPT_WINDOW, l_window=30_000) == 0
    assert one_launches(tile_variants=256) == 0                       # an explicit tile edge keeps the file order
    for key in ("one", "carrier", "two", "three"):
        opt.set(key, 0)
        assert one_launches() == 0, key
        opt.unset(key)
    opt.unset("one_rows")
