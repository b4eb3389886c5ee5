"""The carrier plane as the row operand of the two-product walk: on rows of more than 128 K chunks a two-product launch contracts
the row variant's H | Q against the column variant's H and Q rows - CH = HH + QH and CQ = HQ + QQ in place of HH and HQ - and its screen bounds
S >= CQ and S + HH <= CH + CQ + min(qA, qB) (csrc/hip/ld_two_screen.h: screen2c_keeps, k_screen2_pairs with ScreenWork::carrier).  The bound is
tighter than the H form's, so the walk's cut lies further on (r2 >= 0.1: p ~ 0.21 for ~ 0.16).  What passes is recounted with four products from
the whole rows (k_recount_unphased, which also proves CH and CQ), so the records must be those of carrier = 0, of the file-order walk (two = 0)
and of the four-product form (three = 0), byte for byte, and those of the oracle.

Inputs: unlinked variants, p ~ U(0.05, 0.5), with copies (exact, per-mille noisy, haplotypes swapped) planted among the variants with p < 0.22,
so that the rows the cut newly reaches hold survivors.  N = 140,000 is 137 chunks with a ragged last one, N = 140,000 + 32 * 18 moves the live
half-slots of the last chunk.  M = 420: at r2 >= 0.1 the H form's cut (p ~ 0.16, about 100 sorted rows) rounds down to no A tile at all and
the carrier form's (p ~ 0.21, about 150 rows) to one."""
import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
MODE = T.MODE_UNPHASED
N0, M0, SEED, NCHUNKS = 140_000, 420, 31, 137
KEYS = ("carrier", "prefix", "two", "three", "prefix_stop", "count_min_chunks", "fused")
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
    """One ld_all under options given as keywords (KEYS; absent: the default) -> (records, n_pairs, timing, launch log entries)."""
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


def _tiles5(stats, carrier=None):
    """Tiles of 128 row variants x 64 column variants the two-product launches of a call listed (a prefix launch's row_pairs are scaled by its
    stops: its tiles are its full-row chunks over the chunks of a row)."""
    n = 0
    for x in stats:
        if int(x["kind"]) == 5 and (carrier is None or bool(x["carrier"]) == carrier):
            n += int(x["prefix_chunks_full"]) // NCHUNKS if x["prefix_chunks_full"] else int(x["row_pairs"]) // (128 * 128)
    return n


@pytest.mark.parametrize("prefix", [1, 0])
@pytest.mark.parametrize("N", [N0, N0 + 32 * 18])
@pytest.mark.parametrize("minR2", [0.1, 0.5])
def test_records_are_those_of_every_other_form(hip, opt, N, minR2, prefix):
    util.upload(hip, _iid22(M0, N, SEED))
    f = T.Filters(minR2=minR2)
    got, n_pairs, tm, stats = _run(hip, opt, f, prefix=prefix)
    h_form, np0, tm0, stats0 = _run(hip, opt, f, prefix=prefix, carrier=0)
    file_order, np2, tm2, _ = _run(hip, opt, f, prefix=prefix, two=0)
    four, np4, tm4, _ = _run(hip, opt, f, prefix=prefix, three=0)
    print(f"N={N} r2>={minR2} prefix={prefix}: carrier launches {tm['carrier_launches']} of {tm['two_launches']} two-product of {tm['count_launches']}; "
          f"two-product tiles {_tiles5(stats)} (H plane: {_tiles5(stats0)}); recount candidates {tm['recount_candidates']} (H plane: {tm0['recount_candidates']}); records {len(got)}")
    assert n_pairs == np0 == np2 == np4 == M0 * (M0 - 1) // 2
    assert tm["carrier_launches"] >= 1 and tm["carrier_launches"] == tm["two_launches"], tm
    assert tm0["carrier_launches"] == tm2["carrier_launches"] == tm4["carrier_launches"] == 0
    assert all(bool(x["carrier"]) == (int(x["kind"]) == 5) for x in stats) and not any(x["carrier"] for x in stats0)
    assert tm["two_launches"] + tm["three_launches"] == tm["count_launches"], tm
    assert len(got) >= 10 and _same(got, h_form) and _same(got, file_order) and _same(got, four)
    assert tm["recount_candidates"] >= len(got)
    assert _tiles5(stats) >= _tiles5(stats0)
    if minR2 == 0.1:
        assert _tiles5(stats) > _tiles5(stats0)          # the two-product rows reach beyond the H form's cut
    if prefix:
        assert tm["prefix_launches"] >= 1 and 0 < tm["prefix_chunks"] < tm["prefix_chunks_full"], tm


def test_last_tiles_split_along_k_and_added_into_zeroed_tiles(hip, opt):
    util.upload(hip, _iid22(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    want, _, _, _ = _run(hip, opt, f, carrier=0)
    for prefix in (1, 0):
        got, _, tm, _ = _run(hip, opt, f, count_min_chunks=1, prefix=prefix)
        assert tm["carrier_launches"] >= 1 and len(got) >= 10 and _same(got, want), prefix


@pytest.mark.parametrize("M", [130, 200])
def test_partial_tiles_on_both_axes(hip, opt, M):
    """At r2 >= 0.9 no row floods a list; the cut is a multiple of 128, so two = 2 gives the rows behind it the form as well: a diagonal super-tile of
    one whole A tile, and one whose only A tile is partial (130: 2 rows; 200: 72), both with partial column tiles (64-variant tiles: 130 = 2 x 64 + 2,
    200 = 3 x 64 + 8) and the last A tile's rows ending in the zeroed pad behind the carrier rows."""
    util.upload(hip, _iid22(M, N0, SEED))
    f = T.Filters(minR2=0.9)
    got, n_pairs, tm, stats = _run(hip, opt, f, two=2)
    want, _, tm0, _ = _run(hip, opt, f, carrier=0)
    four, _, _, _ = _run(hip, opt, f, three=0)
    assert n_pairs == M * (M - 1) // 2
    assert tm["carrier_launches"] == tm["two_launches"] == tm["count_launches"] >= 1 and tm0["carrier_launches"] == 0, tm
    assert len(got) >= 3 and _same(got, want) and _same(got, four)


def _thinned_pair(p_w, keep, seed):
    """The _iid22 data with one pair planted across tiles: v is the variant that is no copy of another whose allele frequency is nearest
    p_w / keep, and w - written over such a variant of frequency near 0.45 - keeps each of v's alt alleles with probability `keep`.  r2 of (w, v)
    is about keep (1 - pv) / (1 - keep pv); their allele counts differ by a factor 1 / keep, so in allele-count order they lie more than a tile
    apart.  The samples are then reordered so that every carrier of w comes last -> (alleles, v, w, carriers of w)."""
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


@pytest.mark.parametrize("p_w", [0.10, 0.21])
def test_thinned_copy_whose_carriers_lie_behind_a_fixed_stop(hip, opt, p_w):
    """A thinned copy w (r2 ~ 0.65 with its original v) more than a tile from v in allele-count order, the samples ordered so that every
    carrier of w lies behind chunk 80 of 137.  prefix = 2 with prefix_stop = 16 stops every tile there: the prefix
    of the pair holds CH = CQ = 0 and only the suffix margins keep it (screen2c_prefix_keeps).  The recount compares HH + QH and HQ + QQ over
    [0, stop) with what the launch counted - a mismatch fails the call - and the records are those of carrier = 0 without stops."""
    al, v, w, n_carr = _thinned_pair(p_w, 0.7, 5)
    stop_chunks = 16 * 5
    assert n_carr <= al.shape[1] - stop_chunks * 1024 and al[w, : stop_chunks * 1024].sum() == 0
    util.upload(hip, al)
    f = T.Filters(minR2=0.5)
    want, _, _, _ = _run(hip, opt, f, prefix=0, carrier=0)
    got, _, tm, stats = _run(hip, opt, f, prefix=2, prefix_stop=16)
    print(f"p_w={p_w}: pair ({w}, {v}); launches {[(int(x['kind']), int(x['carrier']), int(x['prefix_chunks']), int(x['prefix_chunks_full']), int(x['candidates'])) for x in stats]}")
    assert tm["carrier_launches"] >= 1 and tm["prefix_launches"] == tm["count_launches"] == len(stats), tm      # every launch with stops, none redone
    for x in stats:
        assert int(x["prefix_chunks"]) * NCHUNKS == int(x["prefix_chunks_full"]) * stop_chunks > 0, x
    rec = {(int(r["idxA"]), int(r["idxB"])): r for r in got}.get((min(v, w), max(v, w)))
    assert rec is not None and 0.5 <= rec["R2"] < 0.8, rec
    assert _same(got, want)


def test_every_launch_on_carrier_rows_floods_and_is_redone_with_three_products(hip, opt):
    """two = 2 gives every launch of the walk the form, the rows behind the cut included: at r2 >= 0.1 their lists flood, each is redone with three
    products, and no record is lost or doubled."""
    util.upload(hip, _iid22(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    want, _, tm0, _ = _run(hip, opt, f, carrier=0)
    got, n_pairs, tm, stats = _run(hip, opt, f, two=2, prefix=0)
    assert n_pairs == M0 * (M0 - 1) // 2
    assert tm["carrier_launches"] == tm["two_launches"] >= 2 and tm["three_launches"] >= 1, tm
    assert tm["count_launches"] > tm["two_launches"]                                         # (what flooded ran again)
    assert len(np.unique(got[ORDER])) == len(got) == len(want) and _same(got, want)


def test_shards_of_the_sorted_triangle_make_the_whole(hip, opt):
    util.upload(hip, _iid22(M0, N0, SEED))
    f = T.Filters(minR2=0.1)
    whole, n_pairs, tm, _ = _run(hip, opt, f)
    assert tm["carrier_launches"] >= 1
    parts = [_run(hip, opt, f, part=k, n_parts=3) for k in range(3)]
    assert sum(p[1] for p in parts) == n_pairs == M0 * (M0 - 1) // 2
    assert sum(p[2]["carrier_launches"] for p in parts) >= 1
    assert _same(np.concatenate([p[0] for p in parts]), whole)


def test_carrier_against_the_oracle(hip, opt):
    M = 150
    al = _iid22(M, N0, 33)
    data, mask, variants = util.upload(hip, al)
    want = O.all_pairs(data, None, variants, N0, O.settings(minR2=0.8, unphased=True), vector_only=False)
    got, _, tm, _ = _run(hip, opt, T.Filters(minR2=0.8))
    assert len(want) >= 2 and tm["carrier_launches"] >= 1 and tm["recount_candidates"] >= len(want)
    util.assert_records_match(got, want, variants, double_root=util.double_root_vetter(data, None, variants, N0))


def test_calls_that_never_take_the_form(hip, opt):
    al = _iid22(M0, N0, SEED)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)

    def carrier_launches(mode=MODE, filters=f, **kw):
        hip.timing_reset()
        hip.ld_all(mode, filters, **kw)
        return hip.timing()["carrier_launches"]
    assert carrier_launches() >= 1                                        # (the form is there to be refused)
    assert carrier_launches(mode=T.MODE_PHASED) == 0
    assert carrier_launches(filters=T.Filters(minR2=0.0)) == 0            # cut-off 0: no screen
    assert carrier_launches(window=T.OPT_WINDOW, l_window=30_000) == 0
    assert carrier_launches(tile_variants=256) == 0                       # an explicit tile edge keeps the file order
    for key in ("carrier", "two", "three"):
        opt.set(key, 0)
        assert carrier_launches() == 0, key
        opt.unset(key)
    miss = al[:200].copy()
    miss[::7, ::50, :] = 2                                                # missing genotypes: masked planes
    util.upload(hip, miss)
    assert carrier_launches() == 0
    util.upload(hip, np.ascontiguousarray(al[:, :40_000, :]))             # rows of 40 chunks through the matrix: the walk on H planes
    opt.set("fused", 0)
    hip.timing_reset()
    hip.ld_all(MODE, T.Filters(minR2=0.5))
    tm = hip.timing()
    opt.unset("fused")
    assert tm["carrier_launches"] == 0 and tm["two_launches"] >= 1 and tm["two_launches"] + tm["three_launches"] == tm["count_launches"], tm
