"""The two-product form of the unphased contraction: an unscreened `-u` call over the whole triangle walks the
allele-count-sorted planes, and the launches over rows with few hom-alt carriers contract HH = popc(H_A & H_B) and HQ = popc(H_A & Q_B) only
(k_count_list_t over the row variants' H planes against the column variants' H and Q rows); S = QH + HQ + 2 QQ is bounded from the margins
(csrc/hip/ld_two_screen.h, k_screen2_pairs) and the pairs that pass are recounted with four products (k_recount_unphased).  The records must
be those of the four-product form (three = 0) and of the file-order walk (two = 0), byte for byte, and those of the oracle.

Inputs: unlinked variants, p ~ U(0.05, 0.5) as in the headline, with a handful of copies planted among the low-frequency variants so that
the recount runs.  At r2 >= 0.1 the rows up to p ~ 0.16 take the form (the first 128 of 700 sorted variants: one row of A tiles); at
r2 >= 0.5 those up to p ~ 0.3, at r2 >= 0.8 every row."""
import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
MODE = T.MODE_UNPHASED
_DATA = {}


def _iid(M, N, seed):
    """(M, N, 2) alleles: iid, p ~ U(0.05, 0.5); of the variants with p < 0.15 every fifth is followed (in file order, some places on) by a
    copy of itself - exact, or with a per-mille of its alleles flipped, or with its two haplotypes swapped.  Built once per shape."""
    key = (M, N, seed)
    if key not in _DATA:
        _DATA.clear()                                    # (one data set at a time: the large ones are a quarter of a gigabyte)
        rng = np.random.default_rng(seed)
        p = rng.uniform(0.05, 0.5, size=M)
        al = np.empty((M, N, 2), dtype=np.int8)
        for v in range(M):
            al[v] = (rng.random((N, 2), dtype=np.float32) < p[v])
        low = np.flatnonzero(p < 0.15)[::5]
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


def _run(hip, opt, f, two=None, three=None, **kw):
    """One ld_all under the given options -> (records, n_pairs, timing, launch log)."""
    for key, val in (("two", two), ("three", three)):
        if val is None:
            opt.unset(key)
        else:
            opt.set(key, val)
    hip.timing_reset()
    recs, n_pairs, n_rec = hip.ld_all(MODE, f, **kw)
    tm = hip.timing()
    log = hip.launch_log()
    opt.unset("two"); opt.unset("three")
    assert n_rec == len(recs)
    return recs, n_pairs, tm, log


def _check_against_both(hip, opt, f, M, expect_two=True, min_records=3):
    got, n_pairs, tm, _ = _run(hip, opt, f)
    four, np4, tm4, _ = _run(hip, opt, f, three=0)
    file_order, np0, tm0, _ = _run(hip, opt, f, two=0)
    assert n_pairs == np4 == np0 == M * (M - 1) // 2
    assert tm4["two_launches"] == tm4["three_launches"] == 0 and tm0["two_launches"] == 0
    assert len(got) >= min_records and _same(got, four) and _same(got, file_order)
    if expect_two:
        assert tm["two_launches"] >= 1 and tm["two_launches"] + tm["three_launches"] == tm["count_launches"], tm
        assert tm["recount_candidates"] >= min_records
    return got, tm


@pytest.mark.parametrize("N", [40_000, 40_000 + 32 * 18])
def test_two_products_on_rows_with_a_ragged_last_chunk(hip, opt, N):
    """fused = 0 sends rows this short through the count matrix: 39 chunks + 1 live half-slot, and + 9 half-slots more."""
    M = 700
    util.upload(hip, _iid(M, N, 11))
    opt.set("fused", 0)
    _check_against_both(hip, opt, T.Filters(minR2=0.1), M)
    opt.set("skip_pad", 0)
    padded, _, tm, _ = _run(hip, opt, T.Filters(minR2=0.1))
    opt.unset("skip_pad")
    plain, _, _, _ = _run(hip, opt, T.Filters(minR2=0.1), two=0)
    assert tm["two_launches"] >= 1 and _same(padded, plain)


@pytest.mark.parametrize("min_chunks", [8, 1])
def test_two_products_on_long_rows_with_tiles_split_along_k(hip, opt, min_chunks):
    """N = 300,000: rows of 293 chunks - no fused form, and the last tiles of a launch are cut along K, their (HH, HQ) added into zeroed
    tiles with atomics.  M = 420 at r2 >= 0.5: the first 256 sorted rows take the form."""
    N, M = 300_000, 420
    util.upload(hip, _iid(M, N, 12))
    opt.set("count_min_chunks", min_chunks)
    _, tm = _check_against_both(hip, opt, T.Filters(minR2=0.5), M)
    assert tm["fused_launches"] == 0
    _check_against_both(hip, opt, T.Filters(minR2=0.1), M, expect_two=False)      # (r* lies below the first tile edge: three products, same records)


@pytest.mark.parametrize("M", [130, 200])
def test_two_products_on_less_than_two_row_tiles(hip, opt, M):
    """M = 130: a whole A tile and two rows of the next, column tiles of 64 variants with a partial last one; M = 200: a diagonal super-tile
    with partial tiles on both axes.  r2 >= 0.9, where every row may take the form (at 0.5 the cut lies at p ~ 0.3, inside the first A tile
    of so few variants); the planted pairs are the survivors."""
    N = 40_000
    util.upload(hip, _iid(M, N, 13 + M))
    opt.set("fused", 0)
    _check_against_both(hip, opt, T.Filters(minR2=0.9), M, min_records=1)
    _check_against_both(hip, opt, T.Filters(minR2=0.1), M, expect_two=False, min_records=1)


def test_two_everywhere_floods_the_list_and_falls_back(hip, opt):
    """two = 2 gives every launch of the walk the form.  At r2 >= 0.1 the rows above the edge (p > 0.17) pass nearly every pair: the list
    of such a launch overflows, the launch is redone with three products, and the records are the same - none twice, none lost."""
    N, M = 40_000, 700
    util.upload(hip, _iid(M, N, 11))
    opt.set("fused", 0)
    f = T.Filters(minR2=0.1)
    want, _, _, _ = _run(hip, opt, f, two=0)
    got, n_pairs, tm, _ = _run(hip, opt, f, two=2)
    assert n_pairs == M * (M - 1) // 2 and tm["two_launches"] >= 1 and tm["three_launches"] >= 1
    assert len(np.unique(got[ORDER])) == len(got) == len(want) and _same(got, want)


def test_cut_offs_on_and_next_to_existing_r2_values(hip, opt):
    N, M = 40_000, 700
    util.upload(hip, _iid(M, N, 11))
    opt.set("fused", 0)
    base, _, _, _ = _run(hip, opt, T.Filters(minR2=0.05), two=0)
    r2 = np.unique(base["R2"]); r2 = r2[(r2 < 1) & (r2 > 0.1)]
    assert len(r2) >= 3
    for x in r2[:: max(1, len(r2) // 3)][:3]:
        for cut in (np.nextafter(x, 0.0), x, np.nextafter(x, 1.0)):
            f = T.Filters(minR2=float(cut))
            got, _, tm, _ = _run(hip, opt, f)
            want, _, _, _ = _run(hip, opt, f, two=0)
            assert tm["two_launches"] >= 1 and _same(got, want), cut


def test_shards_of_the_sorted_triangle_make_the_whole(hip, opt):
    N, M = 40_000, 700
    util.upload(hip, _iid(M, N, 11))
    opt.set("fused", 0)
    f = T.Filters(minR2=0.1)
    whole, n_pairs, tm, _ = _run(hip, opt, f)
    assert tm["two_launches"] >= 1
    parts = [_run(hip, opt, f, part=k, n_parts=3) for k in range(3)]
    assert sum(p[1] for p in parts) == n_pairs == M * (M - 1) // 2
    assert sum(p[2]["two_launches"] for p in parts) >= 1
    assert _same(np.concatenate([p[0] for p in parts]), whole)


def test_launch_log_and_accounting(hip, opt):
    """Kind 5 for the launches in front of r*, kind 1 behind it, in that order; a two-product launch's row_pairs are the plane-row pairs it
    contracted (128 x 128 a tile: one row x two rows per variant pair) and no part of three_row_pairs; the samples are in neither."""
    N, M = 40_000, 700
    util.upload(hip, _iid(M, N, 11))
    opt.set("fused", 0)
    _, _, tm, (stats, seen) = _run(hip, opt, T.Filters(minR2=0.1))
    kinds = [int(x["kind"]) for x in stats]
    assert seen == len(stats) == tm["count_launches"] == tm["two_launches"] + tm["three_launches"]
    assert set(kinds) == {5, 1} and kinds == sorted(kinds, reverse=True), kinds
    assert kinds.count(5) == tm["two_launches"] and kinds.count(1) == tm["three_launches"]
    assert sum(int(x["row_pairs"]) for x in stats) == tm["row_pairs"]
    assert sum(int(x["row_pairs"]) for x in stats if x["kind"] == 1) == tm["three_row_pairs"]
    # the first 128 sorted rows against all 700 columns, diagonal: column tiles of 64 variants -> 11 tiles of 128 x 128 plane-row pairs
    assert sum(int(x["row_pairs"]) for x in stats if x["kind"] == 5) == 11 * 128 * 128


def test_calls_that_never_take_the_form(hip, opt):
    N, M = 40_000, 700
    al = _iid(M, N, 11)
    util.upload(hip, al)
    opt.set("fused", 0)
    f = T.Filters(minR2=0.1)
    def two_launches(mode=MODE, filters=f, **kw):
        hip.timing_reset()
        hip.ld_all(mode, filters, **kw)
        return hip.timing()["two_launches"]
    assert two_launches() >= 1                                            # (the form is there to be refused)
    opt.set("three", 2)
    assert two_launches() == 0
    opt.unset("three")
    assert two_launches(tile_variants=256) == 0
    assert two_launches(window=T.OPT_WINDOW, l_window=30_000) == 0
    assert two_launches(mode=T.MODE_PHASED) == 0
    assert two_launches(filters=T.Filters(minR2=0.0)) == 0
    opt.unset("fused")
    assert two_launches() == 0                                            # rows short enough to fuse
    opt.set("fused", 0)
    miss = al[:300].copy()
    miss[::7, ::50, :] = 2                                                # missing genotypes: masked planes
    util.upload(hip, miss)
    assert two_launches() == 0


def test_two_products_against_the_oracle(hip, opt):
    """220 variants at r2 >= 0.8, where every row may take the form: the first 128 sorted rows in a two-product launch, the rest with three
    products; the survivors are the planted pairs."""
    N, M = 40_000, 220
    al = _iid(M, N, 14)
    data, mask, variants = util.upload(hip, al)
    opt.set("fused", 0)
    want = O.all_pairs(data, None, variants, N, O.settings(minR2=0.8, unphased=True), vector_only=False)
    got, _, tm, _ = _run(hip, opt, T.Filters(minR2=0.8))
    assert len(want) >= 3 and tm["two_launches"] >= 1 and tm["recount_candidates"] >= len(want)
    util.assert_records_match(got, want, variants, double_root=util.double_root_vetter(data, None, variants, N))
