"""The (U, Z) form of the three-product contraction (option "uz", k_count3_uz_list_t, csrc/hip/ld_count_uz.hip.h): a three-product
launch through a count matrix contracts U = popc(H_A | H_B) and Z = popc((Q_A ^ Q_B) & ~(H_A | H_B)) - two popcounts a word - and its screen
(k_screen3_pairs) derives HH = hA + hB - U and S = qA + qB - Z from them and the margins of the range the tile was contracted over, in integers,
before any test.  Candidates, recount, list math and records are what they were: the records must be those of uz = 0, of the four-product form
(three = 0) and of the oracle; every launch must list as many candidates as the same launch of uz = 0 (the lists themselves never leave the
device: their per-launch sizes, the recount - which fails the call on a candidate whose (HH, S) differ from its own products - and the records
are what a caller sees); and the launches must have run in the form (uz_launches).

Inputs: tests.test_gpu_two._iid - unlinked variants, p ~ U(0.05, 0.5), copies planted among the low-frequency ones - a few hundred variants."""
import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.test_gpu_two import _iid

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
MODE = T.MODE_UNPHASED
KEYS = ("uz", "three", "two", "prefix", "prefix_stop", "prefix_substop", "count_min_chunks", "walk_fine")


def _same(a, b):
    return np.sort(a, order=ORDER).tobytes() == np.sort(b, order=ORDER).tobytes()


def _run(hip, opt, f, **kw):
    """One ld_all under the options given as keywords -> (records, n_pairs, timing, launch log)."""
    keys = [k for k in kw if k in KEYS]
    call = {k: v for k, v in kw.items() if k not in keys}
    for k in keys:
        opt.set(k, kw[k])
    hip.timing_reset()
    recs, n_pairs, n_rec = hip.ld_all(MODE, f, **call)
    tm = hip.timing()
    stats, _ = hip.launch_log()
    for k in keys:
        opt.unset(k)
    assert n_rec == len(recs)
    return recs, n_pairs, tm, stats


def _uz_against_products(hip, opt, f, min_records=3, **kw):
    """The call with uz at its default, at 0 and with four products: same records, the same launches with the same numbers of candidates, and the
    three-product launches through a matrix all in the (U, Z) form -> (records, timing, launch log) of the default."""
    got, n_pairs, tm, stats = _run(hip, opt, f, **kw)
    prod, np0, tm0, stats0 = _run(hip, opt, f, uz=0, **kw)
    four, np4, tm4, _ = _run(hip, opt, f, **{**kw, "three": 0})
    print(f"{kw}: launches {tm['count_launches']} ({tm['two_launches']} two-product, {tm['three_launches']} three-product, {tm['uz_launches']} (U, Z), "
          f"{tm['prefix_launches']} with stops); candidates {tm['candidates']} / {tm0['candidates']}, recounted {tm['recount_candidates']}, records {len(got)}")
    assert n_pairs == np0 == np4 and len(got) >= min_records
    assert _same(got, prod) and _same(got, four)
    assert tm["uz_launches"] > 0 and tm0["uz_launches"] == tm4["uz_launches"] == 0 and tm0["uz_row_pairs"] == 0
    # the form changes what a launch counts and nothing else: the same launches, kinds, work and candidates, launch by launch
    assert tm["uz_launches"] == tm["three_launches"] - tm["fused_launches"] == sum(1 for x in stats if x["uz"]) and not any(x["uz"] for x in stats0)
    assert 0 < tm["uz_row_pairs"] == sum(int(x["row_pairs"]) for x in stats if x["uz"]) <= tm["three_row_pairs"]
    assert all(int(x["kind"]) == 1 for x in stats if x["uz"])
    for k in ("count_launches", "two_launches", "three_launches", "three_row_pairs", "row_pairs", "prefix_launches", "prefix_chunks", "candidates", "recount_candidates"):
        assert tm[k] == tm0[k], (k, tm[k], tm0[k])
    assert [(int(x["kind"]), int(x["row_pairs"]), int(x["candidates"]), int(x["prefix_chunks"])) for x in stats] == \
           [(int(x["kind"]), int(x["row_pairs"]), int(x["candidates"]), int(x["prefix_chunks"])) for x in stats0]
    return got, tm, stats


def _against_the_oracle(hip, opt, al, N, minR2, n_sub=90, **kw):
    """... and the first variants against the oracle (it is scalar), in the (U, Z) form."""
    M = al.shape[0]
    sub = np.arange(min(n_sub, M))      # (the head of the file order: _iid plants its first copies a few places behind their originals)
    data, mask, variants = util.upload(hip, np.ascontiguousarray(al[sub]))
    want = O.all_pairs(data, None, variants, N, O.settings(minR2=minR2, unphased=True), vector_only=False)
    got, _, tm, _ = _run(hip, opt, T.Filters(minR2=minR2), **kw)
    assert tm["uz_launches"] > 0 and tm["recount_candidates"] >= len(want)
    util.assert_records_match(got, want, variants, double_root=util.double_root_vetter(data, None, variants, N))
    return len(want)


@pytest.mark.parametrize("N", [140_288, 131_136])
def test_whole_chunks_and_a_single_live_half_slot(hip, opt, N):
    """N = 140,288: rows of 137 whole chunks.  N = 131,136: 128 chunks + 2 words - the last chunk holds one live half-slot, and the slot it lies in
    is contracted by contract_uz_slot.  The sorted walk (default: two-product launches in front of its cut, (U, Z) launches behind it) and the
    file-order walk (two = 0: every launch in the form)."""
    M = 333
    al = _iid(M, N, 21)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)
    got, tm, _ = _uz_against_products(hip, opt, f)
    file_order, tm2, _ = _uz_against_products(hip, opt, f, two=0)
    assert _same(got, file_order) and tm2["uz_launches"] == tm2["count_launches"]
    assert _against_the_oracle(hip, opt, al, N, 0.3) >= 1


@pytest.mark.parametrize("extra_words", [18, 20, 21, 24])
def test_last_chunk_with_nine_to_twelve_live_half_slots(hip, opt, extra_words):
    """Rows of 128 chunks + 18, 20, 21 and 24 words: 9, 10, 11 and 12 live half-slots of 8 bytes in the last chunk - odd and even counts of slots for
    the rolled loop over contract_uz_slot, with and without a half-slot of padding inside the last one.  Against the run that contracts the
    padding too (skip_pad = 0: the unrolled chunk), which adds nothing to U or Z."""
    N = 131_072 + 32 * extra_words
    assert 9 <= (extra_words + 1) // 2 <= 12
    M = 200
    util.upload(hip, _iid(M, N, 33 + extra_words))
    f = T.Filters(minR2=0.1)
    got, tm, _ = _uz_against_products(hip, opt, f, two=0)
    opt.set("skip_pad", 0)
    padded, _, tm_p, _ = _run(hip, opt, f, two=0)
    opt.unset("skip_pad")
    assert tm_p["uz_launches"] > 0 and _same(got, padded)


@pytest.mark.parametrize("min_chunks", [8, 1])
def test_tiles_split_along_k(hip, opt, min_chunks):
    """N = 300,000: rows of 293 chunks, and the last tiles of a launch are cut along K - their parts of U and Z added into the matrix with atomics
    (StoreCounts3's epilogue over tiles k_zero_tiles zeroed); count_min_chunks = 1 cuts them finer.  Small tiles make several launches."""
    N, M = 300_000, 260
    al = _iid(M, N, 4242)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)
    _, tm, _ = _uz_against_products(hip, opt, f, two=0, count_min_chunks=min_chunks, tile_variants=128)
    assert tm["uz_launches"] >= 6 and tm["fused_launches"] == 0
    # tiles were cut along K, and finer with count_min_chunks = 1: units beyond one a tile, whose parts reach the matrix through the atomics
    print(f"count_min_chunks {min_chunks}: {tm['uz_split_units']} units beyond one a tile in {tm['uz_launches']} launches")
    assert tm["uz_split_units"] > 0
    if min_chunks == 1:
        coarse = _run(hip, opt, f, two=0, count_min_chunks=8, tile_variants=128)[2]
        assert tm["uz_split_units"] > coarse["uz_split_units"] > 0
    _uz_against_products(hip, opt, f, count_min_chunks=min_chunks)
    if min_chunks == 1:
        assert _against_the_oracle(hip, opt, al, N, 0.3, n_sub=70, count_min_chunks=1) >= 1


@pytest.mark.parametrize("N,stop,substop", [(140_288, 16, 0), (140_288, 15, 2), (263_168, 16, 1), (263_168, 24, 3)])
def test_forced_prefix_stops(hip, opt, N, stop, substop):
    """Rows of 137 and of 257 chunks (the fine walk begins at 256), prefix = 2 with prefix_stop / prefix_substop: every tile of every launch stops at
    that point of the grid, coarse or not (chunks 80 and 79 of 137, 130 and 199 of 257), and the screen converts the prefix's (U, Z) with the rows' popcounts minus the suffix margins at the stop.
    The recount proves each candidate's converted (HH, S) against its own products over the chunks the tile read (a difference fails the call)."""
    M = 300
    al = _iid(M, N, 21 + stop)
    util.upload(hip, al)
    f = T.Filters(minR2=0.5)      # (as the prefix tests: at 0.5 a stop this early still decides the unlinked pairs, and no list floods)
    got, tm, stats = _uz_against_products(hip, opt, f, prefix=2, prefix_stop=stop, prefix_substop=substop)
    assert tm["prefix_launches"] == tm["count_launches"] and 0 < tm["prefix_chunks"] < tm["prefix_chunks_full"], tm
    assert any(x["uz"] and 0 < int(x["prefix_chunks"]) < int(x["prefix_chunks_full"]) for x in stats)      # a (U, Z) launch with stops
    whole, _, _, _ = _run(hip, opt, f, prefix=0)
    assert _same(got, whole)
    assert _against_the_oracle(hip, opt, al, N, 0.3, n_sub=70, prefix=2, prefix_stop=stop, prefix_substop=substop) >= 1


@pytest.mark.parametrize("M", [201, 333])
def test_variant_counts_that_are_no_multiple_of_the_tile(hip, opt, M):
    """M no multiple of 64, the (U, Z) tile's edge in variants: diagonal tiles, and the rows and columns beyond the last variant are zero padding,
    whose U and Z are the popcounts of the other row alone - the screen never looks at them.  Single tiles with odd origins as well."""
    N = 140_288
    al = _iid(M, N, 5 + M)
    util.upload(hip, al)
    f = T.Filters(minR2=0.1)
    _uz_against_products(hip, opt, f, two=0)
    _uz_against_products(hip, opt, f, two=0, tile_variants=128)
    for a0, nA, b0, nB, diag in ((0, M, 0, M, True), (3, M // 5 + 1, M // 4 + 2, M // 3 + 11, False), (65, 100, 65, M - 65, True)):
        res = {}
        for uz in (1, 0):
            opt.set("uz", uz); opt.set("three", 2)
            hip.timing_reset()
            res[uz] = hip.ld_tile(MODE, a0, nA, b0, nB, diag, f)[0]
            assert (hip.timing()["uz_launches"] > 0) == bool(uz)
        opt.set("three", 0)
        four = hip.ld_tile(MODE, a0, nA, b0, nB, diag, f)[0]
        opt.unset("three"); opt.unset("uz")
        assert _same(res[1], res[0]) and _same(res[1], four), (a0, nA, b0, nB)
    assert _against_the_oracle(hip, opt, al, N, 0.3, two=0) >= 1


def test_candidates_by_chance_are_recounted_without_a_mismatch(hip, opt):
    """A cut-off at which about 1 pair in 500 is a candidate by chance.  The screen drops a pair only when both extreme phasings of its double hets
    leave r2 under the cut-off (e_lo at n11's least value, e_hi at its greatest, HH further on), so an unlinked pair of common variants passes near
    r2 ~ 0.05: the cut-off is the 0.998 quantile, over the pairs of this input, of max(e_lo^2, e_hi^2) / (dA rA dB rB) - the screen's own
    statistic (csrc/hip/ld_two_screen.h: screen_keeps_between, restated here on counts from NumPy).  Between 1 pair in 1000 and 1 in 300 must
    then be a candidate; every one is recounted from its rows, and k_recount_unphased compares the (HH, S) the screen derived from (U, Z) with
    the candidate's own products - pair by pair - and fails the call on a difference.  The list (room for max(pairs / 128, 4096) entries) holds."""
    N, M = 140_288, 420
    al = _iid(M, N, 21)
    util.upload(hip, al)
    g = al.sum(axis=2, dtype=np.int8)
    H, Q = (g == 1).astype(np.float32), (g == 2).astype(np.float32)      # (counts below 2^24: exact in float32)
    hh = (H @ H.T).astype(np.float64)
    qc = Q @ (H + Q).T
    s = (qc + qc.T).astype(np.float64)
    d = (H.sum(axis=1, dtype=np.float64) + 2.0 * Q.sum(axis=1, dtype=np.float64))
    T2n = 2.0 * N
    r = T2n - d
    e_lo = ((r[:, None] - d[None, :]) + s) * T2n - r[:, None] * r[None, :]
    e_hi = ((r[:, None] - d[None, :]) + s + hh) * T2n - r[:, None] * r[None, :]
    stat = np.maximum(e_lo ** 2, e_hi ** 2) / ((d * r)[:, None] * (d * r)[None, :])
    iu = np.triu_indices(M, 1)
    pairs = len(iu[0])
    cut = float(np.sort(stat[iu])[-(pairs // 500)])
    assert 0.02 < cut < 0.1, cut
    f = T.Filters(minR2=cut)
    got, n_pairs, tm, stats = _run(hip, opt, f, two=0, three=2)
    four, _, _, _ = _run(hip, opt, f, three=0)
    prod, _, tm0, _ = _run(hip, opt, f, two=0, three=2, uz=0)
    print(f"cut {cut:.4f}: candidates {tm['candidates']} of {pairs} pairs (1 in {pairs / max(tm['candidates'], 1):.0f}), recounted {tm['recount_candidates']}, records {len(got)}")
    assert n_pairs == pairs and tm["uz_launches"] == tm["count_launches"] == len(stats) >= 1 and tm0["uz_launches"] == 0
    assert 0 < pairs // 1000 <= tm["candidates"] <= pairs // 300
    assert all(int(x["candidates"]) < max(int(x["row_pairs"]) // 4 // 128, 4096) for x in stats)      # under the list's capacity: nothing was redone
    assert tm["recount_candidates"] == tm["candidates"] == tm0["candidates"] >= len(got) >= 3
    assert _same(got, four) and _same(got, prod)
