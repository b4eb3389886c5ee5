"""The prefix contraction's fine grid of stops: 128 points, four sub-steps to each of the 32 coarse intervals, of unequal length
where a sub-step is clipped at the next coarse point (csrc/hip/ld_two_screen.h prefix_stop_chunks); the suffix table over those segments
(k_row_suffix_popcount); and the planner's second question, asked in standard deviations (option prefix_sigma).

Rows: 129 chunks (N = 131,500: the shortest row that takes the form) and 137 chunks (N = 140,011: a ragged last word).  On both the coarse
step is 5 chunks and the sub-step 2, so the fine points of a coarse interval lie 0, 2, 4 and 5 chunks behind its start - the last one on
the next coarse point.  M = 420, the inputs of tests.test_gpu_prefix."""
import numpy as np
import pytest

import tomahawk_amd as T
from tests import util
from tests.test_gpu_two import _iid

pytestmark = pytest.mark.gpu
ORDER = ["idxA", "idxB"]
MODE = T.MODE_UNPHASED
M0, SEED = 420, 21
N129, N137 = 131_500, 140_011
STEP, SUB = 5, 2
KEYS = ("prefix", "prefix_stop", "prefix_substop", "prefix_sigma")


def _same(a, b):
    return np.sort(a, order=ORDER).tobytes() == np.sort(b, order=ORDER).tobytes()


def _run(hip, opt, f, **kw):
    """One ld_all under the options given as keywords -> (records, n_pairs, timing, launch log)."""
    for k in kw:
        assert k in KEYS
        opt.set(k, kw[k])
    hip.timing_reset()
    recs, n_pairs, n_rec = hip.ld_all(MODE, f)
    tm = hip.timing()
    log = hip.launch_log()
    for k in kw:
        opt.unset(k)
    assert n_rec == len(recs)
    return recs, n_pairs, tm, log


def test_rows_are_the_lengths_the_module_says():
    for N, chunks in ((N129, 129), (N137, 137)):
        assert (N + 1023) // 1024 == chunks and (chunks + 31) // 32 == STEP and (STEP + 3) // 4 == SUB
    assert N137 % 32 != 0


@pytest.mark.parametrize("N", [N129, N137])
@pytest.mark.parametrize("minR2", [0.1, 0.5])
def test_default_options_give_the_records_of_whole_rows(hip, opt, N, minR2):
    util.upload(hip, _iid(M0, N, SEED))
    f = T.Filters(minR2=minR2)
    got, n_pairs, tm, _ = _run(hip, opt, f)
    want, np0, tm0, _ = _run(hip, opt, f, prefix=0)
    print(f"N={N} r2>={minR2}: prefix launches {tm['prefix_launches']} of {tm['count_launches']}, chunks {tm['prefix_chunks']} of "
          f"{tm['prefix_chunks_full']}, recount candidates {tm['recount_candidates']}, records {len(got)}")
    assert n_pairs == np0 == M0 * (M0 - 1) // 2
    assert tm0["prefix_launches"] == 0 and tm["prefix_launches"] >= 1 and 0 < tm["prefix_chunks"] < tm["prefix_chunks_full"], tm
    assert len(got) >= 3 and _same(got, want)


def _thinned_pair(N, p_w, keep, seed):
    """tests.test_gpu_prefix._thinned_pair at N samples: w, written over an unplanted variant of frequency near 0.45, keeps each alt allele of
    the unplanted variant v whose frequency is nearest p_w / keep with probability `keep` (r2 about keep (1 - pv) / (1 - keep pv)); the samples
    are reordered so that every carrier of w comes last -> (alleles, v, w, carriers of w)."""
    al = _iid(M0, N, SEED).copy()
    rng = np.random.default_rng(seed)
    g = al.sum(axis=2, dtype=np.int16)
    rows = {}
    for x in range(M0):
        rows.setdefault(g[x].tobytes(), []).append(x)
    lone = np.array([x[0] for x in rows.values() if len(x) == 1])
    freq = al.reshape(M0, -1).mean(axis=1)
    v = int(min(lone, key=lambda x: abs(freq[x] - p_w / keep)))
    w = int(min((x for x in lone if x != v), key=lambda x: abs(freq[x] - 0.45)))
    al[w] = al[v] & (rng.random((N, 2), dtype=np.float32) < keep)
    carr = al[w].any(axis=1)
    order = np.argsort(carr, kind="stable")
    return np.ascontiguousarray(al[:, order, :]), v, w, int(carr.sum())


_PAIRS = {}       # (N, p_w) -> (alleles, v, w, carriers, records of prefix = 0, its launches): built once, shared by the sub-stops


@pytest.mark.parametrize("N,p_w,kind", [(N129, 0.10, 5), (N137, 0.10, 5), (N137, 0.21, 1)])
@pytest.mark.parametrize("substop", [1, 2, 3])       # (the sub-stops of one input run one after the other)
def test_ld_that_lies_wholly_behind_a_fine_stop(hip, opt, N, p_w, kind, substop):
    """tests.test_gpu_prefix.test_ld_that_lies_wholly_in_the_unread_part_of_a_stopped_tile at stops that no grid of 32 has: prefix = 2 with
    prefix_stop = 15 and prefix_substop = 1, 2, 3 stops EVERY tile of every launch after 77, 79 and 80 chunks (coarse point 15 is chunk 75;
    the third sub-step, 6 chunks, is clipped at the next coarse point, so its fine index 63 stands for chunk 80 like 64 does).  Every
    carrier of w lies behind chunk 80, so the contracted prefix of (w, v) holds no count of theirs and only the suffix margins at that fine
    index keep the pair: a suffix count that is wrong at a sub-point - a segment of the wrong length, a chunk in the wrong segment - makes the
    bound too small and loses it.  w at p = 0.10 meets v in a two-product tile (kind 5), w at p = 0.21 in a three-product tile (kind 1).  The
    launch log shows every tile at that chunk, no launch was redone, and the records are those of prefix = 0."""
    nchunks = (N + 1023) // 1024
    stop_chunks = 15 * STEP + min(substop * SUB, STEP)
    assert stop_chunks in (77, 79, 80) and stop_chunks % STEP == (0 if substop == 3 else substop * SUB)
    if (N, p_w) not in _PAIRS:
        _PAIRS.clear()                                   # (one at a time, as the inputs themselves)
        al, v, w, n_carr = _thinned_pair(N, p_w, 0.7, 5)
        assert n_carr <= N - 80 * 1024 and al[w, : 80 * 1024].sum() == 0
        util.upload(hip, al)
        want, _, tm0, _ = _run(hip, opt, T.Filters(minR2=0.5), prefix=0)
        _PAIRS[(N, p_w)] = (al, v, w, n_carr, want, tm0["count_launches"])
    al, v, w, n_carr, want, launches0 = _PAIRS[(N, p_w)]
    util.upload(hip, al)
    got, _, tm, (stats, _) = _run(hip, opt, T.Filters(minR2=0.5), prefix=2, prefix_stop=15, prefix_substop=substop)
    print(f"N={N} p_w={p_w} substop={substop}: pair ({w}, {v}), {n_carr} carriers of w; launches "
          f"{[(int(x['kind']), int(x['prefix_chunks']), int(x['prefix_chunks_full']), int(x['candidates'])) for x in stats]}; "
          f"recount candidates {tm['recount_candidates']}, records {len(got)}")
    assert len(stats) == tm["count_launches"] == launches0 == tm["prefix_launches"], tm          # every launch with stops, none redone
    assert kind in [int(x["kind"]) for x in stats]
    for x in stats:
        assert int(x["prefix_chunks_full"]) > 0 and int(x["prefix_chunks"]) * nchunks == int(x["prefix_chunks_full"]) * stop_chunks, x
    by_pair = {(int(r["idxA"]), int(r["idxB"])): r for r in got}
    rec = by_pair.get((min(v, w), max(v, w)))
    assert rec is not None and 0.5 <= rec["R2"] < 0.8, rec
    assert _same(got, want)


@pytest.mark.parametrize("N", [N129, N137])
def test_sigma_rule_never_moves_a_stop_back(hip, opt, N):
    """prefix_sigma = 0 is the planner of the one question (sqrt(bound) x prefix_margin) on the grid of 128; the default asks both and takes
    a pair as decided where either says so, so no tile stops later with it: the chunks contracted are no more, and the records the same."""
    util.upload(hip, _iid(M0, N, SEED))
    f = T.Filters(minR2=0.1)
    both, _, tm, _ = _run(hip, opt, f)
    one, _, tm1, _ = _run(hip, opt, f, prefix_sigma=0)
    print(f"N={N}: chunks {tm['prefix_chunks']} with both questions, {tm1['prefix_chunks']} with the first alone, of {tm['prefix_chunks_full']}")
    assert tm["prefix_launches"] >= 1 and tm1["prefix_launches"] >= 1 and tm["prefix_chunks_full"] == tm1["prefix_chunks_full"]
    assert 0 < tm["prefix_chunks"] <= tm1["prefix_chunks"] < tm1["prefix_chunks_full"], (tm, tm1)
    assert len(both) >= 3 and _same(both, one)
