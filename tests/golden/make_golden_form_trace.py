"""The form trace: which contraction every launch of a fixed list of calls took - four products through a matrix, three, two, the fused
count -> screen - and what the call made of it, on the calls where a launch gives a form up (a candidate list overflows, a launch is too
rich in candidates, a band launch outgrows its buffers), where a later stage or a later call must or must not see that, where a sample
decides, and where a reduce call sits between two record calls.

    python tests/golden/make_golden_form_trace.py [out.json]

writes tests/golden/form_trace.json (or out.json) on an MI355X.  tests/test_gpu_form_trace.py replays the same scenarios against the current
build and compares.  The fixture is recorded from the commit BEFORE a change to how the engine decides a launch's form, never from the code
under test; it uses nothing but the Python binding as that commit has it.

Per call: the launch log as the sequence of kinds (run lengths), the launches' row_pairs and candidates, their carrier, one, prefix_chunks
and prefix_chunks_full columns, n_pairs, n_records, a SHA-256 of the records sorted by (idxA, idxB), and the timing's work counters.  Every
scenario is run twice and only what both runs agree on is kept: a fused launch's candidate count may include slots a wave reserved and did
not use, so it need not repeat.  The kinds, every *_launches counter, the launches' carrier, one and prefix columns, n_pairs, n_records and
the hash must repeat - the generator stops if they do not.  What was dropped is listed in the fixture."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tomahawk_amd as T                                          # noqa: E402
from tests import util                                            # noqa: E402

FIXTURE = os.path.join(HERE, "form_trace.json")
ORDER = ["idxA", "idxB"]
# (tests/test_gpu_lists.py: WORK_FIELDS, and the two-product launches with their carrier rows, their one product and their stops)
WORK_FIELDS = ("count_launches", "fused_launches", "three_launches", "list_launches", "probe_launches", "row_pairs", "three_row_pairs",
               "list_pairs", "probe_pairs", "variant_pairs", "candidates", "recount_candidates", "stats_launches", "two_launches",
               "prefix_launches", "carrier_launches", "one_launches", "prefix_chunks", "prefix_chunks_full")
LAUNCH_FORM_COLUMNS = ("carrier", "one", "prefix_chunks", "prefix_chunks_full")      # of the launch log, beside kind, row_pairs and candidates
MUST_REPEAT = ("kinds", "n_pairs", "n_records", "sha256") + LAUNCH_FORM_COLUMNS      # ... and every *_launches counter
LONG_LOG = 256                                                    # a longer list of row_pairs / candidates is stored as its hash
_DATA = {}


def _data(key, build):
    if key not in _DATA:
        _DATA.clear()                                             # (one data set at a time)
        _DATA[key] = build()
    return _DATA[key]


def _sha(blob):
    return hashlib.sha256(blob).hexdigest()


def _column(values):
    return values if len(values) <= LONG_LOG else {"sha256": _sha(json.dumps(values).encode())}


def trace(hip, name, call):
    """`call` -> (records or None, n_pairs, n_records) between a timing reset and a reading of timing and launch log -> one entry."""
    hip.timing_reset()
    recs, n_pairs, n_records = call()
    tm = hip.timing()
    stats, seen = hip.launch_log()
    kinds = []
    for s in stats:
        if kinds and kinds[-1][0] == int(s["kind"]):
            kinds[-1][1] += 1
        else:
            kinds.append([int(s["kind"]), 1])
    entry = {"call": name, "kinds": kinds, "launches_seen": int(seen),
             "row_pairs": _column([int(s["row_pairs"]) for s in stats]), "candidates": _column([int(s["candidates"]) for s in stats])}
    entry.update({key: _column([int(s[key]) for s in stats]) for key in LAUNCH_FORM_COLUMNS})
    entry.update({"n_pairs": int(n_pairs), "n_records": int(n_records),
                  "sha256": _sha(np.sort(recs, order=ORDER).tobytes()) if recs is not None else None,
                  "work": {k: int(tm[k]) for k in WORK_FIELDS}})
    return entry


class _Options:
    """Engine switches for the length of a `with`; back at their defaults behind it."""
    def __init__(self, hip, **kw):
        self.hip, self.kw = hip, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.hip.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.hip.unset_option(k)


def _all(hip, mode, f, **kw):
    return lambda: hip.ld_all(mode, f, **kw)


def _tile(hip, mode, a0, nA, b0, nB, diag, f):
    def call():
        recs, n_pairs = hip.ld_tile(mode, a0, nA, b0, nB, diag, f)
        return recs, n_pairs, len(recs)
    return call


def two_product_walk(hip):
    """tests/test_gpu_two.py: two products in front of the walk's cut and three behind it; two = 2 floods a two-product list, and the launch
    is redone with three products; the call after that takes two products again."""
    from tests.test_gpu_two import _iid
    util.upload(hip, _iid(700, 40_000, 11))
    f, out = T.Filters(minR2=0.1), []
    with _Options(hip, fused=0):
        out.append(trace(hip, "default", _all(hip, T.MODE_UNPHASED, f)))
        with _Options(hip, two=2):
            out.append(trace(hip, "two = 2", _all(hip, T.MODE_UNPHASED, f)))
        out.append(trace(hip, "default again", _all(hip, T.MODE_UNPHASED, f)))
    return out


def _rich_mosaic():
    return _data("rich", lambda: util.mosaic_alleles(700, 1200, 77, n_founders=4, switch=0.004, mut=0.001))


def three_product_give_up(hip):
    """tests/test_gpu_three.py::test_candidate_rich_launches_fall_back_to_four_products: through the matrix the list overflows and the rest
    of the call takes four products; fused, a launch too rich in candidates ends the form for the call; three = 2 keeps it."""
    util.upload(hip, _rich_mosaic())
    f, out = T.Filters(minR2=0.002), []
    for fused in (0, 1):
        for three in (1, 2):
            with _Options(hip, fused=fused, three=three):
                out.append(trace(hip, "fused = %d, three = %d" % (fused, three), _all(hip, T.MODE_UNPHASED, f, tile_variants=256)))
    return out


def fused_give_up(hip):
    """tests/test_gpu_fused.py::test_fused_candidate_overflow_falls_back_to_the_plain_path: the fused list overflows, the rest of the call
    goes through the matrix; the next region call and a single tile right after an overflowing call start fused again."""
    util.upload(hip, util.mosaic_alleles(900, 300, 5, n_founders=3, switch=0.002, mut=0.0005))
    low, out = T.Filters(minR2=2e-6), []
    for tile in (0, 256):
        out.append(trace(hip, "tile_variants = %d" % tile, _all(hip, T.MODE_PHASED, low, tile_variants=tile)))
    out.append(trace(hip, "the next call", _all(hip, T.MODE_PHASED, T.Filters(minR2=0.5))))
    out.append(trace(hip, "overflowing again", _all(hip, T.MODE_PHASED, low)))
    out.append(trace(hip, "one tile behind it", _tile(hip, T.MODE_PHASED, 0, 300, 0, 300, True, T.Filters(minR2=0.5))))
    return out


def band_launch_outgrown(hip):
    """tests/test_gpu_fused.py::test_band_launches_equal_matrix_sized_tiles, its window shard: a band launch whose candidate list, then whose
    survivor buffer is too small is redone as matrix-sized tiles, those in row strips."""
    from tests.test_gpu_configs import _cohort_alleles
    util.upload(hip, _data("cohort 6000", lambda: _cohort_alleles(6000, 2504, 4242)))
    f, out = T.Filters(minR2=0.1), []
    for mode, name in ((T.MODE_PHASED, "phased"), (T.MODE_UNPHASED, "unphased")):
        call = _all(hip, mode, f, part=2, n_parts=3, window=T.OPT_WINDOW, l_window=25_000)
        with _Options(hip, band_launch=1, band_work_log2=19):
            out.append(trace(hip, name, call))
            for key, value in (("band_list_entries", 64), ("record_cap", 50)):
                with _Options(hip, **{key: value}):
                    out.append(trace(hip, "%s, %s = %d" % (name, key, value), call))
    return out


def default_mode_with_missing_data(hip):
    """tests/test_gpu_fused.py::test_fused_first_pass_of_default_mode_with_missing_data: three stages a call; at a cut-off that floods the
    first stage's list the planner of the later stages must see that the call gave the fused form up."""
    from tests.test_gpu_configs import _cohort_alleles
    util.upload(hip, _cohort_alleles(1300, 1500, 41, miss=True))
    out = []
    for minR2 in (0.2, 2e-6):
        for wopt, name in ((0, "plain"), (T.OPT_R2_SCREEN, "r2 screen")):
            out.append(trace(hip, "%s, minR2 = %g" % (name, minR2), _all(hip, T.MODE_AUTO, T.Filters(minR2=minR2), window=wopt)))
    return out


def sampling(hip):
    """tests/test_gpu_three.py::test_sampling_decides_between_three_and_four_products_on_long_rows, its short rows: unlinked variants take
    three products, a cohort rich in LD four; the samples are in neither log nor timing.  tile_variants = 256 on the 3000-variant cohort:
    78 launches, more than 64, so that every second one is sampled and its neighbour follows it."""
    from tests.test_gpu_configs import _cohort_alleles
    rng = np.random.default_rng(5)
    f, out = T.Filters(minR2=0.1), []
    util.upload(hip, (rng.random((3000, 2504, 2)) < rng.uniform(0.05, 0.5, size=3000)[:, None, None]).astype(np.int8))
    out.append(trace(hip, "unlinked", _all(hip, T.MODE_UNPHASED, f)))
    util.upload(hip, _cohort_alleles(3000, 2504, 99))
    out.append(trace(hip, "cohort", _all(hip, T.MODE_UNPHASED, f)))
    out.append(trace(hip, "cohort, tile_variants = 256", _all(hip, T.MODE_UNPHASED, f, tile_variants=256)))
    return out


def reduce_between_record_calls(hip):
    """An LD score call - four products through a matrix, whatever the options - between two record calls on one context."""
    util.upload(hip, _rich_mosaic())
    f, out = T.Filters(minR2=0.002), []
    def score():
        n, _, n_pairs = hip.ld_score(T.MODE_UNPHASED, f, tile_variants=256)
        return None, n_pairs, int(n.sum())
    out.append(trace(hip, "records", _all(hip, T.MODE_UNPHASED, f, tile_variants=256)))
    out.append(trace(hip, "score", score))
    out.append(trace(hip, "records again", _all(hip, T.MODE_UNPHASED, f, tile_variants=256)))
    return out


def one_product_walk(hip):
    """tests/test_gpu_one_product.py, its smallest shape (137 chunks with a ragged last one, one_rows = 128): rows long enough for the carrier
    plane, one product a pair and the stops.  Each of the walk's options off or forced in turn; cand_cap = 8 floods every screened launch's
    list, so that each is redone down the ladder; the call after that starts with everything again."""
    from tests.test_gpu_one_product import _iid22
    util.upload(hip, _iid22(700, 140_000, 31))
    f, out = T.Filters(minR2=0.1), []
    with _Options(hip, one_rows=128):
        out.append(trace(hip, "default", _all(hip, T.MODE_UNPHASED, f)))
        for name, kw in (("one = 0", dict(one=0)), ("one = 2", dict(one=2)), ("prefix = 0", dict(prefix=0)),
                         ("prefix = 2, prefix_stop = 24", dict(prefix=2, prefix_stop=24)), ("two = 2", dict(two=2)), ("cand_cap = 8", dict(cand_cap=8))):
            with _Options(hip, **kw):
                out.append(trace(hip, name, _all(hip, T.MODE_UNPHASED, f)))
        out.append(trace(hip, "default again", _all(hip, T.MODE_UNPHASED, f)))
    return out


SCENARIOS = {s.__name__: s for s in (two_product_walk, three_product_give_up, fused_give_up, band_launch_outgrown,
                                     default_mode_with_missing_data, sampling, reduce_between_record_calls, one_product_walk)}


def run(hip, name):
    """One scenario on `hip` -> its list of entries; the engine's switches are at their defaults behind it."""
    try:
        return SCENARIOS[name](hip)
    finally:
        for key in list(hip._defaults):
            hip.unset_option(key)


def agreed(name, first, second, dropped):
    """What two runs of a scenario agree on; what they do not is named in `dropped` (or, where it must repeat, stops the generator)."""
    assert [e["call"] for e in first] == [e["call"] for e in second]
    out = []
    for a, b in zip(first, second):
        where = "%s / %s" % (name, a["call"])
        e = dict(a)
        for key in MUST_REPEAT + ("launches_seen",):
            assert a[key] == b[key], "%s: %s differs between two runs of the same commit: %r, %r" % (where, key, a[key], b[key])
        for key in ("row_pairs", "candidates"):
            if a[key] == b[key]:
                continue
            if isinstance(a[key], list):
                e[key] = [x if x == y else None for x, y in zip(a[key], b[key])]
            else:
                e[key] = None
            dropped.append("%s / %s" % (where, key))
        e["work"] = {}
        for key, x in a["work"].items():
            if x == b["work"][key]:
                e["work"][key] = x
            else:
                assert not key.endswith("_launches"), "%s: %s differs between two runs of the same commit: %r, %r" % (where, key, x, b["work"][key])
                dropped.append("%s / work.%s" % (where, key))
        out.append(e)
    return out


def load(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


def differences(want, got):
    """Where a replayed scenario departs from its recorded entries (fields the fixture dropped compare equal to anything)."""
    out = []
    if [e["call"] for e in want] != [e["call"] for e in got]:
        return ["the calls differ: record the fixture again from the parent commit"]
    for w, g in zip(want, got):
        for key in MUST_REPEAT + ("launches_seen", "row_pairs", "candidates"):
            same = w[key] == g[key]
            if isinstance(w[key], list) and isinstance(g[key], list) and key in ("row_pairs", "candidates"):
                same = len(w[key]) == len(g[key]) and all(x is None or x == y for x, y in zip(w[key], g[key]))
            if w[key] is not None and not same:
                out.append("%s: %s recorded %r, now %r" % (w["call"], key, w[key], g[key]))
        for key, x in w["work"].items():
            if g["work"][key] != x:
                out.append("%s: work.%s recorded %r, now %r" % (w["call"], key, x, g["work"][key]))
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    dropped, scenarios = [], {}
    with T.HipLd(0) as engine:
        for scenario in SCENARIOS:
            first = run(engine, scenario)
            scenarios[scenario] = agreed(scenario, first, run(engine, scenario), dropped)
            print("%s: %d calls" % (scenario, len(first)), flush=True)
    with open(path, "w") as fh:
        json.dump({"dropped": dropped, "scenarios": scenarios}, fh, indent=1)
        fh.write("\n")
    print("%d scenarios recorded, %d fields dropped" % (len(scenarios), len(dropped)))
