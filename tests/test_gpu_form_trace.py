"""Which form every launch takes, call by call: the scenarios of tests/golden/make_golden_form_trace.py - a two-product list that overflows, a
three-product and a fused list that overflow, a band launch that outgrows its buffers, the three stages of a default-mode call, the samples'
decision (every launch's own, and every second launch's of a plan of 78), a reduce call between two record calls, the carrier, one-product
and prefix launches of the two-product walk on long rows with each of their options off or forced - replayed on the current build and compared
with tests/golden/form_trace.json, which the commit before the sample ladder moved into csrc/hip/ld_form.h (decide_wants) recorded: the kinds
of the launches in order, their row_pairs and candidates, their carrier, one and prefix columns, n_pairs, n_records, the records' hash and the
timing's work counters."""
import pytest

from tests.golden import make_golden_form_trace as trace


@pytest.mark.gpu
@pytest.mark.parametrize("scenario", list(trace.SCENARIOS))
def test_every_launch_takes_the_form_it_took_before(hip, opt, scenario):
    want = trace.load()["scenarios"][scenario]
    got = trace.run(hip, scenario)
    different = trace.differences(want, got)
    for line in different[:20]:
        print(line)
    assert not different, "%d fields differ from the recorded trace" % len(different)


def _kinds(entry):
    return [k for k, n in entry["kinds"] for _ in range(n)]


def test_the_fixture_holds_the_transitions_it_is_for():
    """What the trace is there to pin, read off the fixture alone (no device): 0 four products through a matrix, 1 three, 2 fused PhasedMath,
    3 / 4 fused UnphasedMath with four / three products, 5 two products."""
    fixture = trace.load()
    s = {name: {e["call"]: e for e in entries} for name, entries in fixture["scenarios"].items()}
    assert sorted(s) == sorted(trace.SCENARIOS)
    for name in fixture["dropped"]:                      # only what a fused launch's reserved slots make unrepeatable
        assert name.endswith("candidates"), name
    for entries in s.values():
        for e in entries.values():
            assert e["kinds"] and e["n_pairs"] > 0
            assert {"count_launches", "fused_launches", "three_launches", "two_launches", "list_launches", "probe_launches", "stats_launches"} <= set(e["work"])
    two = s["two_product_walk"]
    assert _kinds(two["default"]) == [5, 1] == _kinds(two["default again"]) and _kinds(two["two = 2"]) == [5, 5, 1]
    assert two["default"]["sha256"] == two["two = 2"]["sha256"] == two["default again"]["sha256"] and two["default"]["work"] == two["default again"]["work"]
    three = s["three_product_give_up"]
    assert _kinds(three["fused = 0, three = 1"]) == [0] * 6 and _kinds(three["fused = 1, three = 1"]) == [3] * 6 and _kinds(three["fused = 1, three = 2"]) == [4] * 6
    assert _kinds(three["fused = 0, three = 2"]) == [1, 1, 0, 1, 0, 1, 0, 0]       # a list overflows, the launches in flight behind it too, the rest of the call four products
    assert len({e["sha256"] for e in three.values()}) == 1
    fused = s["fused_give_up"]
    assert _kinds(fused["tile_variants = 0"]) == [2, 2, 0] == _kinds(fused["overflowing again"]) and _kinds(fused["tile_variants = 256"])[-6:] == [0] * 6
    assert _kinds(fused["the next call"]) == [2] == _kinds(fused["one tile behind it"])
    band = s["band_launch_outgrown"]
    assert _kinds(band["phased"]) == [2] and _kinds(band["phased, band_list_entries = 64"]) == [2, 2] and band["phased, record_cap = 50"]["launches_seen"] > 1000
    assert band["unphased"]["sha256"] == band["unphased, band_list_entries = 64"]["sha256"] == band["unphased, record_cap = 50"]["sha256"]
    missing = s["default_mode_with_missing_data"]
    assert _kinds(missing["plain, minR2 = 0.2"]) == [2, 0, 0] and _kinds(missing["plain, minR2 = 2e-06"]) == [2, 2, 0, 0, 0]
    sampled = s["sampling"]
    assert _kinds(sampled["unlinked"]) == [4] and _kinds(sampled["cohort"]) == [3]
    assert sampled["unlinked"]["launches_seen"] == sampled["unlinked"]["work"]["count_launches"] == 1       # the samples are in neither
    many = sampled["cohort, tile_variants = 256"]
    assert many["launches_seen"] == many["work"]["count_launches"] == 78 > 64 and set(_kinds(many)) == {3, 4}      # every second launch sampled, both answers given
    assert many["sha256"] == sampled["cohort"]["sha256"]
    between = s["reduce_between_record_calls"]
    assert set(_kinds(between["score"])) == {0} and between["score"]["work"]["fused_launches"] == 0
    assert {k: v for k, v in between["records"].items() if k != "call"} == {k: v for k, v in between["records again"].items() if k != "call"}
    one = s["one_product_walk"]
    assert not [name for name in fixture["dropped"] if name.startswith("one_product_walk")]                 # no fused launch: everything repeats
    default = one["default"]
    assert sum(default["one"]) == default["work"]["one_launches"] >= 1 and default["work"]["carrier_launches"] > default["work"]["one_launches"]
    assert default["work"]["prefix_launches"] > 0 and 0 < default["work"]["prefix_chunks"] < default["work"]["prefix_chunks_full"]
    assert one["one = 0"]["work"]["one_launches"] == 0 and not any(one["one = 0"]["one"])
    assert len({e["sha256"] for e in one.values()}) == 1 and len(one) == 8
    assert one["prefix = 0"]["work"]["prefix_launches"] == 0 and _kinds(one["two = 2"]).count(5) > _kinds(default).count(5)
    capped = one["cand_cap = 8"]                          # the first launch's list holds 8 of its 28 candidates: redone, the next entry of the log, rung by rung
    assert _kinds(capped)[:5] == [5, 5, 5, 1, 0] and capped["candidates"][:4] == [28] * 4 and capped["one"][:3] == [1, 1, 0] and capped["carrier"][:3] == [1, 1, 1]
    assert capped["prefix_chunks_full"][0] > 0 == capped["prefix_chunks_full"][1]       # ... first over whole rows in the same form
    again = one["default again"]
    assert _kinds(again) == _kinds(default) and again["work"] == default["work"] and all(again[key] == default[key] for key in trace.LAUNCH_FORM_COLUMNS)
