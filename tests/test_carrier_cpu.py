"""The host side of the carrier plane as the two-product walk's row operand, without a GPU: the extended `make two-check`,
`make prefix-check` and `make form-check` (csrc/hip/ld_two_screen.h: screen2c_*, csrc/hip/ld_plan.h: PlanEnv::carrier, csrc/hip/ld_form.h:
LaunchForm::carrier, carrier_operand) under AddressSanitizer and UBSan, and the planner's cut through the library's entry."""
import os
import re
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(target):
    r = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout


def test_carrier_screen_lies_between_three_products_and_the_h_plane():
    """Every 3 x 3 table of up to 7 samples: the true S and T inside the carrier interval, the interval inside the H form's (a failed check fails
    the tool), and kept(three) <= kept(carrier) <= kept(H) - strictly, over all the tests."""
    out = _make("two-check")
    m = re.search(r"two-check: carrier screen kept (\d+) of the same tests \(three products (\d+) <= carrier <= H plane (\d+)\)", out)
    assert m, out[-2000:]
    kc, k3, k2 = (int(x) for x in m.groups())
    assert 0 < k3 < kc < k2
    assert re.search(r"two-check: \d+ cases, 0 bad", out)


@pytest.fixture(scope="module")
def prefix_output():
    out = _make("prefix-check")
    assert "prefix-check: ok" in out
    return out


def test_carrier_prefix_screen_over_every_prefix_and_suffix_table(prefix_output):
    m = re.search(r"the two-product prefix screen on the carrier plane keeps (\d+) \(three products on the whole rows (\d+) <= it <= the H plane's (\d+)\)", prefix_output)
    assert m, prefix_output[-2000:]
    kc, k3, k2 = (int(x) for x in m.groups())
    assert 0 < k3 < kc < k2
    assert re.search(r"violations 0\b", prefix_output)


def test_planner_report_of_the_carrier_form_on_the_headlines_law(prefix_output):
    """1,000,000 samples x 50,000 variants, p over (0.05, 0.5), r2 >= 0.1: more rows in front of the cut than the H plane's report has (p ~ 0.21
    for ~ 0.16), more of the walk's steps with two products, and less count work.  The arithmetic on expectations behind the form gives 0.946 of
    the H plane's work; the planner's own figure is held to +- 0.02 of it (tile edges and the rounding of the margins move it by less)."""
    h = re.search(r"planner: .* two-product cut at sorted row (\d+) \(p = ([0-9.]+)\); (\d+) launches", prefix_output)
    c = re.search(r"carrier form: .* two-product cut at sorted row (\d+) \(p = ([0-9.]+)\); (\d+) steps", prefix_output)
    assert h and c, prefix_output[-3000:]
    assert int(c.group(1)) > int(h.group(1)) and int(c.group(1)) % 128 == 0
    assert 0.14 < float(h.group(2)) < 0.175 and 0.20 < float(c.group(2)) < 0.23
    steps = re.findall(r"carrier form: step +(\d+) +(two|three) +rows +(\d+)\+(\d+) .* contracted ([0-9.]+) of the rows", prefix_output)
    assert len(steps) == int(c.group(3)) and [x[1] for x in steps] == sorted((x[1] for x in steps), reverse=True)
    assert all(int(x[2]) + int(x[3]) <= int(c.group(1)) for x in steps if x[1] == "two") and all(int(x[2]) >= int(c.group(1)) for x in steps if x[1] == "three")
    assert all(0.2 < float(x[4]) <= 1.0 for x in steps)
    m = re.search(r"carrier form: rows in front of the cut (\d+) \(H plane: (\d+)\); count work with stops ([0-9.]+) of the H plane's with stops", prefix_output)
    assert m and int(m.group(1)) == int(c.group(1)) and int(m.group(2)) == int(h.group(1))
    assert 0.926 < float(m.group(3)) < 0.966, m.group(0)
    # the first report's count work stands as it was: the second one's lines do not read as its own
    assert len(re.findall(r"planner: count work", prefix_output)) == 1


def test_form_check_covers_the_carrier_rung():
    out = _make("form-check")
    m = re.search(r"form-check: (\d+) cases, (\d+) bad", out)
    assert m and int(m.group(1)) >= 3000 and int(m.group(2)) == 0, out[-2000:]


def test_planner_entry_takes_the_row_operand_and_defaults_to_the_h_plane():
    M, N = 5000, 1_000_000
    p = np.sort(np.random.default_rng(0).uniform(0.05, 0.5, size=M))
    het = np.round(2 * p * (1 - p) * N).astype(np.uint32)
    hom = np.round(p * p * N).astype(np.uint32)
    meta = np.zeros(M, dtype=T.META_DTYPE)
    meta["pos"] = np.arange(M, dtype=np.uint32) * 100 + 1000
    meta["ac"] = 5

    def plan(**kw):
        return T.plan_region(meta, N, 0, M, 0, M, True, planes_per_variant=2, k_chunks=(N + 1023) // 1024, minR2=0.1, phased_math=False, het=het, hom=hom, **kw)
    h, c = plan(), plan(carrier=True)
    assert plan(carrier=False)["two_end"] == h["two_end"]
    assert h["two_end"] % 128 == 0 and c["two_end"] % 128 == 0 and 0.14 < p[h["two_end"]] < 0.175 and 0.20 < p[c["two_end"]] < 0.23, (h["two_end"], c["two_end"])
    # no launch straddles the carrier form's cut either, and the plans cover the same pairs
    assert h["n_pairs"] == c["n_pairs"] == M * (M - 1) // 2
    for t in c["tiles"]:
        a0, nA = int(t["rowA0"]), int(t["nA"])
        assert a0 + nA <= c["two_end"] or a0 >= c["two_end"]
    # the cut does not fall when the cut-off rises
    ends = [T.plan_region(meta, N, 0, M, 0, M, True, planes_per_variant=2, k_chunks=977, minR2=r2, phased_math=False, het=het, hom=hom, carrier=True)["two_end"] for r2 in (0.02, 0.1, 0.3, 0.8)]
    assert ends == sorted(ends) and ends[0] < ends[-1]
