"""The host side of the prefix contraction, without a GPU: `make prefix-check` - the prefix screens of
csrc/hip/ld_two_screen.h over every pair of a small prefix and a small suffix genotype table, the work table with per-tile stops
(csrc/hip/ld_count_table.h) and the planner's stops on the headline's frequency law (csrc/hip/ld_plan.h), under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_output():
    r = subprocess.run(["make", "-C", ROOT, "prefix-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "prefix-check: ok" in r.stdout
    return r.stdout


def test_prefix_screens_keep_every_pair_the_full_screen_keeps(check_output):
    """Every (prefix table, suffix table) of up to 4 + 4 samples at r2 >= 0.1, 0.5, 0.8 and at cut-offs on and next to the r2 values of the
    summed table: zero violations - and the prefix screens are wider, the two-product one the widest."""
    m = re.search(r"screens: (\d+) tables of up to 4 samples, (\d+) \(prefix table, suffix table, cut-off\) tests; three products on the whole rows keep (\d+), "
                  r"the three-product prefix screen (\d+), the two-product prefix screen (\d+); violations (\d+)", check_output)
    assert m, check_output[-2000:]
    tables, tests, k3, k3p, k2p, violations = (int(x) for x in m.groups())
    assert tables == 715 and tests > 3 * 714 * 715 and violations == 0
    assert 0 < k3 < k3p < k2p < tests


def test_table_builder_with_stops(check_output):
    """Units partition [0, stop) of every tile, split tiles lie in the zeroed range, whole-count units of stopped tiles are flagged, and
    stops at the row's end give the image of the table built without stops."""
    m = re.search(r"table builder with stops: (\d+) cases, (\d+) bad", check_output)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) == 0, check_output[-2000:]


def test_planner_on_the_headlines_law(check_output):
    """1,000,000 samples x 50,000 variants, p over (0.05, 0.5), r2 >= 0.1, margins at their expectation: ten launches, four of them in front of
    the two-product cut; every launch stops short of the rows on average, the rare rows against the common columns the most.  The count
    work: the arithmetic on expectations behind the form gives 0.78 of today's on a 32-point grid, and the planner adds one grid step
    (1 / 32 of a row) to every tile: 0.81, held here to +- 0.05 - the tile edges, the five pairs a tile is asked at and the rounding of the
    margins move it by less (profiles/prefix_contraction_ab.txt records the figure beside the measurement)."""
    launches = re.findall(r"launch +(\d+) +(two|three) +rows +(\d+)\+(\d+) +cols +(\d+)\+(\d+) +(\d+) tiles +stops +(\d+) \.\. +(\d+) chunks +contracted ([0-9.]+) of the rows", check_output)
    assert len(launches) == 10 and [x[1] for x in launches] == ["two"] * 4 + ["three"] * 6
    frac = [float(x[9]) for x in launches]
    assert all(0.2 < f < 1.0 for f in frac) and min(frac) == frac[1]
    assert all(1 <= int(x[7]) <= int(x[8]) <= 977 for x in launches)
    m = re.search(r"planner: count work ([0-9.]+) of today's", check_output)
    assert m and 0.76 < float(m.group(1)) < 0.86, check_output[-1500:]
