"""The fine grid of the prefix contraction's stops and the planner's question in standard deviations, without a GPU: the parts
of `make prefix-check` that csrc/tools/prefix_check.cpp gained with them, under AddressSanitizer and UBSan."""
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


def test_grid_points_and_screens_at_fine_stops(check_output):
    """prefix_stop_chunks against its naive restatement for rows of 1 .. 2,000 chunks (monotone, every coarse point present, the last point
    the row's end: a failed check fails the tool), the suffix table's walk over the unequal segments, and the prefix screens on rows cut at
    every fine stop: they are counted with the exhaustive tests, and the violations stay 0."""
    m = re.search(r"grid of stops: rows of 1 \.\. 2000 chunks against the naive restatement, (\d+) screen tests at fine stops of rows of 129, 137, 977 chunks", check_output)
    assert m and int(m.group(1)) >= 3 * 6 * 129 * 3, check_output[-2000:]
    assert re.search(r"violations 0\b", check_output)


def test_planner_at_the_four_settings(check_output):
    """The headline's law, carrier form.  The arithmetic on expectations: a tile's stop lies about 1.5 grid steps behind its need, so a grid
    four times as fine saves about 1.5 x (1 / 32 - 1 / 128) = 3.5 % of a row, of 76 % contracted: 0.955 of the work, held to +- 0.015.  Six
    standard deviations at a million samples are about half of the 5 % margin, that is about margin 0.975: the default lies within 0.01 of
    the 0.98 report and below the 0.95 one.  The stops of the default cost no more than twice the host time of the grid of 32."""
    rows = re.findall(r"fine grid: (.+?) +H-form work ([0-9.]+) of whole rows, x carrier form ([0-9.]+) = ([0-9.]+); against the first setting ([0-9.]+); stops ([0-9.]+) ms", check_output)
    assert len(rows) == 4, check_output[-3000:]
    names = [r[0] for r in rows]
    assert names[0].startswith("32 points, margin 0.95") and names[1] == "128 points, margin 0.95" and "6 sigma" in names[2] and names[3] == "128 points, margin 0.98"
    ratio = [float(r[4]) for r in rows]
    assert ratio[0] == 1.0 and 0.94 < ratio[1] < 0.97 and ratio[2] < ratio[1] and abs(ratio[2] - ratio[3]) < 0.01 and ratio[2] > 0.90
    for r in rows:
        assert abs(float(r[1]) * float(r[2]) - float(r[3])) < 2e-4
    assert float(rows[2][5]) <= 2.0 * float(rows[0][5]) + 50.0
    m = re.search(r"fine grid: prediction new / before ([0-9.]+)", check_output)
    assert m and float(m.group(1)) == ratio[2]
    frac = re.search(r"fine grid: the default's fraction of the rows contracted, walk step by walk step:((?: [0-9.]+)+)", check_output)
    assert frac and len(frac.group(1).split()) == 10 and all(0.2 < float(x) < 1.0 for x in frac.group(1).split())
