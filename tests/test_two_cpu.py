"""The host side of the two-product form, without a GPU: `make two-check` - the screen of csrc/hip/ld_two_screen.h over every
small genotype table and the work table of a launch with one plane row per row variant, under AddressSanitizer and UBSan - and the
planner's cut of the sorted triangle (csrc/hip/ld_plan.h plan_two_end through twk_hip_plan_region_two)."""
import os
import re
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_product_screen_and_work_table_on_the_cpu():
    """The two-product screen keeps every pair the three-product screen keeps, with the true S inside [S_lo, S_hi], over every 3 x 3 table
    of up to 7 samples at fixed cut-offs and at cut-offs on and next to the values where the three-product screen turns; the 1 : 2 work
    table lists exactly the tiles that hold a wanted pair (edges that are no tile multiples, diagonal super-tiles, a single partial tile),
    its units partition every tile's K range (K-split units included), and its order is the recorded one
    (tests/golden/count_tables_two.json)."""
    r = subprocess.run(["make", "-C", ROOT, "two-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(r"two-check: (\d+) cases, (\d+) bad; screen: (\d+) \(table, cut-off\) tests, three products kept (\d+), two (\d+)", r.stdout)
    assert m and int(m.group(1)) >= 30 and int(m.group(2)) == 0, r.stdout[-2000:]
    assert int(m.group(3)) > 100_000 and 0 < int(m.group(4)) <= int(m.group(5)) < int(m.group(3))


def _sorted_margins(M, N, seed=0, lo=0.05, hi=0.5):
    p = np.sort(np.random.default_rng(seed).uniform(lo, hi, size=M))
    het = np.round(2 * p * (1 - p) * N).astype(np.uint32)
    hom = np.round(p * p * N).astype(np.uint32)
    return p, het, hom


def _meta(M):
    m = np.zeros(M, dtype=T.META_DTYPE)
    m["pos"] = np.arange(M, dtype=np.uint32) * 100 + 1000
    m["ac"] = 5
    return m


def _plan(M, N, het, hom, minR2=0.1, margin=0.0, **kw):
    return T.plan_region(_meta(M), N, 0, M, 0, M, True, planes_per_variant=2, k_chunks=(N + 1023) // 1024, minR2=minR2, phased_math=False,
                         het=het, hom=hom, two_margin=margin, **kw)


def test_the_cut_lies_where_the_rows_hom_alt_carriers_become_too_many():
    """The headline's frequency law at N = 1,000,000: r* at p ~ 0.16 (margin 0.95), a multiple of the A tile edge; it does not fall when the
    cut-off rises or the margin grows, and a cut-off the screen cannot use (every pair kept) leaves no row in front of it."""
    M, N = 5000, 1_000_000
    p, het, hom = _sorted_margins(M, N)
    ends = [_plan(M, N, het, hom, minR2=r2)["two_end"] for r2 in (1e-5, 0.02, 0.1, 0.3, 0.8)]
    assert all(e % 128 == 0 for e in ends) and ends == sorted(ends) and ends[0] == 0 and ends[-1] > ends[2], ends
    assert 0.14 < p[ends[2]] < 0.175, (ends, p[ends[2]])
    by_margin = [_plan(M, N, het, hom, margin=m)["two_end"] for m in (0.5, 0.8, 0.95, 1.0)]
    assert by_margin == sorted(by_margin) and by_margin[0] < by_margin[-1] and 0.165 < p[by_margin[-1] + 127] and p[by_margin[-1]] < 0.18, by_margin
    # without the margins' arrays the plan is twk_hip_plan_region's
    plain = T.plan_region(_meta(M), N, 0, M, 0, M, True, planes_per_variant=2, phased_math=False)
    assert plain["two_end"] == 0
    # a common variant at the head of the order (alt frequency 0.9: few minor alleles, many hom-alt carriers) ends the rows at once
    het2, hom2 = het.copy(), hom.copy()
    het2[0], hom2[0] = round(2 * 0.9 * 0.1 * N), round(0.81 * N)
    assert _plan(M, N, het2, hom2)["two_end"] == 0


@pytest.mark.parametrize("M,n_parts", [(5000, 1), (5000, 3), (1100, 1), (1100, 4), (300, 2)])
def test_no_launch_straddles_the_cut_and_every_pair_is_visited_once(M, n_parts):
    N = 1_000_000
    p, het, hom = _sorted_margins(M, N, seed=M)
    whole = _plan(M, N, het, hom)
    end = whole["two_end"]
    assert (end > 0) == (M >= 1100)
    cov = np.zeros((M, M), dtype=np.int16)
    pairs = 0
    prev_end = 0
    for k in range(n_parts):
        pl = _plan(M, N, het, hom, part=k, n_parts=n_parts)
        assert pl["two_end"] == end                        # every rank derives the same cut
        assert pl["row_begin"] == prev_end and pl["n_band_launches"] == 0
        prev_end = pl["row_end"]
        pairs += pl["n_pairs"]
        before = 0
        for t in pl["tiles"]:
            a0, nA, b0, nB = int(t["rowA0"]), int(t["nA"]), int(t["rowB0"]), int(t["nB"])
            assert a0 + nA <= end or a0 >= end, (a0, nA, end)
            assert pl["row_begin"] <= a0 and a0 + nA <= pl["row_end"]
            before += a0 + nA <= end
            sub = np.ones((nA, nB), dtype=np.int16)
            if t["diag"]:
                assert a0 == b0 and nB >= nA
                sub = np.triu(sub, k=1)
            cov[a0:a0 + nA, b0:b0 + nB] += sub
        if pl["row_begin"] < end:
            assert before >= 1
    assert prev_end == M and pairs == M * (M - 1) // 2
    assert np.array_equal(cov, np.triu(np.ones((M, M), dtype=np.int16), k=1))
    # and the same shards without the cut cover the same rows
    for k in range(n_parts):
        a = _plan(M, N, het, hom, part=k, n_parts=n_parts)
        b = T.plan_region(_meta(M), N, 0, M, 0, M, True, part=k, n_parts=n_parts, planes_per_variant=2, phased_math=False)
        assert (a["row_begin"], a["row_end"], a["n_pairs"]) == (b["row_begin"], b["row_end"], b["n_pairs"])
