"""The host side of the fine walk (option "walk_fine"), without a GPU: the extended `make two-check` and `make prefix-check`
(csrc/hip/ld_two_screen.h: screen2c_slack_cq, csrc/hip/ld_plan.h: PlanEnv::fine, plan_one_tiles, plan_two_stairs) under AddressSanitizer and
UBSan, and the plan through the library's entry."""
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


@pytest.fixture(scope="module")
def prefix_output():
    out = _make("prefix-check")
    assert "prefix-check: ok" in out
    return out


def test_the_fine_carrier_screen_lies_between_three_products_and_the_carrier_screen():
    """Every 3 x 3 table of up to 7 samples: kept(three) <= kept(carrier, QQ <= min(qA, qB, CQ)) <= kept(carrier), pair by pair (a failed check
    fails the tool), and strictly fewer than the carrier screen over all the tests."""
    out = _make("two-check")
    m = re.search(r"two-check: fine carrier screen \(QQ <= min\(qA, qB, CQ\)\) kept (\d+) of the same tests \(three products (\d+) <= fine carrier <= carrier (\d+)\), pair by pair", out)
    assert m, out[-2000:]
    fine, three, carrier = (int(x) for x in m.groups())
    assert 0 < three <= fine < carrier
    assert re.search(r"two-check: \d+ cases, 0 bad", out)


def test_the_fine_carrier_prefix_screen(prefix_output):
    """Every (prefix, suffix) table of up to 4 + 4 samples, and the screens at every fine stop of rows of 129, 137 and 977 chunks."""
    m = re.search(r"the fine carrier prefix screen \(QQ_pre <= min\(qa_pre, qb_pre, CQ_pre\)\) keeps (\d+) \(three products on the whole rows (\d+) <= it <= the carrier plane's (\d+)\), pair by pair", prefix_output)
    assert m, prefix_output[-2000:]
    fine, three, carrier = (int(x) for x in m.groups())
    assert 0 < three <= fine < carrier
    assert re.search(r"violations 0\b", prefix_output)


def test_planner_report_of_the_fine_walk_on_the_headlines_law(prefix_output):
    """walk_fine 0 is the parent's plan; walk_fine 1 moves no cut, adds the two-product launches behind it and predicts less count work at every
    sigma, less at a smaller one.  The model of expected counts behind the change puts all of it at 0.957 of the parent's count work."""
    rows = re.findall(r"walk fine: (walk_fine \d, [0-9.]+ sigma)[^\n]*?two_end (\d+) \(p = [0-9.]+\), two_last (\d+) \(p = [0-9.]+\); (\d+) launches: (\d+) one-product, (\d+) two-product, (\d+) three-product; "
                      r"count work ([0-9.]+) of whole rows in these forms, ([0-9.]+) of the parent's; a step ([0-9.]+) of the parent's", prefix_output)
    assert [r[0] for r in rows] == ["walk_fine 0, 6 sigma", "walk_fine 1, 6 sigma", "walk_fine 1, 5 sigma", "walk_fine 1, 4.5 sigma"], prefix_output[-3000:]
    parent, fine = rows[0], rows[1:]
    assert parent[1] == parent[2] and float(parent[8]) == 1.0 and float(parent[9]) == 1.0
    for r in fine:
        assert int(r[1]) >= int(parent[1]) and int(r[2]) > int(r[1]) and int(r[2]) % 128 == 0
        assert int(r[5]) > int(parent[5]) and int(r[4]) == int(parent[4])
        assert float(r[8]) < float(r[9]) < 1.0
    work = [float(r[8]) for r in fine]
    assert work[0] >= work[1] >= work[2] and 0.93 < work[2] and work[0] < 0.975


def test_the_plan_covers_every_pair_once(prefix_output):
    """Random het / hom tables of 300 .. 3,000 variants: every pair in exactly one launch's tiles and on its side of the staircase, staircases
    that never rise, walk_fine 0 the parent's tile lists (a failed check fails the tool)."""
    m = re.search(r"walk fine: plan cover: (\d+) plans, (\d+) pairs each in exactly one launch and on its side of the staircase; (\d+) launches with a side, (\d+) two-product launches behind the cut, (\d+) "
                  r"steps of a staircase; walk_fine 0 equals the parent's launches in (\d+) plans", prefix_output)
    assert m, prefix_output[-2000:]
    plans, pairs, sides, behind, steps, equal = (int(x) for x in m.groups())
    assert plans >= 50 and equal == plans and pairs > 10_000_000 and sides >= 100 and behind >= 20 and steps >= 20


def test_the_plan_through_the_library():
    """The headline's law scaled down: without the fine walk the entry gives the plan of twk_hip_plan_region_two_form; with it, launches with a side
    only over rows that have a border, one-product launches in front of the borders, and the two-product launches behind the cut between two_end
    and two_last."""
    M, N = 5000, 1_000_000
    p = 0.05 + 0.45 * (np.arange(M) + 0.5) / M
    het = np.round(2 * p * (1 - p) * N).astype(np.uint32)
    hom = np.round(p * p * N).astype(np.uint32)
    meta = np.zeros(M, dtype=T.META_DTYPE)
    meta["pos"] = np.arange(M, dtype=np.uint32) * 100 + 1000
    meta["ac"] = 5

    def plan(**kw):
        return T.plan_region(meta, N, 0, M, 0, M, True, planes_per_variant=2, k_chunks=(N + 1023) // 1024, minR2=0.1, phased_math=False, het=het, hom=hom, carrier=True, one=True, **kw)
    for rows in (512, 0):
        base, fine = plan(one_rows=rows), plan(one_rows=rows, walk_fine=True)
        assert not base["side"].any() and not base["behind"].any() and not base["stair"].any() and base["two_last"] == base["two_end"]
        assert fine["n_pairs"] == base["n_pairs"] == M * (M - 1) // 2
        assert base["two_end"] <= fine["two_end"] < fine["two_last"] < M
        tiles, side, behind, stair = fine["tiles"], fine["side"], fine["behind"], fine["stair"]
        assert (side == 1).sum() >= 2 and (side == 2).sum() >= 2 and behind.sum() >= 1
        decided = 0
        for t, s, b in zip(tiles, side, behind):
            a0, nA, b0, nB = (int(t[k]) for k in ("rowA0", "nA", "rowB0", "nB"))
            rows_ = np.arange(a0, a0 + nA)
            lo = np.full(nA, b0); hi = np.full(nA, b0 + nB)
            if t["diag"]:
                lo = np.maximum(lo, rows_ + 1)
            if s:
                st = stair[a0:a0 + nA].astype(np.int64)
                assert st.all() and (np.diff(st) <= 0).all() and (((st - a0) % 128 == 0) | (st == M)).all()
            if s == 1:
                hi = np.minimum(hi, stair[a0:a0 + nA])
            if s == 2:
                lo = np.maximum(lo, stair[a0:a0 + nA])
            decided += int(np.maximum(hi - lo, 0).sum())
            if b:
                assert s == 1 and t["diag"] and not t["one"] and fine["two_end"] <= a0 and a0 + nA <= fine["two_last"]
            if t["one"]:
                assert a0 + nA <= fine["two_end"]
        assert decided == M * (M - 1) // 2
