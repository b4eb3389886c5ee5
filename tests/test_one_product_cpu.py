"""The host side of the one-product launches of the carrier form, without a GPU: the extended `make two-check`, `make prefix-check`
and `make form-check` (csrc/hip/ld_two_screen.h: screen1c_*, csrc/hip/ld_plan.h: plan_one_end, plan_one_tiles, csrc/hip/ld_form.h:
LaunchForm::one) under AddressSanitizer and UBSan, and the plan through the library's entry."""
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


def test_screen_order_on_whole_rows_and_one_end_is_exact():
    """Every 3 x 3 table of up to 7 samples: kept(three) <= kept(carrier) <= kept(one), pair by pair (a failed check fails the tool) and strictly
    over all the tests.  plan_one_end on random sorted margins: every pair in front of it passes screen1c_lower_ok, the pair (row, one_end) does not."""
    out = _make("two-check")
    c = re.search(r"two-check: carrier screen kept (\d+) of the same tests \(three products (\d+) <= carrier <= H plane (\d+)\)", out)
    m = re.search(r"two-check: one-product screen kept (\d+) of the same tests \(carrier (\d+) <= one product\); one_end exact on (\d+) rows, (\d+) pairs in front of it, (\d+) bad", out)
    assert c and m, out[-2000:]
    k1, kc, rows, pairs, bad = (int(x) for x in m.groups())
    assert int(c.group(1)) == kc and 0 < int(c.group(2)) < kc < k1
    assert rows >= 100 and pairs >= 100_000 and bad == 0
    assert re.search(r"two-check: \d+ cases, 0 bad", out)


@pytest.fixture(scope="module")
def prefix_output():
    out = _make("prefix-check")
    assert "prefix-check: ok" in out
    return out


def test_screen_order_on_prefixes(prefix_output):
    """Every (prefix, suffix) table of up to 4 + 4 samples: the one-product prefix screen keeps every pair the carrier prefix screen keeps and every
    pair three products keep on the whole rows (a violation fails the tool)."""
    c = re.search(r"the two-product prefix screen on the carrier plane keeps (\d+) \(three products on the whole rows (\d+) <=", prefix_output)
    m = re.search(r"the one-product prefix screen keeps (\d+) \(the carrier plane's (\d+) <= it\)", prefix_output)
    assert c and m, prefix_output[-2000:]
    assert 0 < int(c.group(2)) < int(m.group(2)) < int(m.group(1))
    assert re.search(r"violations 0\b", prefix_output)


def test_planner_report_on_the_headlines_law(prefix_output):
    """1,000,000 samples x 50,000 variants, p over (0.05, 0.5), r2 >= 0.1: the predicted count work against the carrier form with stops, with the
    rows in front of the cut in blocks of S and of S / 2.  The arithmetic on expected counts behind the form gives 0.87 - 0.88; the planner's own
    figures are held to 0.85 .. 0.90, lower blocks never predicted worse."""
    rows = re.findall(r"one product: rows in front of the cut (\d+) in blocks of (\d+) \((S|S / 2)\): (\d+) launches, (\d+) of them one-product and (\d+) two-product in front of the cut; "
                      r"count work with stops ([0-9.]+) of the carrier form's with stops", prefix_output)
    assert [r[2] for r in rows] == ["S", "S / 2"], prefix_output[-3000:]
    (s_full, s_half) = (float(r[6]) for r in rows)
    assert 0.85 < s_half <= s_full < 0.90
    assert all(int(r[4]) >= 2 and int(r[5]) >= 2 and int(r[0]) % 128 == 0 for r in rows)
    m = re.search(r"one product: prediction new / parent ([0-9.]+)", prefix_output)
    assert m and float(m.group(1)) == s_half
    # the earlier reports stand as they were
    assert len(re.findall(r"planner: count work", prefix_output)) == 1 and len(re.findall(r"fine grid: prediction new / before", prefix_output)) == 1


def test_form_check_covers_the_one_product_attribute():
    out = _make("form-check")
    m = re.search(r"form-check: (\d+) cases, (\d+) bad", out)
    assert m and int(m.group(1)) >= 3000 and int(m.group(2)) == 0, out[-2000:]
    assert "form-check: one-product attribute: granted with the carrier form only, given up alone" in out


def test_plan_marks_the_columns_in_front_of_one_end():
    """The planner through the library's entry on the headline's law, scaled down: in front of the cut every block's one-product launches start on
    the diagonal and end at a multiple of 128 variants from it (or at the last column), at or behind the block's own end; behind them two-product
    launches to the last column; behind the cut nothing changes; and the pairs are those of the plan without the form."""
    M, N = 5000, 1_000_000
    p = 0.05 + 0.45 * (np.arange(M) + 0.5) / M
    het = np.round(2 * p * (1 - p) * N).astype(np.uint32)
    hom = np.round(p * p * N).astype(np.uint32)
    meta = np.zeros(M, dtype=T.META_DTYPE)
    meta["pos"] = np.arange(M, dtype=np.uint32) * 100 + 1000
    meta["ac"] = 5

    def plan(**kw):
        return T.plan_region(meta, N, 0, M, 0, M, True, planes_per_variant=2, k_chunks=(N + 1023) // 1024, minR2=0.1, phased_math=False, het=het, hom=hom, **kw)
    base = plan(carrier=True)
    assert not base["tiles"]["one"].any() and not plan(one=True)["tiles"]["one"].any()      # (only with the carrier form)
    d = het.astype(np.float64) + 2.0 * hom
    two_n, cut = 2.0 * N, 0.1 * (1.0 - 1e-6)

    def lower_ok(a, b):
        return (-(d[a] * d[b]) - 1e-5 * two_n * two_n) ** 2 < cut * d[a] * (two_n - d[a]) * d[b] * (two_n - d[b])
    for rows in (128, 512, 0):
        pl = plan(carrier=True, one=True, one_rows=rows)
        tiles, end = pl["tiles"], pl["two_end"]
        assert end == base["two_end"] and pl["n_pairs"] == base["n_pairs"] == M * (M - 1) // 2
        behind = [tuple(int(t[k]) for k in ("rowA0", "nA", "rowB0", "nB", "diag")) for t in tiles if int(t["rowA0"]) >= end]
        assert behind == [tuple(int(t[k]) for k in ("rowA0", "nA", "rowB0", "nB", "diag")) for t in base["tiles"] if int(t["rowA0"]) >= end]
        covered = 0
        h = rows if rows else int(tiles[0]["nA"])
        for x in range(0, end, h):
            block = [t for t in tiles if int(t["rowA0"]) == x]
            assert block and all(int(t["nA"]) == min(h, end - x) for t in block)
            ones = [t for t in block if t["one"]]
            at = x
            for t in block:      # the launches tile the columns [x, M) in order, one-product launches first
                assert int(t["rowB0"]) == at and bool(t["diag"]) == (at == x)
                at += int(t["nB"])
            assert at == M and [bool(t["one"]) for t in block] == sorted((bool(t["one"]) for t in block), reverse=True)
            covered += sum(int(t["nA"]) * int(t["nB"]) for t in block)
            if ones:
                one_end = int(ones[-1]["rowB0"]) + int(ones[-1]["nB"])
                last = x + int(block[0]["nA"]) - 1
                assert one_end >= last + 1 and ((one_end - x) % 128 == 0 or one_end == M)
                assert lower_ok(last, one_end - 1) and lower_ok(x, x + 1)
                if one_end < M:      # the exact boundary lies within the next 128 columns
                    assert not all(lower_ok(last, c) for c in range(one_end, min(M, one_end + 128)))
        assert any(t["one"] for t in tiles)
