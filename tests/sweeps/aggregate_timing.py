"""The LD aggregate binned on the device against (a) what a user does without it - every record at minR2 = 0 computed, run through
Fisher's test, sorted and copied to the host, and binned there in both orientations - and (b) ld_decay on the same context, which runs
the same pair math per pair and has the one-dimensional form of the same epilogue: the yardstick for what the second dimension, the
four extra reductions and the 64-byte cells cost.
    python tests/sweeps/aggregate_timing.py [--out profiles/r10_ldaggregate_timing.json] [--reps 5] [--reps-a 3]
One process, one engine context, synthetic input from the on-device generator with LD planted in it (decay_timing.py's shapes and
input); 1000 x 1000 bins over the variants' span, monotone in file order (the generator's positions are 100 bases apart on one contig,
so this is `tomahawk ldaggregate`'s landscape), statistic r2.  Per shape, alternating after a warm-up of each:
  (a) ld_all(mode, Filters(minR2=0)) with the records delivered, then the numpy binning a user would write (bincount over both
      orientations, counts and R2 as weights: the mean heat map; sum_sq and the extremes are left out, to (a)'s advantage) - both in the clock, reported separately;
  (b) ld_decay(mode, Filters(minR2=0), range, 1000 bins);
  (c) ld_aggregate(mode, Filters(minR2=0), bin_x, bin_y, 1000, 1000, STAT_R2).
On the first shape (c) also runs at two extremes: 5 x 5 bins - every adder of the device on 25 cells - and the 1000 x 1000 bins
permuted over the variants - nearly every contribution outside the blocks' LDS windows, straight to global atomics.
Every call returns when its last byte is on the host, so the wall time around a call is device-synchronised; count_ms and stats_ms
are the engine's own device events around the count kernels and the epilogue (twk_hip_timing).  Before anything is timed (c) must
equal (a)'s records binned in integers, bit for bit, in all five arrays (tests/test_gpu_aggregate.py: the same check).  Medians of the
runs.  Fails without a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

import tomahawk_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_ldaggregate_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--reps-a", type=int, default=3)
ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes (debug)")
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("aggregate_timing: no HIP device visible")
assert args.reps >= 5 and args.reps_a >= 3, "medians of at least 5 runs ((a): 3)"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("100,000 x 4,000 -u", 100_000, 4_000, T.MODE_UNPHASED, "u")]
BINS = 1000
KEYS = ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")


def cells_of(recs, bx, by, Y):
    ia, ib = recs["idxA"], recs["idxB"]
    return np.concatenate([bx[ia] * Y + by[ib], bx[ib] * Y + by[ia]])


def host_bins(recs, bx, by, X, Y):
    """The heat map of mean r2 from records as a user's script would build it -> (n, sum)."""
    cell = cells_of(recs, bx, by, Y)
    return np.bincount(cell, minlength=X * Y), np.bincount(cell, weights=np.concatenate([recs["R2"], recs["R2"]]), minlength=X * Y)


def exact_sum(cell, q, cells):
    """Sums of the non-negative integers q (<= 2^33) per cell, exactly: the bits from 16 up and the 16 bits below, each summed by bincount
    in float64 - below 2^17 a contribution and fewer than 2^31 contributions, so every partial sum is an integer below 2^53 - put
    together in Python integers."""
    parts = [np.bincount(cell, weights=(q >> np.uint64(16)).astype(np.float64), minlength=cells),
             np.bincount(cell, weights=(q & np.uint64(0xFFFF)).astype(np.float64), minlength=cells)]
    out = np.zeros(cells, dtype=np.float64)
    for c in np.nonzero(parts[0] + parts[1])[0]:
        out[c] = float((int(parts[0][c]) << 16) + int(parts[1][c])) / 2 ** 32
    return out


def exact_bins(recs, bx, by, X, Y):
    """The same in the engine's integers -> the five arrays (r2 >= 0: q is not negative)."""
    cell = cells_of(recs, bx, by, Y)
    v = recs["R2"].astype(np.float64)
    q1 = np.rint(v * 4294967296.0).astype(np.uint64)
    q2 = np.rint((v * v) * 4294967296.0).astype(np.uint64)
    q, qq = np.concatenate([q1, q1]), np.concatenate([q2, q2])
    n = np.bincount(cell, minlength=X * Y).astype(np.uint64)
    lo, hi = np.full(X * Y, np.iinfo(np.uint64).max, dtype=np.uint64), np.zeros(X * Y, dtype=np.uint64)
    np.minimum.at(lo, cell, q); np.maximum.at(hi, cell, q)
    lo[n == 0] = 0
    return n, exact_sum(cell, q, X * Y), exact_sum(cell, qq, X * Y), lo.astype(np.float64) / 2 ** 32, hi.astype(np.float64) / 2 ** 32


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return wall, {k: tm[k] for k in KEYS}, out


def med(runs, key):
    return float(np.median([r[key] for r in runs]))


result = {"what": "ld_aggregate (c) against ld_all(minR2=0) with records delivered plus the numpy binning on the host (a) and against ld_decay on the "
                  "same context (b): ms per call, one process, alternating, medians over reps; planted synthetic input, positions 100 bases apart, "
                  "1000 x 1000 bins over the variants' span, statistic r2", "reps": args.reps, "reps_a": args.reps_a, "bins": BINS, "shapes": []}
eng = T.HipLd(0)
f = T.Filters(minR2=0.0)
for k, (name, N, M, mode, key) in enumerate(SHAPES):
    if str(k) not in args.shapes.split(","):
        continue
    eng.set_problem(N, M)
    eng.generate_synthetic(42, plant=T.Plant.spread(M))
    range_bp = 100 * M
    bx = (np.arange(M, dtype=np.int64) * BINS // M)          # pos = 1000 + 100 v on one contig: coord // ceil(range / bins)
    by = bx.copy()
    perm = np.random.default_rng(5).permutation(M)
    layouts = {"5x5": ((np.arange(M, dtype=np.int64) * 5 // M), (np.arange(M, dtype=np.int64) * 5 // M), 5, 5),
               "1000x1000_permuted": (bx[perm], by[np.random.default_rng(6).permutation(M)], BINS, BINS)} if k == 0 else {}

    def a():
        recs, _, _ = eng.ld_all(mode, f)
        t0 = time.perf_counter()
        out = host_bins(recs, bx, by, BINS, BINS)
        return out, len(recs), (time.perf_counter() - t0) * 1e3, recs.nbytes

    def b():
        return eng.ld_decay(mode, f, range_bp, BINS)

    def c(lay=None):
        x, y, X, Y = layouts[lay] if lay else (bx, by, BINS, BINS)
        return eng.ld_aggregate(mode, f, x.astype(np.uint16), y.astype(np.uint16), X, Y, T.STAT_R2)

    # warm-up of each, and agreement outside the clock
    recs, _, _ = eng.ld_all(mode, f)
    n_recs = len(recs)
    want = {None: exact_bins(recs, bx, by, BINS, BINS)}
    for lay, (x, y, X, Y) in layouts.items():
        want[lay] = exact_bins(recs, x, y, X, Y)
    hn, hs = host_bins(recs, bx, by, BINS, BINS)
    del recs
    b()
    for lay, w in want.items():
        got = c(lay)
        for what, g, e in zip(("n", "sum", "sum_sq", "min", "max"), got[:5], w):
            assert g.reshape(-1).tobytes() == e.tobytes(), f"{name} {lay or '1000x1000'}: {what} differs from the own records binned in integers"
    got = c()
    cn = got[0].reshape(-1)
    # ... and the floating-point bins within the quantisation, 2^-33 a contribution, plus the rounding of a float64 sum of n terms
    assert np.array_equal(cn, hn) and (np.abs(got[1].reshape(-1) - hs) <= cn * 2.0 ** -33 + cn * 2.0 ** -53 * hs).all(), f"{name}: differs from the host's floating-point bins"
    del want
    print(f"{name}: {n_recs} records; ld_aggregate equals them binned in integers, bit for bit", flush=True)
    runs_a, runs_b, runs_c, runs_x = [], [], [], {lay: [] for lay in layouts}
    for rep in range(args.reps):
        if rep < args.reps_a:
            wa, ta, oa = timed(eng, a)
            runs_a.append({"wall_ms": wa, "host_binning_ms": oa[2], **ta, "records": int(oa[1]), "record_bytes": int(oa[3])})
            del oa
        wb, tb, _ = timed(eng, b)
        runs_b.append({"wall_ms": wb, **tb})
        wc, tc, _ = timed(eng, c)
        runs_c.append({"wall_ms": wc, **tc})
        for lay in layouts:
            wx, tx, _ = timed(eng, lambda: c(lay))
            runs_x[lay].append({"wall_ms": wx, **tx})
        print(f"{name}: repetition {rep + 1} of {args.reps}", flush=True)
    shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "pairs": M * (M - 1) // 2, "records": int(n_recs),
             "cells_populated": int((cn > 0).sum()), "aggregate_equals_own_records_bit_for_bit": True,
             "a_records_then_host_binning": runs_a, "b_ld_decay": runs_b, "c_ld_aggregate": runs_c,
             "a_wall_ms_median": med(runs_a, "wall_ms"), "a_host_binning_ms_median": med(runs_a, "host_binning_ms"), "a_record_bytes": runs_a[0]["record_bytes"],
             "b_wall_ms_median": med(runs_b, "wall_ms"), "b_count_ms_median": med(runs_b, "count_ms"), "b_epilogue_ms_median": med(runs_b, "stats_ms"),
             "c_wall_ms_median": med(runs_c, "wall_ms"), "c_count_ms_median": med(runs_c, "count_ms"), "c_epilogue_ms_median": med(runs_c, "stats_ms"),
             "c_wall_ms_min_max": [min(r["wall_ms"] for r in runs_c), max(r["wall_ms"] for r in runs_c)],
             "b_wall_ms_min_max": [min(r["wall_ms"] for r in runs_b), max(r["wall_ms"] for r in runs_b)]}
    shape["a_over_c_wall"] = shape["a_wall_ms_median"] / shape["c_wall_ms_median"]
    shape["c_over_b_epilogue"] = shape["c_epilogue_ms_median"] / shape["b_epilogue_ms_median"]
    shape["c_over_b_wall"] = shape["c_wall_ms_median"] / shape["b_wall_ms_median"]
    for lay in layouts:
        shape[f"c_{lay}"] = {"runs": runs_x[lay], "wall_ms_median": med(runs_x[lay], "wall_ms"), "epilogue_ms_median": med(runs_x[lay], "stats_ms")}
    result["shapes"].append(shape)
    print(f"{name}: {n_recs} records, {shape['cells_populated']} cells populated; (a) {shape['a_wall_ms_median']:.1f} ms (host binning "
          f"{shape['a_host_binning_ms_median']:.1f}, {shape['a_record_bytes'] / 1e6:.1f} MB of records); (b) decay {shape['b_wall_ms_median']:.2f} ms: count "
          f"{shape['b_count_ms_median']:.2f}, epilogue {shape['b_epilogue_ms_median']:.2f}; (c) aggregate {shape['c_wall_ms_median']:.2f} ms: count "
          f"{shape['c_count_ms_median']:.2f}, epilogue {shape['c_epilogue_ms_median']:.2f}; a / c {shape['a_over_c_wall']:.1f}, c / b wall "
          f"{shape['c_over_b_wall']:.3f}, epilogue c / b {shape['c_over_b_epilogue']:.3f}"
          + "".join(f"; {lay}: {shape[f'c_{lay}']['wall_ms_median']:.2f} ms, epilogue {shape[f'c_{lay}']['epilogue_ms_median']:.2f}" for lay in layouts), flush=True)
    # (written after every shape: a run cut short keeps what it measured)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
eng.close()
print("written:", args.out)
