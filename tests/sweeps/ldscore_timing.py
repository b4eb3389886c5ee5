"""LD scores against the only way to the same numbers without them: every record computed, sorted, copied to the host and dropped.
    python tests/sweeps/ldscore_timing.py [--out profiles/r07_ldscore_timing.json] [--reps 3]
One process, one engine context, synthetic input from the on-device generator.  Per shape, alternating after a warm-up of each:
  (a) ld_all(mode, Filters(minR2=0), collect=False): all pairs through math, Fisher, sort, PCIe and the sink (which drops them) - the
      per-variant summing a user would still have to do is NOT in the clock, so (a) is a lower bound of the old way;
  (b) ld_score(mode, Filters(minR2=0)).
Both calls return when their last byte is on the host (they synchronise the engine's streams themselves), so the wall time around
a call is device-synchronised.  Before anything is timed, at the same sample count with 4,000 variants: a summing sink over (a)'s
records and (b) must agree (n equal, sums to 2 M 2^-53 relative).  Fails without a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ctypes as C

import numpy as np

import tomahawk_amd as T
from tomahawk_amd.hip import RECORD_DTYPE, _SINK

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_ldscore_timing.json"))
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("ldscore_timing: no HIP device visible")

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("100,000 x 4,000 -u", 100_000, 4_000, T.MODE_UNPHASED, "u")]
CHECK_M = 4_000
F0 = T.Filters(minR2=0.0)


def summed_records(eng, mode, M):
    """(a) with a sink that sums instead of dropping: -> (n uint64[M], sum float64[M], records)."""
    n = np.zeros(M, dtype=np.int64)
    s = np.zeros(M, dtype=np.float64)
    total = [0]

    def sink(_user, recs, k):
        r = np.frombuffer((C.c_char * (k * RECORD_DTYPE.itemsize)).from_address(recs), dtype=RECORD_DTYPE)
        for idx in (r["idxA"], r["idxB"]):
            n[:] += np.bincount(idx, minlength=M)
            s[:] += np.bincount(idx, weights=r["R2"], minlength=M)
        total[0] += k
        return 0

    cb = _SINK(sink)
    f = F0._c()
    eng._check(eng._lib.twk_hip_ld_all(eng._ctx, mode, C.byref(f), 0, 1, 0, 0, 0, cb, None, None, None), "twk_hip_ld_all")
    return n.astype(np.uint64), s, total[0]


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return wall, {k: tm[k] for k in ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")}, out


result = {"what": "ld_score (b) against ld_all(minR2=0, collect=False) (a): wall ms per call and twk_hip_timing, one process, alternating",
          "reps": args.reps, "shapes": []}
eng = T.HipLd(0)
for name, N, M, mode, key in SHAPES:
    # agreement first, outside the clock
    eng.set_problem(N, CHECK_M)
    eng.generate_synthetic(42)
    rn, rs, nrec = summed_records(eng, mode, CHECK_M)
    sn, ss, _ = eng.ld_score(mode, F0)
    rel = float(np.max(np.abs(ss - rs) / np.maximum(rs, 1e-300)))
    assert np.array_equal(rn, sn), f"{name}: n differs between the summed records and ld_score"
    assert rel <= 2 * CHECK_M * 2.0 ** -53, f"{name}: sums differ by {rel:.3g} relative"
    print(f"{name}: check at M = {CHECK_M}: {nrec} records, n equal, largest relative difference of the sums {rel:.3g}", flush=True)

    eng.set_problem(N, M)
    eng.generate_synthetic(42)
    a = lambda: eng.ld_all(mode, F0, collect=False)
    b = lambda: eng.ld_score(mode, F0)
    a(); b()                                   # warm-up of each: plane sets, buffers, staging, clocks
    runs_a, runs_b = [], []
    for _ in range(args.reps):
        wa, ta, oa = timed(eng, a)
        wb, tb, ob = timed(eng, b)
        runs_a.append({"wall_ms": wa, **ta, "records": int(oa[2])})
        runs_b.append({"wall_ms": wb, **tb})
    pairs = M * (M - 1) // 2
    wa = [r["wall_ms"] for r in runs_a]; wb = [r["wall_ms"] for r in runs_b]
    med_b = sorted(runs_b, key=lambda r: r["wall_ms"])[len(runs_b) // 2]
    shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "pairs": pairs,
             "check": {"n_variants": CHECK_M, "records": int(nrec), "n_equal": True, "largest_relative_difference": rel},
             "a_ld_all_dropped": runs_a, "b_ld_score": runs_b,
             "a_wall_ms_min_max": [min(wa), max(wa)], "b_wall_ms_min_max": [min(wb), max(wb)],
             "ratio_of_medians": float(np.median(wa) / np.median(wb)),
             "b_faster_by_more_than_the_spread": bool(max(wb) < min(wa)),
             "b_stats_ms_le_count_ms": bool(med_b["stats_ms"] <= med_b["count_ms"]),
             "b_epilogue_pairs_per_s": pairs / (med_b["stats_ms"] * 1e-3) if med_b["stats_ms"] > 0 else None,
             "b_count_pairs_per_s": pairs / (med_b["count_ms"] * 1e-3) if med_b["count_ms"] > 0 else None}
    result["shapes"].append(shape)
    print(f"{name}: (a) {min(wa):.1f} .. {max(wa):.1f} ms, (b) {min(wb):.1f} .. {max(wb):.1f} ms, ratio of medians {shape['ratio_of_medians']:.2f}; "
          f"(b) count {med_b['count_ms']:.2f} ms, score epilogue {med_b['stats_ms']:.2f} ms in {med_b['stats_launches']} launches "
          f"({shape['b_epilogue_pairs_per_s'] / 1e9:.2f} G pairs/s)", flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("written:", args.out)
bad = [s["name"] for s in result["shapes"] if not s["b_faster_by_more_than_the_spread"]]
if bad:
    sys.exit(f"ld_score is not faster than the record path by more than the spread on: {bad}")
