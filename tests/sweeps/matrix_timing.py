"""The LD matrix filled on the device against the only way to the same matrix without it: every record at minR2 = 0 computed, run
through Fisher's test, sorted and copied to the host, and scattered into an array there.
    python tests/sweeps/matrix_timing.py [--out profiles/r08_matrix_timing.json] [--reps 5]
One process, one engine context, synthetic input from the on-device generator with LD planted in it (prune_timing.py's: every odd
variant a noisy copy of an even one, Plant.spread).  Per shape, alternating after a warm-up of each:
  (a) ld_all(mode, Filters(minR2=0)) with the records delivered (the record path as it stands), then the numpy scatter a user would
      write - copysign(R, D) as float32 at (idxA, idxB) and (idxB, idxA), the diagonal set - both in the clock, reported separately;
  (b) ld_matrix(mode, Filters(minR2=0), stat=STAT_R, fill=0).
Both calls return when their last byte is on the host, so the wall time around a call is device-synchronised.  (a) and (b) must
return the same matrix, bit for bit, before anything is timed.  Reported for (b): the count kernels (count_ms), the fill epilogue
(stats_ms), the device-to-host copy (twk_hip_matrix_last) and the matrix's bytes against the records' bytes of (a).  Medians of
--reps runs.  Fails without a GPU."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_matrix_timing.json"))
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("matrix_timing: no HIP device visible")
assert args.reps >= 5, "medians of at least 5 runs"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("100,000 x 4,000 -u", 100_000, 4_000, T.MODE_UNPHASED, "u")]


def host_scatter(recs, M):
    """The matrix of signed r from records (idxA < idxB, each pair once), as a user's script would build it."""
    m = np.zeros((M, M), dtype=np.float32)
    x = np.copysign(recs["R"], recs["D"]).astype(np.float32)
    a, b = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64)
    m[a, b] = x
    m[b, a] = x
    np.fill_diagonal(m, 1.0)
    return m


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return wall, {k: tm[k] for k in ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")}, out


result = {"what": "ld_matrix (b) against ld_all(minR2=0) with records delivered plus the numpy scatter on the host (a): ms per call, one process, "
                  "alternating, medians over reps; planted synthetic input; signed r, fill 0", "reps": args.reps, "shapes": []}
eng = T.HipLd(0)
f = T.Filters(minR2=0.0)
for name, N, M, mode, key in SHAPES:
    eng.set_problem(N, M)
    eng.generate_synthetic(42, plant=T.Plant.spread(M))

    def a():
        recs, _, _ = eng.ld_all(mode, f)
        t0 = time.perf_counter()
        m = host_scatter(recs, M)
        return m, len(recs), (time.perf_counter() - t0) * 1e3, recs.nbytes

    def b():
        out = eng.ld_matrix(mode, f, stat=T.STAT_R, fill=0.0)
        return out, eng.matrix_last()

    (ma, n_recs, _, _), ((mb, n_records, _), _) = a(), b()          # warm-up of each, and agreement outside the clock
    assert n_records == n_recs and np.array_equal(ma.view(np.uint32), mb.view(np.uint32)), f"{name}: the two ways disagree"
    del ma, mb
    runs_a, runs_b = [], []
    for _ in range(args.reps):
        wa, ta, oa = timed(eng, a)
        runs_a.append({"wall_ms": wa, "host_scatter_ms": oa[2], **ta, "records": int(oa[1]), "record_bytes": int(oa[3])})
        del oa
        wb, tb, ob = timed(eng, b)
        runs_b.append({"wall_ms": wb, **tb, "copy_ms": ob[1]["copy_ms"], "matrix_bytes": int(ob[1]["matrix_bytes"])})
        del ob
    wa = [r["wall_ms"] for r in runs_a]; wb = [r["wall_ms"] for r in runs_b]
    shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "pairs": M * (M - 1) // 2, "records": int(n_recs), "matrices_equal": True,
             "a_records_then_host_scatter": runs_a, "b_ld_matrix": runs_b,
             "a_wall_ms_median": float(np.median(wa)), "b_wall_ms_median": float(np.median(wb)),
             "a_wall_ms_min_max": [min(wa), max(wa)], "b_wall_ms_min_max": [min(wb), max(wb)],
             "a_host_scatter_ms_median": float(np.median([r["host_scatter_ms"] for r in runs_a])),
             "a_record_bytes": runs_a[0]["record_bytes"],
             "b_count_ms_median": float(np.median([r["count_ms"] for r in runs_b])),
             "b_fill_epilogue_ms_median": float(np.median([r["stats_ms"] for r in runs_b])),
             "b_copy_ms_median": float(np.median([r["copy_ms"] for r in runs_b])),
             "b_matrix_bytes": runs_b[0]["matrix_bytes"],
             "b_wall_minus_kernels_and_copy_ms_median": float(np.median([r["wall_ms"] - r["count_ms"] - r["stats_ms"] - r["copy_ms"] for r in runs_b]))}
    result["shapes"].append(shape)
    print(f"{name}: {n_recs} records; (a) {min(wa):.1f} .. {max(wa):.1f} ms (host scatter {shape['a_host_scatter_ms_median']:.1f}, "
          f"{shape['a_record_bytes'] / 1e6:.1f} MB of records), (b) {min(wb):.1f} .. {max(wb):.1f} ms: count {shape['b_count_ms_median']:.2f}, "
          f"fill epilogue {shape['b_fill_epilogue_ms_median']:.2f}, copy {shape['b_copy_ms_median']:.2f} ms, matrix {shape['b_matrix_bytes'] / 1e6:.1f} MB", flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("written:", args.out)
