"""The banded LD matrix against the dense one at the same window: what the band buys (bytes held and copied) and what it costs or
saves in the fill epilogue.
    python tests/sweeps/bandmat_timing.py [--out profiles/bandmat_timing.json] [--reps 5] [--window 50000]
One process, one engine context, synthetic input from the on-device generator with LD planted in it (matrix_timing.py's shapes and
input: positions 1000 + 100 v on one contig, so the default window of 50,000 bases is +-500 variants).  Per shape, alternating after
a warm-up of each:
  (a) ld_matrix(mode, Filters(minR2=0), stat=STAT_R, fill=0, window=OPT_WINDOW, l_window=W): n * n floats held and copied;
  (b) ld_matrix_band(mode, Filters(minR2=0), W, stat=STAT_R, fill=0): indptr[n] floats held and copied.
Both calls return when their last byte is on the host.  (b) must equal (a) at every slot it stores, bit for bit, and (a) must be the
fill outside the band, before anything is timed.  Reported for both: the count kernels (count_ms), the fill epilogue (stats_ms: for
the band the dead blocks return early, but every row reads its BandRow and every block its columns'), the device-to-host copy
(twk_hip_matrix_last / twk_hip_bandmat_last) and the bytes.  The ratio of the bytes is nnz / n^2 by construction; nothing else is
fixed in advance.  Medians of --reps runs.  Fails without a GPU."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bandmat_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--window", type=int, default=50_000)
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("bandmat_timing: no HIP device visible")
assert args.reps >= 5, "medians of at least 5 runs"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("100,000 x 4,000 -u", 100_000, 4_000, T.MODE_UNPHASED, "u")]
KEYS = ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return wall, {k: tm[k] for k in KEYS}, out


def median(runs, key):
    return float(np.median([r[key] for r in runs]))


W = args.window
result = {"what": "ld_matrix_band (b) against ld_matrix (a) at the same window: ms per call, one process, alternating, medians over reps; "
                  "planted synthetic input; signed r, fill 0", "reps": args.reps, "window_bases": W, "shapes": []}
eng = T.HipLd(0)
f = T.Filters(minR2=0.0)
for name, N, M, mode, key in SHAPES:
    eng.set_problem(N, M)
    eng.generate_synthetic(42, plant=T.Plant.spread(M))

    def a():
        out = eng.ld_matrix(mode, f, stat=T.STAT_R, fill=0.0, window=T.OPT_WINDOW, l_window=W)
        return out, eng.matrix_last()

    def b():
        out = eng.ld_matrix_band(mode, f, W, stat=T.STAT_R, fill=0.0)
        return out, eng.bandmat_last()

    ((dense, nrec_a, _), _), ((values, first, indptr, nrec_b, _), _) = a(), b()          # warm-up of each, and agreement outside the clock
    data, indices, ptr = T.band_to_csr(values, first, indptr)
    rows = np.repeat(np.arange(M, dtype=np.int64), np.diff(ptr))
    # (equal inside the band, and as many non-zero words in all as the band holds: with a fill of 0 nothing outside the band has a value)
    assert nrec_a == nrec_b and np.array_equal(dense.view(np.uint32)[rows, indices], values.view(np.uint32)) \
        and np.count_nonzero(dense.view(np.uint32)) == np.count_nonzero(values.view(np.uint32)), f"{name}: the two ways disagree"
    nnz = int(indptr[-1])
    del dense, values, rows, indices, data
    runs_a, runs_b = [], []
    for _ in range(args.reps):
        wa, ta, oa = timed(eng, a)
        runs_a.append({"wall_ms": wa, **ta, "copy_ms": oa[1]["copy_ms"], "bytes": int(oa[1]["matrix_bytes"])})
        del oa
        wb, tb, ob = timed(eng, b)
        runs_b.append({"wall_ms": wb, **tb, "copy_ms": ob[1]["copy_ms"], "bytes": int(ob[1]["band_bytes"])})
        del ob
    shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "records": int(nrec_a), "nnz": nnz, "nnz_over_n2": nnz / (M * M), "band_equals_dense": True,
             "a_ld_matrix": runs_a, "b_ld_matrix_band": runs_b}
    for tag, runs in (("a", runs_a), ("b", runs_b)):
        shape.update({f"{tag}_wall_ms_median": median(runs, "wall_ms"), f"{tag}_wall_ms_min_max": [min(r["wall_ms"] for r in runs), max(r["wall_ms"] for r in runs)],
                      f"{tag}_count_ms_median": median(runs, "count_ms"), f"{tag}_fill_epilogue_ms_median": median(runs, "stats_ms"),
                      f"{tag}_copy_ms_median": median(runs, "copy_ms"), f"{tag}_bytes": runs[0]["bytes"]})
    result["shapes"].append(shape)
    print(f"{name}: window +-{W} bases, {nrec_a} records, nnz / n^2 = {shape['nnz_over_n2']:.4f}; "
          f"(a) dense wall {shape['a_wall_ms_median']:.1f} ms: count {shape['a_count_ms_median']:.2f}, fill epilogue {shape['a_fill_epilogue_ms_median']:.2f}, "
          f"copy {shape['a_copy_ms_median']:.2f} ms, {shape['a_bytes'] / 1e6:.1f} MB; "
          f"(b) band wall {shape['b_wall_ms_median']:.1f} ms: count {shape['b_count_ms_median']:.2f}, fill epilogue {shape['b_fill_epilogue_ms_median']:.2f}, "
          f"copy {shape['b_copy_ms_median']:.2f} ms, {shape['b_bytes'] / 1e6:.1f} MB", flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("written:", args.out)
