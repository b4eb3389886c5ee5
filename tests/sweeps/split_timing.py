"""LD splitting: where the time of ld_split goes, against the only other route to the same numbers - the banded r2 matrix copied to
the host and the dynamic programme in NumPy.
    python tests/sweeps/split_timing.py [--out profiles/split_timing.json] [--reps 5] [--window 50000] [--shapes 0,1,2]
One process, one engine context.  Synthetic input from the on-device generator with LD planted in it (bandmat_timing.py's shapes and
input: positions 1000 + 100 v on one contig, so the default window of 50,000 bases is +-500 variants) and one block-structured set from
the host (tests/util.py's mosaic of founder haplotypes, 250 samples x 4,000 variants, the same positions).  Blocks of 50 .. 500
variants, K up to 200.  Per shape, alternating after a warm-up of each:
  (a) ld_split(mode, Filters(minR2=0), W, 50, 500, 200): wall, the count kernels, the band's epilogue, and the stages of
      twk_hip_split_last - the band's launches, row prefixes + block sums, the layers, the backtrack - with the device memory held;
  (b) ld_matrix_band(mode, Filters(minR2=0), W, stat=STAT_R2, fill=0) to the host, then split_of_band below: the contract restated over
      the band with NumPy operations along b (a dense restatement as tests/split_cases.py's does not fit at these sizes; the two are
      compared on a slice of 600 variants first).
(a) and (b) must agree exactly in every run.  Medians of --reps runs; nothing is fixed in advance.  Fails without a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

import tomahawk_amd as T
from tests import split_cases as SC

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--window", type=int, default=50_000)
ap.add_argument("--shapes", default="0,1,2")
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("split_timing: no HIP device visible")
assert args.reps >= 5, "medians of at least 5 runs"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("mosaic 250 x 4,000 -p", 250, 4_000, T.MODE_PHASED, "p")]
MIN_SIZE, MAX_SIZE, K_MAX = 50, 500, 200
KEYS = ("count_ms", "stats_ms", "count_launches", "stats_launches", "variant_pairs")


def split_of_band(values, first, indptr, min_size, max_size, k_max):
    """The contract of twk_hip_ld_split over a band, in int64 NumPy operations along b -> SC.split_of's dictionary."""
    n = len(first)
    ptr, first = indptr.astype(np.int64), first.astype(np.int64)
    upper = first + (ptr[1:] - ptr[:-1]) - 1 - np.arange(n)
    J = max(1, int(min(upper.max(), max_size - 1)))
    Q = np.zeros((n, J), dtype=np.int64)
    total = 0
    for u in range(n):
        up = np.rint(values[ptr[u] + (u - first[u]) + 1:ptr[u + 1]].astype(np.float64) * SC.SCALE).astype(np.int64)
        total += int(up.sum())
        Q[u, :min(J, len(up))] = up[:J]
    R = np.cumsum(Q, axis=1)                        # R[u, j - 1] = Rp[u][j]; beyond the band the prefix stays (zeros were added)
    del Q
    W = np.zeros((max_size + 1, n + 1), dtype=np.int64)      # W[d, b] = within(b - d, b) for d <= b
    for d in range(2, max_size + 1):
        if d > n:
            break
        W[d, d:] = W[d - 1, d:] + R[:n + 1 - d, min(d - 1, J) - 1]
    G = np.full(n + 1, SC.INFEASIBLE, dtype=np.int64)
    G[0] = 0
    D = np.zeros((k_max + 1, n + 1), dtype=np.uint16)
    gain = np.full(k_max + 1, SC.INFEASIBLE, dtype=np.int64)
    for k in range(1, k_max + 1):
        best = np.full(n + 1, SC.INFEASIBLE, dtype=np.int64)
        lo, hi = k * min_size, min(n, k * max_size)
        for d in range(min_size, min(max_size, hi) + 1):          # ascending d and a strict >: the smallest d of a maximum stays
            b0 = max(lo, d)
            if b0 > hi:
                continue
            prev = G[b0 - d:hi + 1 - d]
            cand = np.where(prev >= 0, prev + W[d, b0:hi + 1], SC.INFEASIBLE)
            better = cand > best[b0:hi + 1]
            best[b0:hi + 1][better] = cand[better]
            D[k, b0:hi + 1][better] = d
        G = best
        gain[k] = G[n]
    feasible = (gain[1:] >= 0).astype(np.uint8)
    cost = np.where(gain[1:] >= 0, total - gain[1:], 0).astype(np.uint64)
    cuts, ks = [], []
    for K in range(1, k_max + 1):
        if not feasible[K - 1]:
            continue
        c, b = [n], n
        for k in range(K, 0, -1):
            b -= int(D[k, b])
            c.append(b)
        assert b == 0
        cuts.append(np.array(c[::-1], dtype=np.uint32))
        ks.append(K)
    return {"total": total, "feasible": feasible, "cost": cost, "cuts": cuts, "K": ks}


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return {"wall_ms": wall, **{k: tm[k] for k in KEYS}}, out


def medians(runs):
    return {k + "_median": float(np.median([r[k] for r in runs])) for k in runs[0] if k.endswith("_ms")}


def zero_infeasible(got):
    got["cost"][got["feasible"] == 0] = 0
    return got


W = args.window
result = {"what": "ld_split (a) against ld_matrix_band to the host + the NumPy restatement (b) on the same context: ms per call, one process, "
                  "alternating, medians over reps; blocks of 50 .. 500 variants, K up to 200", "reps": args.reps, "window_bases": W,
          "min_size": MIN_SIZE, "max_size": MAX_SIZE, "k_max": K_MAX, "shapes": []}
eng = T.HipLd(0)
f = T.Filters(minR2=0.0)
for k in (int(x) for x in args.shapes.split(",")):
    name, N, M, mode, key = SHAPES[k]
    if name.startswith("mosaic"):
        from oracle import oracle as O
        from tests import util
        al = util.mosaic_alleles(M, N, 5004, n_founders=7, switch=0.02, mut=0.002)
        util.upload(eng, al, O.variants_from_alleles(al, pos=(1000 + 100 * np.arange(M)).astype(np.uint32)))
        del al
    else:
        eng.set_problem(N, M)
        eng.generate_synthetic(42, plant=T.Plant.spread(M))
    # the two restatements on a slice, before anything is timed
    v, fi, ip, _, _ = eng.ld_matrix_band(mode, f, W, stat=T.STAT_R2, fill=0.0, a0=0, n=600)
    SC.assert_same(split_of_band(v, fi, ip, 20, 130, 12), SC.split_of(v, fi, ip, 20, 130, 12), "the sweep's restatement against the tests'")

    def route_a():
        return zero_infeasible(eng.ld_split(mode, f, W, MIN_SIZE, MAX_SIZE, K_MAX))

    def route_b():
        t0 = time.perf_counter()
        values, first, indptr, _, _ = eng.ld_matrix_band(mode, f, W, stat=T.STAT_R2, fill=0.0)
        t1 = time.perf_counter()
        out = split_of_band(values, first, indptr, MIN_SIZE, MAX_SIZE, K_MAX)
        out["band_ms"], out["numpy_ms"], out["nnz"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, int(indptr[-1])
        return out

    calls = {"a_ld_split": route_a, "b_band_numpy": route_b}
    warm = {tag: call() for tag, call in calls.items()}
    SC.assert_same(warm["a_ld_split"], warm["b_band_numpy"], name)
    shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "nnz": warm["b_band_numpy"]["nnz"], "feasible_K": [warm["a_ld_split"]["K"][0], warm["a_ld_split"]["K"][-1]],
             "total": warm["a_ld_split"]["total"] / SC.SCALE, "cost_first_K": int(warm["a_ld_split"]["cost"][warm["a_ld_split"]["K"][0] - 1]) / SC.SCALE,
             "cost_last_K": int(warm["a_ld_split"]["cost"][warm["a_ld_split"]["K"][-1] - 1]) / SC.SCALE}
    print(f"{name}: warm, the routes agree; feasible K {shape['feasible_K']}", flush=True)
    runs = {tag: [] for tag in calls}
    for rep in range(args.reps):
        for tag, call in calls.items():
            r, out = timed(eng, call)
            if tag == "a_ld_split":
                last = eng.split_last()
                r.update({"band_stage_ms": last["band_ms"], "sums_ms": last["sums_ms"], "layers_ms": last["layers_ms"], "backtrack_ms": last["backtrack_ms"]})
                shape["device_bytes"] = int(last["bytes"])
                kept = out
            else:
                r.update({"band_to_host_ms": out["band_ms"], "numpy_ms": out["numpy_ms"]})
                SC.assert_same(kept, out, f"{name} rep {rep}")
            runs[tag].append(r)
            print(f"  rep {rep} {tag}: wall {r['wall_ms']:.1f} ms", flush=True)
    for tag in calls:
        shape[tag] = {"runs": runs[tag], **medians(runs[tag])}
    result["shapes"].append(shape)
    a, b = shape["a_ld_split"], shape["b_band_numpy"]
    print(f"{name}: window +-{W} bases, nnz {shape['nnz']}; (a) ld_split wall {a['wall_ms_median']:.1f} ms: count {a['count_ms_median']:.2f}, band epilogue {a['stats_ms_median']:.2f}, "
          f"band stage {a['band_stage_ms_median']:.2f}, prefixes + sums {a['sums_ms_median']:.2f}, layers {a['layers_ms_median']:.2f}, backtrack {a['backtrack_ms_median']:.3f} ms, "
          f"{shape['device_bytes'] / 1e6:.1f} MB held; (b) band to host {b['band_to_host_ms_median']:.1f} + NumPy {b['numpy_ms_median']:.0f} ms = wall {b['wall_ms_median']:.0f} ms", flush=True)
    with open(args.out, "w") as fh:          # (after every shape: what ran is kept)
        json.dump(result, fh, indent=1)
eng.close()
print("written:", args.out)
