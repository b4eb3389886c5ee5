"""LD clumping on the device against the only way to the same clumps without it: the records at the cut-off computed, sorted, copied
to the host, and the walk in P order done over them there.
    python tests/sweeps/clump_timing.py [--out profiles/r08_clump_timing.json] [--reps 5]
One process, one engine context, synthetic input from the on-device generator with LD planted in it (prune_timing.py's: every odd
variant a noisy copy of an even one, Plant.spread: M / 2 pairs whose r2 spans the cut-offs).  P values: the tests' standard recipe,
10 ** (-8 * default_rng(77).random(M)).  Per shape, cut-off and pair of thresholds - (1e-4, 1e-2), and (1, 1): the most index
variants the walk can see - alternating after a warm-up of each:
  (a) ld_all(mode, Filters(minR2=thr)) with the records delivered (the record path as it stands, its screens included), then the
      clump over them in numpy / Python on the host - both in the clock, reported separately;
  (b) ld_clump(mode, Filters(minR2=thr), p, p1, p2).
Both calls return when their last byte is on the host, so the wall time around a call is device-synchronised.  (a) and (b) must
return the same index_of, edge for record, before anything is timed.  Reported for (b): the count kernels (count_ms), the mask
epilogue (stats_ms), the walk kernel (twk_hip_clump_last), the walk time per index variant and the bitmap's bytes.  Medians of
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_clump_timing.json"))
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("clump_timing: no HIP device visible")
assert args.reps >= 5, "medians of at least 5 runs"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("100,000 x 4,000 -u", 100_000, 4_000, T.MODE_UNPHASED, "u")]
CUTS = (0.2, 0.8)
THRESHOLDS = ((1e-4, 1e-2), (1.0, 1.0))
NO = T.NO_CLUMP


def host_clump(recs, M, p, p1, p2):
    """The definition over records (idxA < idxB, each pair once): -> index_of uint32[M]."""
    ia, ib = recs["idxA"].astype(np.int64), recs["idxB"].astype(np.int64)
    src, dst = np.concatenate([ia, ib]), np.concatenate([ib, ia])
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    start = np.searchsorted(src, np.arange(M + 1))
    out = np.full(M, NO, dtype=np.uint32)
    eligible = p <= p2          # (NaN compares false)
    cand = np.nonzero(p <= p1)[0]
    for v in cand[np.argsort(p[cand], kind="stable")].tolist():
        if out[v] != NO:
            continue
        out[v] = v
        nb = dst[start[v]:start[v + 1]]
        nb = nb[(out[nb] == NO) & eligible[nb]]
        out[nb] = v
    return out


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return wall, {k: tm[k] for k in ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")}, out


def median_run(runs, key):
    return sorted(runs, key=lambda r: r[key])[len(runs) // 2]


result = {"what": "ld_clump (b) against ld_all(minR2=thr) with records delivered plus the clump on the host (a): ms per call, one process, "
                  "alternating, medians over reps; planted synthetic input; P = 10 ** (-8 * default_rng(77).random(M))", "reps": args.reps, "shapes": []}
eng = T.HipLd(0)
for name, N, M, mode, key in SHAPES:
    eng.set_problem(N, M)
    eng.generate_synthetic(42, plant=T.Plant.spread(M))
    p = 10.0 ** (-8.0 * np.random.default_rng(77).random(M))
    for thr in CUTS:
        f = T.Filters(minR2=thr)
        for p1, p2 in THRESHOLDS:
            def a():
                recs, _, _ = eng.ld_all(mode, f)
                t0 = time.perf_counter()
                index_of = host_clump(recs, M, p, p1, p2)
                return index_of, len(recs), (time.perf_counter() - t0) * 1e3

            def b():
                out = eng.ld_clump(mode, f, p, p1, p2)
                return out, eng.clump_last()

            (xa, n_recs, _), ((xb, n_clumps, n_members, n_edges, _), _) = a(), b()          # warm-up of each, and agreement outside the clock
            assert n_edges == n_recs and xa.tobytes() == xb.tobytes() and n_clumps == int((xa == np.arange(M)).sum()), \
                f"{name} thr={thr} p1={p1}: the two ways disagree"
            runs_a, runs_b = [], []
            for _ in range(args.reps):
                wa, ta, oa = timed(eng, a)
                wb, tb, ob = timed(eng, b)
                runs_a.append({"wall_ms": wa, "host_clump_ms": oa[2], **ta, "records": int(oa[1])})
                runs_b.append({"wall_ms": wb, **tb, "walk_ms": ob[1]["walk_ms"], "bitmap_bytes": int(ob[1]["bitmap_bytes"])})
            mb = median_run(runs_b, "wall_ms")
            wa = [r["wall_ms"] for r in runs_a]; wb = [r["wall_ms"] for r in runs_b]
            walk = float(np.median([r["walk_ms"] for r in runs_b]))
            shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "thr": thr, "p1": p1, "p2": p2, "pairs": M * (M - 1) // 2,
                     "edges": int(n_edges), "clumps": int(n_clumps), "members": int(n_members), "index_of_equal": True,
                     "a_records_then_host_clump": runs_a, "b_ld_clump": runs_b,
                     "a_wall_ms_median": float(np.median(wa)), "b_wall_ms_median": float(np.median(wb)),
                     "a_wall_ms_min_max": [min(wa), max(wa)], "b_wall_ms_min_max": [min(wb), max(wb)],
                     "a_host_clump_ms_median": float(np.median([r["host_clump_ms"] for r in runs_a])),
                     "b_count_ms_median": float(np.median([r["count_ms"] for r in runs_b])),
                     "b_mask_epilogue_ms_median": float(np.median([r["stats_ms"] for r in runs_b])),
                     "b_walk_ms_median": walk, "b_walk_us_per_index_variant": 1e3 * walk / max(int(n_clumps), 1),
                     "b_walk_share_of_wall": walk / float(np.median(wb)),
                     "b_bitmap_bytes": mb["bitmap_bytes"],
                     "b_wall_minus_kernels_ms_median": float(np.median([r["wall_ms"] - r["count_ms"] - r["stats_ms"] - r["walk_ms"] for r in runs_b]))}
            result["shapes"].append(shape)
            print(f"{name} thr={thr} p1={p1} p2={p2}: {n_edges} edges, {n_clumps} clumps, {n_members} members; (a) {min(wa):.1f} .. {max(wa):.1f} ms "
                  f"(host clump {shape['a_host_clump_ms_median']:.1f}), (b) {min(wb):.1f} .. {max(wb):.1f} ms: count {shape['b_count_ms_median']:.2f}, "
                  f"mask epilogue {shape['b_mask_epilogue_ms_median']:.2f}, walk {walk:.2f} ms ({shape['b_walk_us_per_index_variant']:.3f} us per index variant), "
                  f"bitmap {mb['bitmap_bytes'] / 1e6:.1f} MB", flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("written:", args.out)
