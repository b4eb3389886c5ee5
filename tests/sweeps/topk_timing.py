"""Top-k LD partners (ld_topk) against ld_score on the same context - the same pair math per pair, so the difference of the two
epilogues is what the selection costs - and, on the smallest shape, against what a user does without it: every record at minR2 = 0
computed, sorted, copied to the host and cut to the k strongest per variant there with numpy.
    python tests/sweeps/topk_timing.py [--out profiles/topk_timing.json] [--reps 5] [--limit 400]
The three shapes of profiles/r07_ldscore_timing.json, synthetic input from the on-device generator, at k = 1, 8 and 32, in TWO ORDERS
of data, because the order decides when the lists fill and the thresholds begin to bite: "near" - LD planted between neighbours
(Plant.near, distance 1): the strongest partner sits next to the diagonal - and "iid" - nothing planted: every list keeps changing to
the end.  EVERY SHAPE RUNS IN A PROCESS OF ITS OWN UNDER ITS OWN `timeout` (--limit seconds): this script starts them one after the
other with --step K, never touches the GPU itself, and stops at the first that fails - nothing more is started on a device after a fault.
Per shape and order, after a warm-up of each and alternating: ld_score, then ld_topk per k; wall ms around the call (every call returns
when its last byte is on the host) and the engine's own device events (count_ms: the count kernels, stats_ms: the epilogue).  Medians.
THE FLUSH'S SHARE: a second pass per shape (--step K --no-flush) loads a library of its own, build/topk_noflush/libtwk_hip.so - the
engine compiled with -DTWK_TOPK_TIMING_SKIP_FLUSH, which leaves the global cascade out of k_ld_topk's flush (`make hip` never defines
it; this script builds the library if it is not there).  Its lists are wrong and are not looked at: only its epilogue times are kept.
Without the flush the global lists stay empty, so the thresholds the blocks load stay 0 as well: the variant's time is the flush's
cost taken away AND the thresholds' saving taken away, and no_flush_over_epilogue says which of the two is larger.
Fails without a GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limit", type=int, default=400, help="seconds a shape's process may take")
ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes (debug)")
ap.add_argument("--step", type=int, default=None, help="(internal) run shape K in this process and write --out")
ap.add_argument("--no-flush", action="store_true", help="(internal) the timing-only library without the flush's atomics")
args = ap.parse_args()
assert args.reps >= 5, "medians of at least 5 runs"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, "p"), ("100,000 x 10,000 -p", 100_000, 10_000, "p"), ("100,000 x 4,000 -u", 100_000, 4_000, "u")]
SMALLEST = 2          # by pairs: the records-plus-numpy path runs there
KS = (1, 8, 32)
ORDERS = ("near", "iid")
KEYS = ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")
NOFLUSH_DIR = os.path.join(ROOT, "build", "topk_noflush")
NOFLUSH_LIB = os.path.join(NOFLUSH_DIR, "libtwk_hip.so")
WHAT = ("ld_topk (r2) against ld_score on the same context, and on the smallest shape against ld_all(minR2=0) with the records delivered plus "
        "a numpy top-k on the host: ms per call, one process per shape, alternating, medians over reps; synthetic input, near = LD planted "
        "between neighbours, iid = nothing planted; no_flush_epilogue_ms: the same epilogue from a timing-only build whose flush skips its "
        "global atomics (wrong lists, and thresholds that never rise: above 1 the flush earns more than it costs)")

if args.step is None:
    if not os.path.exists(NOFLUSH_LIB):
        flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -DTWK_TOPK_TIMING_SKIP_FLUSH"
        subprocess.run(["make", "-C", ROOT, "hip", "LIBDIR=" + NOFLUSH_DIR, "HIPFLAGS=" + flags], check=True)
    result = {"what": WHAT, "reps": args.reps, "k": list(KS), "shapes": []}
    for k in [int(x) for x in args.shapes.split(",")]:
        parts = []
        for extra in ([], ["--no-flush"]):
            part = args.out + f".shape{k}" + ("nf" if extra else "")
            r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", str(k), "--out", part,
                                "--reps", str(args.reps)] + extra)
            if r.returncode != 0:
                sys.exit(f"topk_timing: shape {k} {extra} ended with status {r.returncode}; nothing more is started")
            with open(part) as fh:
                parts.append(json.load(fh))
            os.remove(part)
        shape, nf = parts
        for e, n in zip(shape["topk"], nf["topk"]):
            assert (e["order"], e["k"]) == (n["order"], n["k"])
            e["no_flush_epilogue_ms_median"] = n["epilogue_ms_median"]
            e["no_flush_over_epilogue"] = n["epilogue_ms_median"] / e["epilogue_ms_median"]
        result["shapes"].append(shape)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written:", args.out)
    sys.exit(0)

# ---- one shape, in this process ----------------------------------------------------------------------------------------------------
import numpy as np

import tomahawk_amd.hip as H

if args.no_flush:
    H.LIB_PATH = NOFLUSH_LIB
import tomahawk_amd as T

if T.device_count() < 1:
    sys.exit("topk_timing: no HIP device visible")
name, N, M, key = SHAPES[args.step]
mode = T.MODE_PHASED if key == "p" else T.MODE_UNPHASED
f = T.Filters(minR2=0.0)


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return wall, {k: tm[k] for k in KEYS}, out


def med(runs, k):
    return float(np.median([r[k] for r in runs]))


def host_topk(eng, k):
    """What a user's script does: the records, then a sort per variant -> (idx, val, records, ms of the numpy part)."""
    recs, _, _ = eng.ld_all(mode, f)
    t0 = time.perf_counter()
    owner = np.concatenate([recs["idxA"], recs["idxB"]]).astype(np.int64)
    partner = np.concatenate([recs["idxB"], recs["idxA"]]).astype(np.int64)
    v = np.concatenate([recs["R2"], recs["R2"]]).astype(np.float32)
    order = np.lexsort((partner, -v, owner))
    owner, partner, v = owner[order], partner[order], v[order]
    rank = np.arange(len(owner)) - np.searchsorted(owner, np.arange(M))[owner]
    keep = rank < k
    idx = np.full((M, k), T.NO_PARTNER, dtype=np.uint32)
    val = np.zeros((M, k), dtype=np.float32)
    idx[owner[keep], rank[keep]] = partner[keep]
    val[owner[keep], rank[keep]] = v[keep]
    return idx, val, len(recs), (time.perf_counter() - t0) * 1e3


eng = T.HipLd(0)
eng.set_problem(N, M)
shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "pairs": M * (M - 1) // 2, "no_flush_build": bool(args.no_flush), "score": [], "topk": []}
for order in ORDERS:
    eng.generate_synthetic(42, plant=T.Plant.near(M, 1) if order == "near" else None)
    eng.ld_score(mode, f)          # warm-up outside the clock
    for k in KS:
        eng.ld_topk(mode, f, k)
    runs_b, runs = [], {k: [] for k in KS}
    for rep in range(args.reps):
        wb, tb, _ = timed(eng, lambda: eng.ld_score(mode, f))
        runs_b.append({"wall_ms": wb, **tb})
        for k in KS:
            w, t, _ = timed(eng, lambda: eng.ld_topk(mode, f, k))
            runs[k].append({"wall_ms": w, **t, **eng.topk_last()})
    b = {"order": order, "runs": runs_b, "wall_ms_median": med(runs_b, "wall_ms"), "count_ms_median": med(runs_b, "count_ms"), "epilogue_ms_median": med(runs_b, "stats_ms")}
    shape["score"].append(b)
    for k, rr in runs.items():
        e = {"order": order, "k": k, "runs": rr, "wall_ms_median": med(rr, "wall_ms"), "count_ms_median": med(rr, "count_ms"),
             "epilogue_ms_median": med(rr, "stats_ms"), "unpack_ms_median": med(rr, "unpack_ms"), "wall_ms_min_max": [min(r["wall_ms"] for r in rr), max(r["wall_ms"] for r in rr)]}
        e["epilogue_over_score_epilogue"] = e["epilogue_ms_median"] / b["epilogue_ms_median"]
        e["wall_over_score_wall"] = e["wall_ms_median"] / b["wall_ms_median"]
        e["device_over_score_device"] = (e["count_ms_median"] + e["epilogue_ms_median"]) / (b["count_ms_median"] + b["epilogue_ms_median"])
        shape["topk"].append(e)
        print(f"{name} {order} k={k}{' (no flush)' if args.no_flush else ''}: wall {e['wall_ms_median']:.2f} ms (score {b['wall_ms_median']:.2f}), epilogue "
              f"{e['epilogue_ms_median']:.2f} ms (score {b['epilogue_ms_median']:.2f}), unpack {e['unpack_ms_median']:.2f} ms", flush=True)
    if args.step == SMALLEST and not args.no_flush:
        shape.setdefault("records_then_numpy", [])
        for k in KS:
            t0 = time.perf_counter()
            hi, hv, n_recs, numpy_ms = host_topk(eng, k)
            wall = (time.perf_counter() - t0) * 1e3
            di, dv, _ = eng.ld_topk(mode, f, k)
            assert np.array_equal(di, hi) and np.array_equal(dv.view(np.uint32), hv.view(np.uint32)), f"{name} {order}: k={k} differs from the host's lists"
            dev_wall = next(e["wall_ms_median"] for e in shape["topk"] if e["order"] == order and e["k"] == k)
            shape["records_then_numpy"].append({"order": order, "k": k, "records": int(n_recs), "wall_ms": wall, "numpy_ms": numpy_ms, "over_topk_wall": wall / dev_wall,
                                                "equal_lists": True})
            print(f"{name} {order} records + numpy k={k}: {wall:.0f} ms ({numpy_ms:.0f} in numpy), {wall / dev_wall:.0f} x the device call", flush=True)
eng.close()
with open(args.out, "w") as fh:
    json.dump(shape, fh, indent=1)
