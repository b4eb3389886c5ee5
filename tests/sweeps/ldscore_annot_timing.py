"""Partitioned LD scores (ld_score_annot) against ld_score on the same context - the same pair math per pair, so the difference of the
two epilogues is what the annotation product costs - and, on the smallest shape, against what a user does without it: every record at
minR2 = 0 computed, sorted, copied to the host and multiplied into the annotations there with numpy.
    python tests/sweeps/ldscore_annot_timing.py [--out profiles/ldscore_annot_timing.json] [--reps 5] [--limit 300]
The three shapes of profiles/r07_ldscore_timing.json, synthetic input from the on-device generator with LD planted in it
(decay_timing.py's), at C = 1, 8, 64 and 97 categories, once with dense random annotations (U(0, 1)) and once with binary ones that are
5 % ones.  EVERY SHAPE RUNS IN A PROCESS OF ITS OWN UNDER ITS OWN `timeout` (--limit seconds): this script starts them one after the other
with --step K, never touches the GPU itself, and stops at the first that fails - nothing more is started on a device after a fault.
Per shape, after a warm-up of each and alternating: ld_score, then ld_score_annot per (kind, C); wall ms around the call (every call
returns when its last byte is on the host) and the engine's own device events (count_ms: the count kernels, stats_ms: the epilogue).
Before the clock n_partners must equal ld_score's and an all-ones column its sum within the quantisation (2^-33 a record).  Medians.
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldscore_annot_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limit", type=int, default=300, help="seconds a shape's process may take")
ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes (debug)")
ap.add_argument("--step", type=int, default=None, help="(internal) run shape K in this process and write --out")
args = ap.parse_args()
assert args.reps >= 5, "medians of at least 5 runs"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, "p"), ("100,000 x 10,000 -p", 100_000, 10_000, "p"), ("100,000 x 4,000 -u", 100_000, 4_000, "u")]
SMALLEST = 2          # by pairs: the records-plus-numpy path runs there
CATEGORIES = (1, 8, 64, 97)
KEYS = ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")
WHAT = ("ld_score_annot against ld_score on the same context, and on the smallest shape against ld_all(minR2=0) with the records delivered plus "
        "the numpy product on the host: ms per call, one process per shape, alternating, medians over reps; planted synthetic input; "
        "dense = U(0, 1) annotations, sparse = binary, 5 % ones")

if args.step is None:
    result = {"what": WHAT, "reps": args.reps, "categories": list(CATEGORIES), "shapes": []}
    for k in [int(x) for x in args.shapes.split(",")]:
        part = args.out + f".shape{k}"
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", str(k), "--out", part, "--reps", str(args.reps)])
        if r.returncode != 0:
            sys.exit(f"ldscore_annot_timing: shape {k} ended with status {r.returncode}; nothing more is started")
        with open(part) as fh:
            result["shapes"].append(json.load(fh))
        os.remove(part)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("written:", args.out)
    sys.exit(0)

# ---- one shape, in this process ----------------------------------------------------------------------------------------------------
import numpy as np

import tomahawk_amd as T

if T.device_count() < 1:
    sys.exit("ldscore_annot_timing: no HIP device visible")
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


def host_product(eng, annot):
    """What a user's script does: the records, then per column two weighted bincounts -> (score, records, ms of the numpy part)."""
    recs, _, _ = eng.ld_all(mode, f)
    t0 = time.perf_counter()
    ia, ib, r2 = recs["idxA"], recs["idxB"], recs["R2"]
    out = np.empty(annot.shape)
    for c in range(annot.shape[1]):
        col = annot[:, c]
        out[:, c] = np.bincount(ia, weights=r2 * col[ib], minlength=M) + np.bincount(ib, weights=r2 * col[ia], minlength=M)
    return out, len(recs), (time.perf_counter() - t0) * 1e3


rng = np.random.default_rng(97)
dense = rng.random((M, max(CATEGORIES)))
sparse = (rng.random((M, max(CATEGORIES))) < 0.05).astype(np.float64)
eng = T.HipLd(0)
eng.set_problem(N, M)
eng.generate_synthetic(42, plant=T.Plant.spread(M))
# warm-up and agreement outside the clock
sn, ss, _ = eng.ld_score(mode, f)
an, as_, _ = eng.ld_score_annot(mode, f, np.ones(M))
assert np.array_equal(an, sn) and (np.abs(as_[:, 0] - ss) <= sn * 2.0 ** -33 + 2 * M * 2.0 ** -53 * ss).all(), f"{name}: an all-ones column is not the LD score"
for kind in (dense, sparse):
    for C in CATEGORIES:
        eng.ld_score_annot(mode, f, np.ascontiguousarray(kind[:, :C]))
runs_b = []
runs = {(kname, C): [] for kname in ("dense", "sparse") for C in CATEGORIES}
for rep in range(args.reps):
    wb, tb, _ = timed(eng, lambda: eng.ld_score(mode, f))
    runs_b.append({"wall_ms": wb, **tb})
    for kname, kind in (("dense", dense), ("sparse", sparse)):
        for C in CATEGORIES:
            a = np.ascontiguousarray(kind[:, :C])
            w, t, _ = timed(eng, lambda: eng.ld_score_annot(mode, f, a))
            runs[(kname, C)].append({"wall_ms": w, **t})
shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "pairs": M * (M - 1) // 2, "all_ones_column_is_the_ld_score": True,
         "b_ld_score": runs_b, "b_wall_ms_median": med(runs_b, "wall_ms"), "b_count_ms_median": med(runs_b, "count_ms"),
         "b_epilogue_ms_median": med(runs_b, "stats_ms"), "annot": []}
for (kname, C), rr in runs.items():
    e = {"annotations": kname, "categories": C, "runs": rr, "wall_ms_median": med(rr, "wall_ms"), "count_ms_median": med(rr, "count_ms"),
         "epilogue_ms_median": med(rr, "stats_ms"), "wall_ms_min_max": [min(r["wall_ms"] for r in rr), max(r["wall_ms"] for r in rr)]}
    e["epilogue_over_score_epilogue"] = e["epilogue_ms_median"] / shape["b_epilogue_ms_median"]
    e["extra_epilogue_ms_per_8_categories"] = (e["epilogue_ms_median"] - shape["b_epilogue_ms_median"]) / (C / 8.0)
    e["wall_over_score_wall"] = e["wall_ms_median"] / shape["b_wall_ms_median"]
    shape["annot"].append(e)
    print(f"{name} {kname} C={C}: wall {e['wall_ms_median']:.2f} ms (score {shape['b_wall_ms_median']:.2f}), epilogue {e['epilogue_ms_median']:.2f} ms "
          f"(score {shape['b_epilogue_ms_median']:.2f}): {e['extra_epilogue_ms_per_8_categories']:.3f} ms more per 8 categories", flush=True)
if args.step == SMALLEST:
    shape["records_then_numpy"] = []
    for C in CATEGORIES:
        a = np.ascontiguousarray(dense[:, :C])
        t0 = time.perf_counter()
        got, n_recs, numpy_ms = host_product(eng, a)
        wall = (time.perf_counter() - t0) * 1e3
        dev = eng.ld_score_annot(mode, f, a)[1]
        assert (np.abs(dev - got) <= sn[:, None] * 2.0 ** -33 + 4 * M * 2.0 ** -53 * np.abs(got)).all(), f"{name}: C={C} differs from the host's floating-point product"
        annot_wall = next(e["wall_ms_median"] for e in shape["annot"] if e["annotations"] == "dense" and e["categories"] == C)
        shape["records_then_numpy"].append({"categories": C, "records": int(n_recs), "wall_ms": wall, "numpy_ms": numpy_ms, "over_annot_wall": wall / annot_wall})
        print(f"{name} records + numpy C={C}: {wall:.0f} ms ({numpy_ms:.0f} in numpy), {wall / annot_wall:.0f} x the device call", flush=True)
eng.close()
with open(args.out, "w") as fh:
    json.dump(shape, fh, indent=1)
