"""Variant subsets (select_variants): what the selection's kernels reach, and what selecting on the device saves.
    python tests/sweeps/varsel_timing.py [--out profiles/varsel_timing.json] [--reps 5] [--limit 900]
THE KERNELS, on three shapes of synthetic input from the on-device generator - 2,504 samples x 20,000 variants, 100,000 x 10,000 and
1,000,000 x 50,000 - with min_maf at the median of the generator's allele frequencies, which keeps about half the variants:
select_variants_last()'s device time (predicate, scan and map; row and metadata gather), the bytes of rows read (the base once for the
predicate, the kept rows once for the gather) and written (the working rows, padding included), and the rate
(bytes_read + bytes_written) / time.  For comparison the rate csrc/tools/hbm_read_bw.hip reaches on the same machine (build/hbm_read_bw,
`make tools`; skipped with a note if it is not built) and the sample-subset kernel's figures from profiles/subset_timing.json.
THE PAY-OFF, on the first two shapes, wall ms: ld_score (phased, minR2 = 0) after select_variants (the selection's own wall time is
reported beside it); ld_score on the full set; and the route without it - download() -> the counts and the rule in NumPy -> set_problem
+ upload of the kept rows -> ld_score - whose scores must equal the selected context's, bit for bit.
EVERY SHAPE RUNS IN A PROCESS OF ITS OWN UNDER ITS OWN `timeout` (--limit seconds): this script starts them one after the other with
--step K, never touches the GPU itself, and stops at the first that fails - nothing more is started on a device after a fault.
Medians of --reps alternating runs, each after a warm-up.  Fails without a GPU."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varsel_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limit", type=int, default=900, help="seconds a shape's process may take")
ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes (debug)")
ap.add_argument("--step", type=int, default=None, help="(internal) run shape K in this process and write --out")
args = ap.parse_args()
assert args.reps >= 5, "medians of at least 5 runs"

# name, samples, variants, pay-off measured
SHAPES = [("2,504 x 20,000", 2504, 20_000, True), ("100,000 x 10,000", 100_000, 10_000, True), ("1,000,000 x 50,000", 1_000_000, 50_000, False)]
MIN_MAF = 0.275          # the generator draws the ALT frequency from U(0.05, 0.5): about half the variants lie above
WHAT = ("select_variants(min_maf=0.275) on synthetic input, about half the variants kept: the kernels' time, bytes and rate ((bytes_read + bytes_written) "
        "/ time), hbm_read_bw's rate on the same machine, the sample-subset kernel's figures (profiles/subset_timing.json), and wall ms of ld_score -p "
        "minR2 = 0 after the selection, on the full set, and by the host route (download, NumPy counts and rule, set_problem + upload, ld_score); "
        "one process per shape, alternating, medians over reps")

if args.step is None:
    result = {"what": WHAT, "reps": args.reps, "min_maf": MIN_MAF, "shapes": []}
    bw = os.path.join(ROOT, "build", "hbm_read_bw")
    if os.path.exists(bw):
        r = subprocess.run(["timeout", "-k", "10", "120", bw, "8"], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"varsel_timing: hbm_read_bw ended with status {r.returncode}; nothing more is started")
        rates = [float(x) for x in re.findall(r"-> ([0-9.]+) GB/s", r.stdout)]
        result["hbm_read_bw"] = {"output": r.stdout.splitlines(), "best_gb_per_s": max(rates)}
    else:
        result["hbm_read_bw"] = {"note": "build/hbm_read_bw is not built (`make tools`)"}
    try:
        with open(os.path.join(ROOT, "profiles", "subset_timing.json")) as fh:
            sub = json.load(fh)
        result["sample_subset_kernel"] = {"from": "profiles/subset_timing.json", "hbm_read_bw_gb_per_s": sub["hbm_read_bw"].get("best_gb_per_s"),
                                          "shapes": [{"name": s["name"], "gb_per_s_median": s["select"]["gb_per_s_median"]} for s in sub["shapes"]]}
    except OSError:
        result["sample_subset_kernel"] = {"note": "profiles/subset_timing.json is not there"}
    for k in [int(x) for x in args.shapes.split(",")]:
        part = args.out + f".shape{k}"
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", str(k), "--out", part, "--reps", str(args.reps)])
        if r.returncode != 0:
            sys.exit(f"varsel_timing: shape {k} ended with status {r.returncode}; nothing more is started")
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
    sys.exit("varsel_timing: no HIP device visible")
name, N, M, payoff = SHAPES[args.step]
f = T.Filters(minR2=0.0)


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def med(xs):
    return float(np.median(xs))


def host_rule(data):
    """uint64 [M, w] raw rows without missing data -> the rule's verdict per variant, from the bits (NumPy's popcount, in slabs of rows)."""
    E = np.uint64(0x5555555555555555)
    keep = np.zeros(data.shape[0], dtype=bool)
    for v0 in range(0, data.shape[0], 1024):
        x = data[v0:v0 + 1024]
        x0, x1 = x & E, (x >> np.uint64(1)) & E
        het = np.bitwise_count(x0 ^ x1).sum(axis=1, dtype=np.int64)
        hom = np.bitwise_count(x0 & x1).sum(axis=1, dtype=np.int64)
        alt, obs = het + 2 * hom, 2 * N
        minor = np.minimum(alt, obs - alt)
        keep[v0:v0 + 1024] = minor.astype(np.float64) >= np.float64(MIN_MAF) * np.float64(obs)
    return keep


def host_route(eng, other):
    data, _ = eng.download()
    kept = np.nonzero(host_rule(data))[0]
    meta = eng.meta()[kept]
    other.set_problem(N, len(kept))
    other.upload(np.ascontiguousarray(data[kept]), meta)
    return other.ld_score(T.MODE_PHASED, f)


eng = T.HipLd(0)
eng.set_problem(N, M)
eng.generate_synthetic(42)
row_bytes = ((2 * N + 31) // 32 + 31) // 32 * 32 * 4
shape = {"name": name, "n_samples": N, "n_variants": M, "base_row_bytes": M * row_bytes}
n_kept = eng.select_variants(min_maf=MIN_MAF)          # warm-up outside the clock
eng.select_variants(None)
shape["n_kept"] = n_kept
sel_runs, after, full, route = [], [], [], []
other = T.HipLd(0) if payoff else None
if payoff:
    eng.ld_score(T.MODE_PHASED, f)
    want = host_route(eng, other)
for rep in range(args.reps):
    w, _ = wall(lambda: eng.select_variants(min_maf=MIN_MAF))
    last = eng.select_variants_last()
    last["wall_ms"] = w
    last["gb_per_s"] = (last["bytes_read"] + last["bytes_written"]) / (last["select_ms"] * 1e-3) / 1e9
    sel_runs.append(last)
    if payoff:
        w, got = wall(lambda: eng.ld_score(T.MODE_PHASED, f))
        after.append(w)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), f"{name}: the selected context's scores differ from the host route's"
    eng.select_variants(None)
    if payoff:
        full.append(wall(lambda: eng.ld_score(T.MODE_PHASED, f))[0])
        route.append(wall(lambda: host_route(eng, other))[0])
shape["select"] = {"runs": sel_runs, "select_ms_median": med([r["select_ms"] for r in sel_runs]), "wall_ms_median": med([r["wall_ms"] for r in sel_runs]),
                   "gb_per_s_median": med([r["gb_per_s"] for r in sel_runs]), "bytes_read": sel_runs[0]["bytes_read"], "bytes_written": sel_runs[0]["bytes_written"]}
s = shape["select"]
print(f"{name}: kept {n_kept} of {M}; kernels {s['select_ms_median']:.3f} ms, {s['gb_per_s_median']:.0f} GB/s; call {s['wall_ms_median']:.1f} ms", flush=True)
if payoff:
    shape["ld_score_wall_ms"] = {"after_select": after, "full_set": full, "host_route": route, "after_select_median": med(after), "full_set_median": med(full),
                                 "host_route_median": med(route), "select_plus_score_median": med(after) + s["wall_ms_median"], "equal_scores": True}
    p = shape["ld_score_wall_ms"]
    p["host_route_over_device_route"] = p["host_route_median"] / p["select_plus_score_median"]
    print(f"{name}: ld_score after select {p['after_select_median']:.1f} ms (+ select {s['wall_ms_median']:.1f}), full set {p['full_set_median']:.1f} ms, "
          f"host route {p['host_route_median']:.1f} ms", flush=True)
    other.close()
eng.close()
with open(args.out, "w") as fh:
    json.dump(shape, fh, indent=1)
