"""Sample subsets (select_samples): what the selection kernel reaches, and what selecting on the device saves.
    python tests/sweeps/subset_timing.py [--out profiles/subset_timing.json] [--reps 5] [--limit 900]
THE KERNEL, on three shapes of synthetic input from the on-device generator - 2,504 -> 503 samples x 20,000 variants (one population of
1000 Genomes), 100,000 -> 10,000 x 10,000, and 1,000,000 -> 2,504 x 50,000 (the sparse case: a kept sample every 400) - keep lists drawn
at random: select_last()'s kernel time, the bytes of source words it asked for and of working rows it wrote, and the rate
(bytes_read + bytes_written) / time.  bytes_read counts the 4-byte source words that hold a kept sample; what the memory system moves
for them is whole lines, so for the sparse list the figure beside it is the one to read: source_row_bytes, the dense rows it did NOT
read.  For comparison the rate csrc/tools/hbm_read_bw.hip reaches on the same machine (build/hbm_read_bw, `make tools`; skipped with a
note if it is not built).
THE PAY-OFF, on the first two shapes, wall ms: ld_score (phased, minR2 = 0) after select_samples (the selection's own wall time is
reported beside it); ld_score on the full set; and today's route - download() -> the subset in NumPy (unpack the 2-bit fields, take
the columns, pack) -> set_problem + upload -> ld_score - whose scores must equal the selected context's, bit for bit.
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--limit", type=int, default=900, help="seconds a shape's process may take")
ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes (debug)")
ap.add_argument("--step", type=int, default=None, help="(internal) run shape K in this process and write --out")
args = ap.parse_args()
assert args.reps >= 5, "medians of at least 5 runs"

# name, source samples, kept samples, variants, pay-off measured
SHAPES = [("2,504 -> 503 x 20,000", 2504, 503, 20_000, True), ("100,000 -> 10,000 x 10,000", 100_000, 10_000, 10_000, True),
          ("1,000,000 -> 2,504 x 50,000 (sparse)", 1_000_000, 2504, 50_000, False)]
WHAT = ("select_samples on synthetic input, keep lists drawn at random: the kernel's time, bytes and rate ((bytes_read + bytes_written) / time; "
        "bytes_read = the 4-byte source words with a kept sample), hbm_read_bw's rate on the same machine, and wall ms of ld_score -p minR2 = 0 "
        "after the selection, on the full set, and by today's route (download, NumPy subset, set_problem + upload, ld_score); one process per "
        "shape, alternating, medians over reps")

if args.step is None:
    result = {"what": WHAT, "reps": args.reps, "shapes": []}
    bw = os.path.join(ROOT, "build", "hbm_read_bw")
    if os.path.exists(bw):
        r = subprocess.run(["timeout", "-k", "10", "120", bw, "8"], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"subset_timing: hbm_read_bw ended with status {r.returncode}; nothing more is started")
        rates = [float(x) for x in re.findall(r"-> ([0-9.]+) GB/s", r.stdout)]
        result["hbm_read_bw"] = {"output": r.stdout.splitlines(), "best_gb_per_s": max(rates)}
    else:
        result["hbm_read_bw"] = {"note": "build/hbm_read_bw is not built (`make tools`)"}
    for k in [int(x) for x in args.shapes.split(",")]:
        part = args.out + f".shape{k}"
        r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--step", str(k), "--out", part, "--reps", str(args.reps)])
        if r.returncode != 0:
            sys.exit(f"subset_timing: shape {k} ended with status {r.returncode}; nothing more is started")
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
    sys.exit("subset_timing: no HIP device visible")
name, N, n_keep, M, payoff = SHAPES[args.step]
keep = np.sort(np.random.default_rng(7).choice(N, size=n_keep, replace=False)).astype(np.uint32)
f = T.Filters(minR2=0.0)


def wall(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def med(xs):
    return float(np.median(xs))


def host_subset(data, keep, n_keep):
    """uint64 [M, w] raw rows -> the rows of the kept samples, in slabs of variants (the unpacked bits of 100,000 samples are 200 kB a row)."""
    w_out = T.hip.words64(n_keep)
    out = np.zeros((data.shape[0], w_out), dtype=np.uint64)
    cols = np.stack([2 * keep.astype(np.int64), 2 * keep.astype(np.int64) + 1], axis=1).reshape(-1)
    for v0 in range(0, data.shape[0], 512):
        bits = np.unpackbits(data[v0:v0 + 512].view(np.uint8), axis=1, bitorder="little")[:, cols]
        packed = np.packbits(bits, axis=1, bitorder="little")
        out[v0:v0 + 512].view(np.uint8)[:, :packed.shape[1]] = packed
    return out


def host_route(eng, other):
    data, _ = eng.download()
    sub = host_subset(data, keep, n_keep)
    meta = eng.meta()
    meta["ac"] = np.unpackbits(sub.view(np.uint8), axis=1).sum(axis=1)
    other.set_problem(n_keep, M)
    other.upload(sub, meta)
    return other.ld_score(T.MODE_PHASED, f)


eng = T.HipLd(0)
eng.set_problem(N, M)
eng.generate_synthetic(42)
shape = {"name": name, "n_source": N, "n_kept": n_keep, "n_variants": M, "source_row_bytes": M * ((2 * N + 31) // 32) * 4, "select": []}
eng.select_samples(keep)          # warm-up outside the clock
eng.select_samples(None)
sel_runs, after, full, route = [], [], [], []
other = T.HipLd(0) if payoff else None
if payoff:
    eng.ld_score(T.MODE_PHASED, f)
    want = host_route(eng, other)
for rep in range(args.reps):
    w, _ = wall(lambda: eng.select_samples(keep))
    last = eng.select_last()
    last["wall_ms"] = w
    last["gb_per_s"] = (last["bytes_read"] + last["bytes_written"]) / (last["select_ms"] * 1e-3) / 1e9
    sel_runs.append(last)
    if payoff:
        w, got = wall(lambda: eng.ld_score(T.MODE_PHASED, f))
        after.append(w)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), f"{name}: the selected context's scores differ from the host route's"
    eng.select_samples(None)
    if payoff:
        full.append(wall(lambda: eng.ld_score(T.MODE_PHASED, f))[0])
        route.append(wall(lambda: host_route(eng, other))[0])
shape["select"] = {"runs": sel_runs, "select_ms_median": med([r["select_ms"] for r in sel_runs]), "wall_ms_median": med([r["wall_ms"] for r in sel_runs]),
                   "gb_per_s_median": med([r["gb_per_s"] for r in sel_runs]), "bytes_read": sel_runs[0]["bytes_read"], "bytes_written": sel_runs[0]["bytes_written"],
                   "bytes_read_over_source_rows": sel_runs[0]["bytes_read"] / shape["source_row_bytes"]}
s = shape["select"]
print(f"{name}: kernel {s['select_ms_median']:.3f} ms, {s['gb_per_s_median']:.0f} GB/s, reads {s['bytes_read_over_source_rows']:.3f} of the source rows; "
      f"call {s['wall_ms_median']:.1f} ms", flush=True)
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
