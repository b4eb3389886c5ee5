"""LD decay binned on the device against (a) what a user does without it - every record at minR2 = 0 computed, run through Fisher's
test, sorted and copied to the host, and binned there - and (b) ld_score on the same context, which runs the same pair math per pair
and differs only in its epilogue: the kernel-level yardstick for what the histogram costs.
    python tests/sweeps/decay_timing.py [--out profiles/r09_lddecay_timing.json] [--reps 5] [--reps-a 3]
One process, one engine context, synthetic input from the on-device generator with LD planted in it (prune_timing.py's: every odd
variant a noisy copy of an even one, Plant.spread); positions are the generator's (100 bases apart, one contig) and the range is the
span of the variants, so that all 1000 bins are populated.  Per shape, alternating after a warm-up of each:
  (a) ld_all(mode, Filters(minR2=0)) with the records delivered, then the numpy binning a user would write (bincount of
      |posA - posB| // width with R2 as weights) - both in the clock, reported separately; --reps-a runs (a run holds every record
      of the shape in host memory: 20 GB at 20,000 variants);
  (b) ld_score(mode, Filters(minR2=0));
  (c) ld_decay(mode, Filters(minR2=0), range, 1000 bins); on the first shape also with 1 bin (every lane of a block on one LDS word)
      and 4096 bins (the cap: 48 KiB of LDS a block, the occupancy extreme).
Every call returns when its last byte is on the host, so the wall time around a call is device-synchronised; count_ms and stats_ms
are the engine's own device events around the count kernels and the epilogue (twk_hip_timing).  Before anything is timed (c) must
equal (a)'s records binned in integers, bit for bit (tests/test_gpu_decay.py: the same check), and the floating-point bins of (a)
within the quantisation (2^-33 a pair).  Medians of the runs.  Fails without a
GPU."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_lddecay_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--reps-a", type=int, default=3)
ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes (debug)")
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("decay_timing: no HIP device visible")
assert args.reps >= 5 and args.reps_a >= 3, "medians of at least 5 runs ((a): 3)"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("100,000 x 4,000 -u", 100_000, 4_000, T.MODE_UNPHASED, "u")]
N_BINS = 1000
KEYS = ("count_ms", "stats_ms", "finish_ms", "count_launches", "stats_launches", "variant_pairs")


def host_bins(recs, pos, range_bp, n_bins):
    """The decay table from records (one contig, distinct positions), as a user's script would build it -> (n, sum_r2)."""
    d = np.abs(pos[recs["idxA"]] - pos[recs["idxB"]])
    b = np.minimum(d // (range_bp // n_bins), n_bins - 1)
    return np.bincount(b, minlength=n_bins).astype(np.uint64), np.bincount(b, weights=recs["R2"], minlength=n_bins)


def exact_bins(recs, pos, range_bp, n_bins):
    """The same in the engine's integers: q = rint(R2 * 2^32) summed exactly -> (n, sum_r2)."""
    d = np.abs(pos[recs["idxA"]] - pos[recs["idxB"]])
    b = np.minimum(d // (range_bp // n_bins), n_bins - 1)
    q = np.rint(recs["R2"] * 4294967296.0).astype(np.uint64)
    # three slices of q, each summed by bincount in float64: below 2^16 (2^1 for the top one) a record and fewer than 2^31 records, so
    # every partial sum is an integer below 2^53 and exact
    parts = [np.bincount(b, weights=((q >> np.uint64(sh)) & np.uint64(mask)).astype(np.float64), minlength=n_bins)
             for sh, mask in ((32, 0xFFFF), (16, 0xFFFF), (0, 0xFFFF))]
    s = np.array([float((int(x) << 32) + (int(y) << 16) + int(z)) / 2 ** 32 for x, y, z in zip(*parts)], dtype=np.float64)
    return np.bincount(b, minlength=n_bins).astype(np.uint64), s


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return wall, {k: tm[k] for k in KEYS}, out


def med(runs, key):
    return float(np.median([r[key] for r in runs]))


result = {"what": "ld_decay (c) against ld_all(minR2=0) with records delivered plus the numpy binning on the host (a) and against ld_score on the same "
                  "context (b): ms per call, one process, alternating, medians over reps; planted synthetic input, positions 100 bases apart, "
                  "range = the variants' span", "reps": args.reps, "reps_a": args.reps_a, "n_bins": N_BINS, "shapes": []}
eng = T.HipLd(0)
f = T.Filters(minR2=0.0)
for k, (name, N, M, mode, key) in enumerate(SHAPES):
    if str(k) not in args.shapes.split(","):
        continue
    eng.set_problem(N, M)
    eng.generate_synthetic(42, plant=T.Plant.spread(M))
    # the generator's metadata (twk_hip_generate_synthetic: one contig, pos = 1000 + 100 v; tests/test_formats.py pins the same for the
    # host twin); if it ever differs, the bit-for-bit agreement in front of the clock fails
    pos = 1000 + 100 * np.arange(M, dtype=np.int64)
    range_bp = 100 * M

    def a():
        recs, _, _ = eng.ld_all(mode, f)
        t0 = time.perf_counter()
        n, s = host_bins(recs, pos, range_bp, N_BINS)
        return n, s, len(recs), (time.perf_counter() - t0) * 1e3, recs.nbytes

    def b():
        return eng.ld_score(mode, f)

    def c(n_bins=N_BINS):
        return eng.ld_decay(mode, f, range_bp, n_bins)

    # warm-up of each, and agreement outside the clock
    recs, _, _ = eng.ld_all(mode, f)
    n_recs = len(recs)
    en, es = exact_bins(recs, pos, range_bp, N_BINS)
    hn, hs = host_bins(recs, pos, range_bp, N_BINS)
    del recs
    b()
    cn, cs, c_pairs = c()
    assert np.array_equal(cn, en) and cs.tobytes() == es.tobytes(), f"{name}: ld_decay differs from its own records binned in integers"
    # ... and the floating-point bins within the quantisation, 2^-33 a pair, plus the rounding of a float64 sum of n terms
    assert np.array_equal(cn, hn) and (np.abs(cs - hs) <= cn * 2.0 ** -33 + cn * 2.0 ** -53 * hs).all(), f"{name}: ld_decay differs from the host's floating-point bins"
    extremes = [1, 4096] if k == 0 else []
    for nb in extremes:
        c(nb)
    runs_a, runs_b, runs_c, runs_x = [], [], [], {nb: [] for nb in extremes}
    for rep in range(args.reps):
        if rep < args.reps_a:
            wa, ta, oa = timed(eng, a)
            runs_a.append({"wall_ms": wa, "host_binning_ms": oa[3], **ta, "records": int(oa[2]), "record_bytes": int(oa[4])})
            del oa
        wb, tb, _ = timed(eng, b)
        runs_b.append({"wall_ms": wb, **tb})
        wc, tc, _ = timed(eng, c)
        runs_c.append({"wall_ms": wc, **tc})
        for nb in extremes:
            wx, tx, _ = timed(eng, lambda: c(nb))
            runs_x[nb].append({"wall_ms": wx, **tx})
    shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "pairs": M * (M - 1) // 2, "records": int(n_recs), "range_bp": range_bp,
             "bins_populated": int((cn > 0).sum()), "decay_equals_own_records_bit_for_bit": True,
             "a_records_then_host_binning": runs_a, "b_ld_score": runs_b, "c_ld_decay": runs_c,
             "a_wall_ms_median": med(runs_a, "wall_ms"), "a_host_binning_ms_median": med(runs_a, "host_binning_ms"), "a_record_bytes": runs_a[0]["record_bytes"],
             "b_wall_ms_median": med(runs_b, "wall_ms"), "b_count_ms_median": med(runs_b, "count_ms"), "b_epilogue_ms_median": med(runs_b, "stats_ms"),
             "c_wall_ms_median": med(runs_c, "wall_ms"), "c_count_ms_median": med(runs_c, "count_ms"), "c_epilogue_ms_median": med(runs_c, "stats_ms"),
             "c_wall_ms_min_max": [min(r["wall_ms"] for r in runs_c), max(r["wall_ms"] for r in runs_c)],
             "b_wall_ms_min_max": [min(r["wall_ms"] for r in runs_b), max(r["wall_ms"] for r in runs_b)]}
    shape["a_over_c_wall"] = shape["a_wall_ms_median"] / shape["c_wall_ms_median"]
    shape["c_over_b_epilogue"] = shape["c_epilogue_ms_median"] / shape["b_epilogue_ms_median"]
    shape["c_over_b_wall"] = shape["c_wall_ms_median"] / shape["b_wall_ms_median"]
    for nb in extremes:
        shape[f"c_{nb}_bins"] = {"runs": runs_x[nb], "wall_ms_median": med(runs_x[nb], "wall_ms"), "epilogue_ms_median": med(runs_x[nb], "stats_ms")}
    result["shapes"].append(shape)
    print(f"{name}: {n_recs} records, {shape['bins_populated']} bins populated; (a) {shape['a_wall_ms_median']:.1f} ms (host binning "
          f"{shape['a_host_binning_ms_median']:.1f}, {shape['a_record_bytes'] / 1e6:.1f} MB of records); (b) score {shape['b_wall_ms_median']:.2f} ms: count "
          f"{shape['b_count_ms_median']:.2f}, epilogue {shape['b_epilogue_ms_median']:.2f}; (c) decay {shape['c_wall_ms_median']:.2f} ms: count "
          f"{shape['c_count_ms_median']:.2f}, epilogue {shape['c_epilogue_ms_median']:.2f}; a / c {shape['a_over_c_wall']:.1f}, epilogue c / b "
          f"{shape['c_over_b_epilogue']:.3f}" + "".join(f"; {nb} bins: {shape[f'c_{nb}_bins']['wall_ms_median']:.2f} ms, epilogue "
                                                          f"{shape[f'c_{nb}_bins']['epilogue_ms_median']:.2f}" for nb in extremes), flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("written:", args.out)
