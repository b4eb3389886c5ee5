"""Haplotype blocks: where the time of ld_blocks goes, against the banded matrix on the same context and against the route through
records and NumPy.
    python tests/sweeps/blocks_timing.py [--out profiles/blocks_timing.json] [--reps 5] [--window 50000] [--no-records]
One process, one engine context, synthetic input from the on-device generator with LD planted in it (bandmat_timing.py's shapes and
input: positions 1000 + 100 v on one contig, so the default window of 50,000 bases is +-500 variants) and, because the generator's
planted pairs form no block, one block-structured set from the host (tests/util.py's mosaic of founder haplotypes, 250 samples x
4,000 variants, the same positions), which is what exercises the sort and the walk.  Per shape, alternating after
a warm-up of each:
  (a) ld_matrix_band(mode, Filters(minR2=0), W, stat=STAT_DPRIME): the yardstick - the same launches, band map and write-out, four
      bytes a slot and no scan;
  (b) ld_dprime_ci_band(mode, Filters(minR2=0), W): the bounds alone, two bytes a slot;
  (c) ld_blocks(mode, Filters(minR2=0), W): the bounds kept on the device, then prefix counts, candidate counts and scan, the
      emitting pass, the sort, the walk.
Reported per call: wall, the count kernels (count_ms), the epilogue (stats_ms: for (b) and (c) the pair function and the likelihood
scan), and for (c) the stages behind it from twk_hip_blocks_stages / twk_hip_blocks_last, the band's bytes, candidates and blocks.
Once per shape, outside the alternation and unless --no-records: (d) ld_region with the same arguments, its records' bounds and the
blocks by the NumPy restatement of tests/blocks_cases.py where that fits in memory (n <= 4000), else the bounds alone - and the two
routes must agree wherever both ran.  Medians of --reps runs; nothing is fixed in advance.  Fails without a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

import tomahawk_amd as T
from tests import blocks_cases as BC

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--window", type=int, default=50_000)
ap.add_argument("--no-records", action="store_true")
ap.add_argument("--shapes", default="0,1,2,3")
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("blocks_timing: no HIP device visible")
assert args.reps >= 5, "medians of at least 5 runs"

SHAPES = [("2,504 x 20,000 -p", 2504, 20_000, T.MODE_PHASED, "p"),
          ("100,000 x 10,000 -p", 100_000, 10_000, T.MODE_PHASED, "p"),
          ("100,000 x 4,000 -u", 100_000, 4_000, T.MODE_UNPHASED, "u"),
          ("mosaic 250 x 4,000 -p", 250, 4_000, T.MODE_PHASED, "p")]
KEYS = ("count_ms", "stats_ms", "count_launches", "stats_launches", "variant_pairs")


def timed(eng, call):
    eng.timing_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    tm = eng.timing()
    return {"wall_ms": wall, **{k: tm[k] for k in KEYS}}, out


def medians(runs):
    return {k + "_median": float(np.median([r[k] for r in runs])) for k in runs[0] if k.endswith("_ms")}


W = args.window
result = {"what": "ld_blocks (c) against ld_dprime_ci_band (b) and ld_matrix_band (a) on the same context, and once against records + NumPy (d): "
                  "ms per call, one process, alternating, medians over reps; planted synthetic input", "reps": args.reps, "window_bases": W, "shapes": []}
eng = T.HipLd(0)
f = T.Filters(minR2=0.0)
for k in (int(x) for x in args.shapes.split(",")):
    name, N, M, mode, key = SHAPES[k]
    if name.startswith("mosaic"):      # block-structured data from the host (tests/util.py): the planted pairs of the generator form no block
        from oracle import oracle as O
        from tests import util
        al = util.mosaic_alleles(M, N, 5004, n_founders=7, switch=0.02, mut=0.002)
        util.upload(eng, al, O.variants_from_alleles(al, pos=(1000 + 100 * np.arange(M)).astype(np.uint32)))
        del al
    else:
        eng.set_problem(N, M)
        eng.generate_synthetic(42, plant=T.Plant.spread(M))
    calls = {"a_ld_matrix_band": lambda: eng.ld_matrix_band(mode, f, W, stat=T.STAT_DPRIME, fill=0.0),
             "b_ld_dprime_ci_band": lambda: eng.ld_dprime_ci_band(mode, f, W),
             "c_ld_blocks": lambda: eng.ld_blocks(mode, f, W)}
    warm = {tag: call() for tag, call in calls.items()}
    lo, hi, first, indptr, nrec, _ = warm["b_ld_dprime_ci_band"]
    block_of, b_first, b_last, b_s, b_r, n_cand, n_inf, _ = warm["c_ld_blocks"]
    assert n_inf == nrec == warm["a_ld_matrix_band"][3], f"{name}: the three calls disagree on the informative pairs"
    nnz = int(indptr[-1])
    shape = {"name": name, "n_samples": N, "n_variants": M, "mode": key, "nnz": nnz, "informative": int(n_inf), "candidates": int(n_cand),
             "blocks": int(len(b_first)), "largest_block": int((b_last - b_first + 1).max()) if len(b_first) else 0}
    del warm
    runs = {tag: [] for tag in calls}
    for _ in range(args.reps):
        for tag, call in calls.items():
            r, out = timed(eng, call)
            if tag == "c_ld_blocks":
                last = eng.blocks_last()
                r.update({"counts_ms": last["counts_ms"], "emit_ms": last["emit_ms"], "sort_ms": last["sort_ms"], "walk_ms": last["walk_ms"]})
                shape["band_bytes"] = int(last["band_bytes"])
            del out
            runs[tag].append(r)
    for tag in calls:
        shape[tag] = {"runs": runs[tag], **medians(runs[tag])}
    if not args.no_records:
        t0 = time.perf_counter()
        recs, _, _ = eng.ld_region(mode, f, 0, M, 0, M, True, window=T.OPT_WINDOW, l_window=W)
        t1 = time.perf_counter()
        want_lo, want_hi, gap = BC.band_of_records(recs, first, indptr)
        t2 = time.perf_counter()
        d = {"records": int(len(recs)), "ld_region_ms": (t1 - t0) * 1e3, "numpy_bounds_ms": (t2 - t1) * 1e3, "smallest_gap": gap,
             "bounds_differ": int(((lo != want_lo) | (hi != want_hi)).sum())}
        if M <= 4000:
            pos = 1000 + 100 * np.arange(M)
            want = BC.blocks_of(lo, hi, first, indptr, pos)
            d["numpy_blocks_ms"] = (time.perf_counter() - t2) * 1e3
            d["blocks_agree"] = bool(np.array_equal(want["first"], b_first) and np.array_equal(want["last"], b_last))
        shape["d_records_numpy"] = d
        del recs, want_lo, want_hi
    result["shapes"].append(shape)
    c = shape["c_ld_blocks"]
    print(f"{name}: window +-{W} bases, nnz {nnz}, {n_inf} informative, {n_cand} candidates, {shape['blocks']} blocks; "
          f"(a) band D' wall {shape['a_ld_matrix_band']['wall_ms_median']:.1f} ms (epilogue {shape['a_ld_matrix_band']['stats_ms_median']:.2f}); "
          f"(b) bounds wall {shape['b_ld_dprime_ci_band']['wall_ms_median']:.1f} ms (epilogue {shape['b_ld_dprime_ci_band']['stats_ms_median']:.2f}); "
          f"(c) blocks wall {c['wall_ms_median']:.1f} ms: count {c['count_ms_median']:.2f}, bounds epilogue {c['stats_ms_median']:.2f}, counts {c['counts_ms_median']:.2f}, "
          f"emit {c['emit_ms_median']:.2f}, sort {c['sort_ms_median']:.2f}, walk {c['walk_ms_median']:.2f} ms, band {shape['band_bytes'] / 1e6:.1f} MB"
          + (f"; (d) {shape['d_records_numpy']}" if "d_records_numpy" in shape else ""), flush=True)
    with open(args.out, "w") as fh:          # (after every shape: what ran is kept)
        json.dump(result, fh, indent=1)
eng.close()
print("written:", args.out)
