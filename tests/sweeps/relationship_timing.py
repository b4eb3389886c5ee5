"""The sample relationship matrix at cohort sizes: where a call's time goes, and whether the count kernel runs as fast over planes of
samples as it does over planes of variants.
    python tests/sweeps/relationship_timing.py [--out profiles/r11_relationship_timing.json] [--reps 5] [--shapes 0,1,2]
One process, one engine context, synthetic input from the on-device generator (iid genotypes, no missing data: two planes a sample).
Per shape (samples x variants), after a warm-up call, --reps calls of relationship(stat=REL_KING) over all samples and variants:
  transpose_ms   k_relate_transpose (twk_hip_relationship_last)
  count_ms       the k_count_list_t launches of the call (twk_hip_timing), with their plane-row pairs; word pairs per second =
                 row_pairs x ceil(variants / 32) / count_ms - the padding the kernel skips (last_halves) is not counted as work
  epilogue_ms    k_relate_epilogue (stats_ms)
  wall_ms        around the call: it returns when the matrix is on the host, so it holds the device-to-host copy of 8 bytes a pair
Next to it the SAME kernel on variant pairs of equal row length: a problem of W x 16 samples (phased rows of W words, W the plane
pitch of the shape) x 8,192 variants, the whole triangle through the matrix form of the record path (fused = 0, minR2 = 1: no
survivors) - count_ms and row_pairs x words_per_row of that run.  It is one kernel, so a clear shortfall of the first figure against
the second points at the tile or unit lists of the relationship path, not at the hardware.  (bench.py's extra.cfg2 holds the same
kind of figure for configs[1]: 0.914 of the and+bcnt ceiling of 2.62e13 word pairs/s in profiles/r06_*.)  No test asserts a time.
Medians of --reps runs.  Fails without a GPU."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_relationship_timing.json"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", default="0,1,2")
args = ap.parse_args()
if T.device_count() < 1:
    sys.exit("relationship_timing: no HIP device visible")
assert args.reps >= 3, "medians of at least 3 runs"

SHAPES = [("2,504 x 20,000", 2504, 20_000), ("2,504 x 531,500", 2504, 531_500), ("20,000 x 50,000", 20_000, 50_000)]
CEILING = 2.6214e13          # and+bcnt word pairs per second of the chip
REF_VARIANTS = 8192

result = {"what": "relationship(stat=REL_KING) over all samples and variants of a synthetic problem without missing data: ms per call, medians over reps; "
                  "and k_count_list_t over variant planes of the same row length (record path, matrix form, no survivors)",
          "reps": args.reps, "and_bcnt_ceiling_word_pairs_per_s": CEILING, "shapes": []}
eng = T.HipLd(0)
for idx in [int(x) for x in args.shapes.split(",") if x != ""]:
    name, N, M = SHAPES[idx]
    eng.set_problem(N, M)
    eng.generate_synthetic(42)
    words_live = (M + 31) // 32
    W = (words_live + 31) // 32 * 32
    out = eng.relationship(stat=T.REL_KING)          # warm-up, and a sanity check outside the clock
    assert out.shape == (N, N) and (np.diag(out) == 0.5).all() and abs(np.median(out)) < 0.05, name
    del out
    runs = []
    for _ in range(args.reps):
        eng.timing_reset()
        t0 = time.perf_counter()
        out = eng.relationship(stat=T.REL_KING)
        wall = (time.perf_counter() - t0) * 1e3
        tm, last = eng.timing(), eng.relationship_last()
        del out
        runs.append({"wall_ms": wall, "transpose_ms": last["transpose_ms"], "count_ms": tm["count_ms"], "epilogue_ms": tm["stats_ms"],
                     "count_launches": int(tm["count_launches"]), "row_pairs": int(tm["row_pairs"]), "planes_per_sample": last["planes_per_sample"],
                     "plane_bytes": int(last["plane_bytes"])})
    med = lambda k: float(np.median([r[k] for r in runs]))
    wps = runs[0]["row_pairs"] * words_live / (med("count_ms") * 1e-3)
    # the same kernel over variant planes of the same row length
    n_ref = W * 16
    eng.set_problem(n_ref, REF_VARIANTS)
    eng.generate_synthetic(43)
    eng.set_option("fused", 0)
    f = T.Filters(minR2=1.0)
    eng.ld_all(T.MODE_PHASED, f, collect=False)
    ref_runs = []
    for _ in range(args.reps):
        eng.timing_reset()
        eng.ld_all(T.MODE_PHASED, f, collect=False)
        tm = eng.timing()
        ref_runs.append({"count_ms": tm["count_ms"], "row_pairs": int(tm["row_pairs"]), "words_per_row": int(tm["words_per_row"]), "count_launches": int(tm["count_launches"])})
    eng.unset_option("fused")
    ref_ms = float(np.median([r["count_ms"] for r in ref_runs]))
    ref_wps = ref_runs[0]["row_pairs"] * ref_runs[0]["words_per_row"] / (ref_ms * 1e-3)
    shape = {"name": name, "n_samples": N, "n_variants": M, "plane_words": W, "plane_words_live": words_live, "sample_pairs": N * (N + 1) // 2,
             "runs": runs, "wall_ms_median": med("wall_ms"), "transpose_ms_median": med("transpose_ms"), "count_ms_median": med("count_ms"),
             "epilogue_ms_median": med("epilogue_ms"), "matrix_bytes": N * N * 8,
             "count_word_pairs_per_s": wps, "count_frac_of_ceiling": wps / CEILING,
             "variant_planes_same_row_length": {"n_samples": n_ref, "n_variants": REF_VARIANTS, "runs": ref_runs, "count_ms_median": ref_ms,
                                                "count_word_pairs_per_s": ref_wps, "count_frac_of_ceiling": ref_wps / CEILING},
             "relationship_over_variant_planes": wps / ref_wps}
    result["shapes"].append(shape)
    print(f"{name}: wall {shape['wall_ms_median']:.1f} ms = transpose {shape['transpose_ms_median']:.2f} + count {shape['count_ms_median']:.2f} "
          f"({runs[0]['count_launches']} launches) + epilogue {shape['epilogue_ms_median']:.2f} + copy of {N * N * 8 / 1e6:.0f} MB and the rest; "
          f"count {wps:.3e} word pairs/s ({100 * wps / CEILING:.1f} % of the ceiling) against {ref_wps:.3e} ({100 * ref_wps / CEILING:.1f} %) "
          f"over variant planes of {W} words: ratio {wps / ref_wps:.3f}", flush=True)
eng.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("written:", args.out)
