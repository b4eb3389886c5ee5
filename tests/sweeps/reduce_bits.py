"""The bytes the six reduce calls return, hashed: what two builds of the engine must agree on when a change claims to move no bit.
    python tests/sweeps/reduce_bits.py [--lib path/to/libtwk_hip.so] [--out bits.json]
--lib (or TWK_HIP_LIB) names the engine library to load in place of the tree's own: tomahawk_amd/hip.py honours no variable of its
own, but load_library() reads its module global LIB_PATH when the library is first loaded, and this script sets it before that.  The
Python side, the data, the calls and the host library (unused here) are this tree's either way, on purpose: only the engine differs.
Run it once per build and compare the two objects it prints: they must be equal.
Hashed, as SHA-256 of everything a call returns (tests/reduce_cases.py blob): ld_score, ld_prune, ld_clump, ld_matrix (all four
statistics), ld_decay (1, 500 and 4096 bins) and ld_aggregate (all four statistics, 50 x 31 bins, every seventh variant's bins random)
on the `plain` (700 x 250) and `missing` (600 x 128, regrouped in the default mode) sets of the reduce tests, in -p, -u and the default
mode, as one launch (tile_variants = 0) and as tiles of 128 variants.  Score's sums are doubles added in an order the kernel fixes:
this is the check that would notice a changed order.  Fails without a GPU."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import tomahawk_amd as T
import tomahawk_amd.hip

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.environ.get("TWK_HIP_LIB"))
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.lib:
    tomahawk_amd.hip.LIB_PATH = os.path.abspath(args.lib)      # (read when the library is first loaded: below)
if T.device_count() < 1:
    sys.exit("reduce_bits: no HIP device visible")

from tests import util
from tests.reduce_cases import MODES, STATS, FIELD, bins_every_seventh_random, blob, data_set, standard_p

RANGE_BP, X_BINS, Y_BINS = 50000, 50, 31
ALL, EDGES = T.Filters(minR2=0.0), T.Filters(minR2=0.2)

result = {}
for name in ("plain", "missing"):
    al = data_set(name)
    M = al.shape[0]
    p = standard_p(M)
    bx, by = bins_every_seventh_random(M, X_BINS, Y_BINS)
    with T.HipLd(0) as eng:
        util.upload(eng, al)
        for mode_key, (mode, _, _) in MODES.items():
            for tile in (0, 128):
                calls = {"score": lambda: eng.ld_score(mode, ALL, tile_variants=tile),
                         "prune": lambda: eng.ld_prune(mode, EDGES, tile_variants=tile),
                         "clump": lambda: eng.ld_clump(mode, EDGES, p, 1e-4, 1e-2, tile_variants=tile)}
                for stat in STATS:
                    calls[f"matrix {FIELD[stat]}"] = lambda stat=stat: eng.ld_matrix(mode, ALL, stat, -2.0, tile_variants=tile)
                    calls[f"aggregate {FIELD[stat]}"] = lambda stat=stat: eng.ld_aggregate(mode, ALL, bx, by, X_BINS, Y_BINS, stat, tile_variants=tile)
                for n_bins in (1, 500, 4096):
                    calls[f"decay {n_bins} bins"] = lambda n_bins=n_bins: eng.ld_decay(mode, ALL, RANGE_BP, n_bins, tile_variants=tile)
                for kind, call in calls.items():
                    result[f"{name} -{mode_key} tile={tile} {kind}"] = hashlib.sha256(blob(call())).hexdigest()
print(json.dumps(result, sort_keys=True))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
