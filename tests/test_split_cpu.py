"""LD splitting without a GPU: the NumPy restatement (tests/split_cases.py) against a brute-force enumeration of all partitions, the
restatement on a planted mosaic of independent blocks over the oracle's r2, and the host check of the kernels' index arithmetic."""
import itertools
import os
import re
import subprocess

import numpy as np

from oracle import oracle as O
from tests import split_cases as SC
from tests.reduce_cases import oracle_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_q(n, rng, kind):
    if kind == "zero":
        Q = np.zeros((n, n), dtype=np.int64)
    elif kind == "equal":
        Q = np.full((n, n), 5, dtype=np.int64)
    elif kind == "ties":
        Q = rng.integers(0, 3, (n, n)).astype(np.int64)             # few distinct values: many partitions tie
    else:
        Q = rng.integers(0, 1 << 32, (n, n)).astype(np.int64)
    if kind == "banded":
        Q[np.abs(np.subtract.outer(np.arange(n), np.arange(n))) > 3] = 0
    return np.triu(Q, 1)


def test_restatement_equals_brute_force():
    rng = np.random.default_rng(20211)
    cases = 0
    for n, kind in itertools.product((1, 2, 5, 8, 11, 12), ("zero", "equal", "ties", "random", "banded")):
        Q = random_q(n, rng, kind)
        for min_size in range(1, n + 1):
            for max_size in range(min_size, n + 1):
                got = SC.split_of_q(Q, min_size, max_size, n)
                assert got["total"] == int(Q.sum())
                for K in range(1, n + 1):
                    want = SC.brute_force(Q, min_size, max_size, K)
                    assert (want is not None) == bool(got["feasible"][K - 1]), (n, kind, min_size, max_size, K)
                    if want is None:
                        assert K not in got["K"] and got["cost"][K - 1] == 0
                        continue
                    gain, cuts = want
                    assert int(got["cost"][K - 1]) == got["total"] - gain, (n, kind, min_size, max_size, K)
                    assert list(got["cuts"][got["K"].index(K)]) == cuts, (n, kind, min_size, max_size, K, cuts)
                    cases += 1
    assert cases > 2000


def test_one_block_costs_nothing_and_single_variants_cost_everything():
    Q = random_q(9, np.random.default_rng(5), "random")
    got = SC.split_of_q(Q, 1, 9, 9)
    assert got["K"] == list(range(1, 10)) and got["cost"][0] == 0 and int(got["cost"][8]) == got["total"]
    assert (np.diff(got["cost"].astype(np.int64)) >= 0).all()


def test_restatement_recovers_the_planted_cuts_on_the_oracles_r2():
    al = SC.planted_alleles()
    M, N, _ = al.shape
    pos = np.arange(M, dtype=np.int64) * 100 + 1000
    variants = O.variants_from_alleles(al, pos=pos.astype(np.uint32))
    data, mask = O.bitvectors_from_alleles(al)
    p = SC.PLANTED
    ia, ib, recs = oracle_records(data, mask, variants, N, "p", 0.0, p["window"])
    first, indptr = SC.layout(pos, p["window"])
    values = SC.band_of_pairs(ia, ib, recs["R2"], first, indptr)
    got = SC.split_of(values, first, indptr, p["min_size"], p["max_size"], p["k_max"])
    K = len(SC.PLANTED_SIZES)
    assert K in got["K"]
    assert np.array_equal(got["cuts"][got["K"].index(K)], SC.planted_cuts()), got["cuts"][got["K"].index(K)]
    # every other K has to cut inside a planted block (K < 5: max_size forces it), so the planted K is the cheapest
    cost = got["cost"].astype(np.float64) / SC.SCALE
    print("planted mosaic: cost by K", np.round(cost, 2), "feasible", got["K"], "total", got["total"] / SC.SCALE)
    assert len(got["K"]) > 3 and all(got["cost"][K - 1] <= got["cost"][k - 1] for k in got["K"])


def test_make_split_check_passes():
    """Every lane of the prefix, block-sum, layer and backtrack index arithmetic (csrc/hip/ld_split_index.h) - LDS window bounds and
    saturation included - against a direct evaluation of the definition (csrc/tools/split_check.cpp), under ASan and UBSan."""
    r = subprocess.run(["make", "-C", ROOT, "split-check"], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"^split-check: (\d+) cases, (\d+) bad$", r.stdout, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, r.stdout[-500:]
