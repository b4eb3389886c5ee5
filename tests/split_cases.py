"""LD splitting restated in NumPy, for tests/test_split_cpu.py, tests/test_gpu_split.py and tests/test_split_cli.py: the contract of
twk_hip_ld_split (include/twk_hip.h) over a band (values, first, indptr) as ld_matrix_band returns it - the weights q, the block sums
from a dense two-dimensional prefix sum, the recurrence with np.argmax over ascending d (the first maximum is the smallest d), the
backtracking - and a brute-force enumerator of all partitions for tiny n.  Nothing of the device's arrangement.
A plain module: no fixtures, no tests."""
import functools

import numpy as np

from tests import util

SCALE = 4294967296.0          # 2^32
INFEASIBLE = -1


def layout(pos, window):
    """The band layout of one contig's sorted positions for a window of `window` bases -> (first uint32[n], indptr uint64[n + 1])."""
    pos = np.asarray(pos, dtype=np.int64)
    first = np.searchsorted(pos, pos - window, side="left")
    end = np.searchsorted(pos, pos + window, side="right")
    return first.astype(np.uint32), np.concatenate([[0], np.cumsum(end - first)]).astype(np.uint64)


def band_of_pairs(ia, ib, r2, first, indptr, fill=0.0):
    """Pairs (ia < ib, relative to the slice) with their r2 -> the float32 band values, both orientations, diagonal 1."""
    values = np.full(int(indptr[-1]), fill, dtype=np.float32)
    first, ptr = first.astype(np.int64), indptr.astype(np.int64)
    r2 = np.asarray(r2, dtype=np.float64).astype(np.float32)
    values[ptr[ia] + ib - first[ia]] = r2
    values[ptr[ib] + ia - first[ib]] = r2
    n = len(first)
    values[ptr[:n] + np.arange(n) - first] = 1.0
    return values


def q_dense(values, first, indptr):
    """-> int64[n, n], strictly upper triangular: q(u, v) = rint(float64(B[u][v]) * 2^32) inside u's band, 0 outside.  (The product is
    exact in float64; rint rounds ties to even, as llrint does.)"""
    n = len(first)
    Q = np.zeros((n, n), dtype=np.int64)
    ptr = indptr.astype(np.int64)
    for u in range(n):
        f, row = int(first[u]), values[ptr[u]:ptr[u + 1]]
        up = row[u - f + 1:].astype(np.float64)
        Q[u, u + 1:u + 1 + len(up)] = np.rint(up * SCALE).astype(np.int64)
    return Q


def within_all(Q):
    """-> int64[n + 1, n + 1]: W[a, b] = the sum of Q[u, v] over a <= u < v < b, for a <= b."""
    n = Q.shape[0]
    P = np.zeros((n + 1, n + 1), dtype=np.int64)
    P[1:, 1:] = np.cumsum(np.cumsum(Q, axis=0), axis=1)
    dg = np.diagonal(P)
    return dg[None, :] - P - P.T + dg[:, None]


def split_of_q(Q, min_size, max_size, k_max):
    """The contract over a dense weight matrix -> {"total", "feasible" uint8[k_max], "cost" uint64[k_max] (0 where infeasible),
    "cuts": [uint32[K + 1] per feasible K], "K": the feasible K}."""
    n = Q.shape[0]
    W = within_all(Q)
    total = int(W[0, n])
    G = np.full(n + 1, INFEASIBLE, dtype=np.int64)
    G[0] = 0
    D = np.zeros((k_max + 1, n + 1), dtype=np.int64)
    gain = np.full(k_max + 1, INFEASIBLE, dtype=np.int64)
    for k in range(1, k_max + 1):
        new = np.full(n + 1, INFEASIBLE, dtype=np.int64)
        for b in range(k * min_size, min(n, k * max_size) + 1):
            d = np.arange(min_size, min(max_size, b) + 1)
            prev = G[b - d]
            cand = np.where(prev >= 0, prev + W[b - d, b], INFEASIBLE)
            at = int(np.argmax(cand))                         # the first maximum: the smallest d
            if cand[at] >= 0:
                new[b], D[k, b] = cand[at], d[at]
        G = new
        gain[k] = G[n]
    feasible = (gain[1:] >= 0).astype(np.uint8)
    cost = np.where(gain[1:] >= 0, total - gain[1:], 0).astype(np.uint64)
    cuts, ks = [], []
    for K in range(1, k_max + 1):
        if not feasible[K - 1]:
            continue
        c, b = [n], n
        for k in range(K, 0, -1):
            b -= int(D[k, b])
            c.append(b)
        assert b == 0
        cuts.append(np.array(c[::-1], dtype=np.uint32))
        ks.append(K)
    return {"total": total, "feasible": feasible, "cost": cost, "cuts": cuts, "K": ks}


def split_of(values, first, indptr, min_size, max_size, k_max):
    return split_of_q(q_dense(values, first, indptr), min_size, max_size, k_max)


def brute_force(Q, min_size, max_size, K):
    """All K-partitions of n = len(Q), the last block's size ascending, then the one before it, ..: the first strict maximum is the
    optimum whose size sequence, read from the last block, is lexicographically smallest.  -> (gain, cuts) or None."""
    n = Q.shape[0]
    W = within_all(Q)
    best = [None, None]

    def walk(k, b, gain, cuts):
        if k == 0:
            if b == 0 and (best[0] is None or gain > best[0]):
                best[0], best[1] = gain, cuts[::-1]
            return
        for d in range(min_size, min(max_size, b) + 1):
            if (k - 1) * min_size <= b - d <= (k - 1) * max_size:
                walk(k - 1, b - d, gain + int(W[b - d, b]), cuts + [b - d])

    walk(K, n, 0, [n])
    return None if best[0] is None else (best[0], best[1])


def assert_same(got, want, what=""):
    """A result of HipLd.ld_split against a restatement's, exactly."""
    assert got["total"] == want["total"], (what, got["total"], want["total"])
    assert got["K"] == want["K"] and np.array_equal(got["feasible"], want["feasible"]), (what, got["K"], want["K"])
    assert got["cost"].dtype == np.uint64 and np.array_equal(got["cost"], want["cost"]), (what, got["cost"], want["cost"])
    for K, a, b in zip(got["K"], got["cuts"], want["cuts"]):
        assert a.dtype == np.uint32 and np.array_equal(a, b), (what, K, a, b)


# ---- the planted mosaic: independent blocks, one after the other -----------------------------------------------------------------------
PLANTED_SIZES = (37, 52, 41, 60, 45)
PLANTED_N = 200
PLANTED_SEED = 7130
PLANTED = dict(min_size=20, max_size=80, k_max=8, window=10000)          # (positions 100 bases apart: +- 100 variants)


@functools.lru_cache(maxsize=None)
def planted_alleles():
    """Every block a mosaic of its own founders with its own seed: strong LD inside, sampling noise across."""
    parts = [util.mosaic_alleles(m, PLANTED_N, PLANTED_SEED + i, n_founders=8, switch=0.005, mut=0.0) for i, m in enumerate(PLANTED_SIZES)]
    al = np.ascontiguousarray(np.concatenate(parts, axis=0))
    al.setflags(write=False)
    return al


def planted_cuts():
    return np.concatenate([[0], np.cumsum(PLANTED_SIZES)]).astype(np.uint32)
