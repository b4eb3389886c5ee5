"""Haplotype blocks restated in NumPy, for tests/test_gpu_blocks.py and tests/test_blocks_cli.py: the D' confidence bounds of a 2 x 2
table, the bounds of a set of records scattered into band storage, and the blocks of a band by the contract of
twk_hip_ld_blocks - with dense n x n class matrices and two-dimensional prefix sums, nothing of the device's arrangement.
A plain module: no fixtures, no tests."""
import numpy as np

NONE = 255
CHUNK = 1 << 17
GAP = 1e-9         # the condition on the input: no running sum of any pair within this, relative, of its threshold
DEFAULTS = dict(strong_lo=70, strong_hi=98, recomb_hi=90, strong_lo_2=80, strong_lo_34=50, inform_permille=950, max_span_2=20000, max_span_3=30000)


def positions(M, seed=9):
    """The tests' positions: steps of 1 .. 399 base pairs, so that max_span_2 and max_span_3 can bind."""
    return 1000 + np.cumsum(np.random.default_rng(seed).integers(1, 400, M))


def bounds_of(cnt):
    """cnt float64[K, 4] = (n11, nX, nY, n22) -> (lo uint8[K], hi uint8[K], gap): the definition, row by row in float64; gap is the
    smallest relative distance of any running sum of any row from its threshold."""
    cnt = np.asarray(cnt, dtype=np.float64).reshape(-1, 4)
    if not len(cnt):
        return np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.inf
    if len(cnt) > CHUNK:          # (101 values a row: a slab at a time)
        parts = [bounds_of(cnt[k:k + CHUNK]) for k in range(0, len(cnt), CHUNK)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), min(p[2] for p in parts)
    n11, nX, nY, n22 = cnt.T
    neg = n11 * n22 < nX * nY
    m11, m12, m21, m22 = np.where(neg, nX, n11), np.where(neg, n11, nX), np.where(neg, n22, nY), np.where(neg, nY, n22)
    T = (m11 + m22) + (m12 + m21)
    pA, qA, pB, qB = (m11 + m12) / T, (m21 + m22) / T, (m11 + m21) / T, (m12 + m22) / T
    dmax = np.minimum(pA * qB, qA * pB)
    d = (np.arange(101) / 100.0)[None, :] * dmax[:, None]
    f11 = np.maximum((pA * pB)[:, None] + d, 1e-10)
    f22 = np.maximum((qA * qB)[:, None] + d, 1e-10)
    f12 = np.maximum((pA * qB)[:, None] - d, 1e-10)
    f21 = np.maximum((qA * pB)[:, None] - d, 1e-10)
    L = (m11[:, None] * np.log(f11) + m22[:, None] * np.log(f22)) + (m12[:, None] * np.log(f12) + m21[:, None] * np.log(f21))
    w = np.exp(L - L.max(axis=1, keepdims=True))
    up = np.cumsum(w, axis=1)                    # (cumsum adds in order: up[:, 100] is the total as the definition sums it)
    down = np.cumsum(w[:, ::-1], axis=1)
    thr = 0.05 * up[:, -1]
    i_up = np.argmax(up > thr[:, None], axis=1)
    i_down = 100 - np.argmax(down > thr[:, None], axis=1)
    gap = min(float((np.abs(up - thr[:, None]) / thr[:, None]).min()), float((np.abs(down - thr[:, None]) / thr[:, None]).min()))
    return np.maximum(i_up - 1, 0).astype(np.uint8), np.minimum(i_down + 1, 100).astype(np.uint8), gap


def band_of_records(recs, first, indptr, a0=0):
    """The records' bounds in band storage, both orientations, 255 elsewhere -> (lo, hi, gap).  Every record must lie in the band."""
    first, ptr = first.astype(np.int64), indptr.astype(np.int64)
    lo = np.full(int(ptr[-1]), NONE, dtype=np.uint8)
    hi = lo.copy()
    l, h, gap = bounds_of(recs["cnt"])
    u, v = recs["idxA"].astype(np.int64) - a0, recs["idxB"].astype(np.int64) - a0
    for x, y in ((u, v), (v, u)):
        k = y - first[x]
        assert ((k >= 0) & (k < ptr[x + 1] - ptr[x])).all(), "a record outside the band"
        lo[ptr[x] + k] = l
        hi[ptr[x] + k] = h
    return lo, hi, gap


def dense_of_band(values, first, indptr):
    n = len(first)
    ptr = indptr.astype(np.int64)
    lens = np.diff(ptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.arange(int(ptr[-1]), dtype=np.int64) - ptr[:-1][rows] + first.astype(np.int64)[rows]
    out = np.full((n, n), NONE, dtype=np.uint8)
    out[rows, cols] = values
    return out


def _inside(C):
    """C bool[n, n], upper triangle only -> f(i, j) = the number of set (x, y), i <= x < y <= j, for arrays i, j."""
    P = np.zeros((C.shape[0] + 1, C.shape[1] + 1), dtype=np.int64)
    P[1:, 1:] = C.astype(np.int64).cumsum(0).cumsum(1)
    return lambda i, j: P[j + 1, j + 1] - P[i, j + 1] - P[j + 1, i] + P[i, i]


def blocks_of(lo, hi, first, indptr, pos, **params):
    """The contract of twk_hip_ld_blocks over the slice's band -> dict(block_of (relative to the slice, -1: none), first, last,
    n_strong, n_recomb, n_candidates, n_informative)."""
    p = dict(DEFAULTS, **params)
    n = len(first)
    pos = np.asarray(pos, dtype=np.int64)
    LO, HI = dense_of_band(lo, first, indptr).astype(np.int64), dense_of_band(hi, first, indptr).astype(np.int64)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    inf = (LO != NONE) & upper
    strong = {cut: _inside(inf & (LO >= cut) & (HI >= p["strong_hi"])) for cut in {p["strong_lo"], p["strong_lo_2"], p["strong_lo_34"]}}
    recomb = _inside(inf & (HI < p["recomb_hi"]))
    i, j = np.nonzero(inf & (LO >= p["strong_lo"]) & (HI >= p["strong_hi"]))
    m, sep = j - i + 1, pos[j] - pos[i]
    assert (sep >= 0).all()
    cut = np.where(m == 2, p["strong_lo_2"], np.where(m <= 4, p["strong_lo_34"], p["strong_lo"]))
    s = np.zeros(len(i), dtype=np.int64)
    for c, f in strong.items():
        s = np.where(cut == c, f(i, j), s)
    r = recomb(i, j)
    ok = ~((m == 2) & (sep > p["max_span_2"])) & ~((m == 3) & (sep > p["max_span_3"]))
    ok &= s + r >= np.where(m == 2, 1, np.where(m == 3, 3, 6))
    ok &= s * 1000 > p["inform_permille"] * (s + r)
    i, j, m, sep, s, r = (x[ok] for x in (i, j, m, sep, s, r))
    order = np.lexsort((i, -m, -sep))
    block_of = np.full(n, -1, dtype=np.int64)
    found = []
    for k in order:
        a, b = int(i[k]), int(j[k])
        if block_of[a] >= 0 or block_of[b] >= 0:
            continue
        assert (block_of[a:b + 1] < 0).all(), "an interior variant of a new block lies in an earlier one"
        block_of[a:b + 1] = a
        found.append((a, b, int(s[k]), int(r[k])))
    found.sort()
    cols = [np.array([f[c] for f in found], dtype=np.int64) for c in range(4)]
    return dict(block_of=block_of, first=cols[0], last=cols[1], n_strong=cols[2], n_recomb=cols[3],
                n_candidates=int((inf & (LO >= p["strong_lo"]) & (HI >= p["strong_hi"])).sum()), n_informative=int(inf.sum()))
