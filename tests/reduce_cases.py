"""What the test modules of the reduce kinds (score, prune, clump, matrix, decay, aggregate, their sequence) share: modes, data sets,
the oracle's records, the statistics and a few small helpers - one definition each.  A plain module: no fixtures, no tests."""
import functools

import numpy as np

import tomahawk_amd as T
from oracle import oracle as O
from tests import util

MODES = {"p": (T.MODE_PHASED, True, False), "u": (T.MODE_UNPHASED, False, True), "auto": (T.MODE_AUTO, False, False)}
RTOL = 1e-6
MOSAICS = {64: (5001, 4, 0.02, 0.002, False), 250: (5004, 7, 0.02, 0.002, False), 128: (5003, 6, 0.005, 0.0, True),
           1000: (5006, 3, 0.005, 0.0, False)}          # N -> seed, founders, switch, mut, miss (test_haplotype_block_data_all_modes)
FIELD = {T.STAT_R: "R", T.STAT_R2: "R2", T.STAT_D: "D", T.STAT_DPRIME: "Dprime"}
STATS = [T.STAT_R, T.STAT_R2, T.STAT_D, T.STAT_DPRIME]


# ---- the data sets ---------------------------------------------------------------------------------------------------------------------
def mosaic140(N):
    seed, founders, switch, mut, miss = MOSAICS[N]
    return util.mosaic_alleles(140, N, seed, n_founders=founders, switch=switch, mut=mut,
                               miss_rate=0.05 if miss else 0.0, miss_variants=0.3 if miss else 0.0)


def big_plain():
    return util.mosaic_alleles(700, 250, 5004, n_founders=7, switch=0.02, mut=0.002)


def big_missing():
    return util.mosaic_alleles(600, 128, 5003, n_founders=6, switch=0.005, mut=0.0, miss_rate=0.05, miss_variants=0.3)


# the sets of the walks (prune, clump) and of the sequence tests: real LD, more than one column block
DATA = {"mosaic250": lambda: mosaic140(250), "mosaic128": lambda: mosaic140(128), "mosaic64": lambda: mosaic140(64),
        "plain": big_plain, "missing": big_missing}
# the sets of the kinds that bin (decay, aggregate)
BINNED_DATA = {"random": lambda: util.random_alleles(300, 1000, seed=2024, low_ac=4),
               "missing": lambda: util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4),
               "mosaic64": lambda: mosaic140(64), "mosaic250": lambda: mosaic140(250), "mosaic128": lambda: mosaic140(128),
               "mosaic1000": lambda: mosaic140(1000)}


@functools.lru_cache(maxsize=None)
def data_set(name):
    al = DATA[name]()
    al.setflags(write=False)
    return al


@functools.lru_cache(maxsize=None)
def alleles(name):
    al = BINNED_DATA[name]()
    al.setflags(write=False)
    return al


def positions(M, pos=None, rid=None):
    pos = np.arange(M, dtype=np.int64) * 100 + 1000 if pos is None else np.asarray(pos, dtype=np.int64)
    rid = np.zeros(M, dtype=np.int64) if rid is None else np.asarray(rid, dtype=np.int64)
    return pos, rid


def standard_p(M):
    return 10.0 ** (-8.0 * np.random.default_rng(77).random(M))


def monotone(M, bins):
    return (np.arange(M, dtype=np.int64) * bins // M).astype(np.uint16)


def bins_monotone(M, X, Y):
    return monotone(M, X), monotone(M, Y)


def bins_every_seventh_random(M, X, Y, seed=12):
    rng = np.random.default_rng(seed)
    bx, by = bins_monotone(M, X, Y)
    sel = np.arange(M) % 7 == 3
    bx[sel] = rng.integers(0, X, int(sel.sum()))
    by[sel] = rng.integers(0, Y, int(sel.sum()))
    return bx, by


# ---- the oracle's records ----------------------------------------------------------------------------------------------------------------
def oracle_records(data, mask, variants, N, mode_key, minR2=0.0, window=None):
    """-> (idxA, idxB, records) of the oracle for the mode, each pair once (A < B in file order)."""
    _, ph, un = MODES[mode_key]
    want = O.all_pairs(data, mask, variants, N, O.settings(minR2=minR2, minP=1, phased=ph, unphased=un), vector_only=False)
    index = {(int(v["rid"]), int(v["pos"])): i for i, v in enumerate(variants)}
    ia = np.array([index[(int(r), int(p))] for r, p in zip(want["ridA"], want["Apos"])], dtype=np.int64)
    ib = np.array([index[(int(r), int(p))] for r, p in zip(want["ridB"], want["Bpos"])], dtype=np.int64)
    assert (ia < ib).all()
    if window is not None:
        pos, rid = variants["pos"].astype(np.int64), variants["rid"].astype(np.int64)
        keep = (rid[ia] == rid[ib]) & (np.abs(pos[ia] - pos[ib]) <= window)
        ia, ib, want = ia[keep], ib[keep], want[keep]
    return ia, ib, want


def stat_of(recs, stat):
    """The statistic of records, in float64: r carries D's sign."""
    return np.copysign(recs["R"], recs["D"]) if stat == T.STAT_R else recs[FIELD[stat]].astype(np.float64)


def margin_holds(r2, thr):
    return not (np.abs(r2 - thr) <= 1e-6 * thr).any()


def blob(result):
    """Everything a call returned, as bytes."""
    return b"".join(np.asarray(x).tobytes() for x in result)
