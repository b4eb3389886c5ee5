"""What the reduce calls' shared host side owes their callers beyond each kind's own results (tests of the kinds: test_gpu_<kind>.py):
a call's report is its own, whichever epilogue its launches ran; nothing a call held or set reaches the next call, in any order of
kinds; and a call refused after its call object exists leaves nothing behind either.

One synthetic planted problem of 64 samples x 300 variants on one contig (the on-device generator: positions 1000 + 100 v, copies
five variants from their sources), a window of 2,000 base pairs - a band of up to 41 columns a row.  Equality is of bytes; nothing here
is compared with a tolerance."""
import numpy as np
import pytest

import tomahawk_amd as T
from tests.reduce_cases import bins_every_seventh_random, blob, standard_p

pytestmark = pytest.mark.gpu

N, M = 64, 300
WINDOW = 2000
MODE = T.MODE_PHASED
F = T.Filters(minR2=0.1)
MIN_SIZE, MAX_SIZE, K_MAX = 10, 40, 12
X_BINS, Y_BINS = 9, 7
HALF = M // 2          # test 3: the second half relabelled as a second contig


def planted(eng):
    eng.set_problem(N, M)
    eng.generate_synthetic(7, plant=T.Plant.near(M, 5))


def records(eng):
    return blob(eng.ld_region(MODE, F, 0, M, 0, M, True))


def split(eng, n=M):
    got = eng.ld_split(MODE, F, WINDOW, MIN_SIZE, MAX_SIZE, K_MAX, n=n)
    return (got["total"], got["feasible"], got["cost"], *got["cuts"], got["K"], got["n_records"], got["n_pairs"])


def split_bytes_closed_form(first, indptr, n, min_size, max_size, k_max):
    """What twk_hip_split_last reports as `bytes`, from the call's arguments and the band's layout: the band's floats and its map of 16
    bytes a row; the row prefixes (the widest row's upper entries, at most max_size - 1 and at least 1, times n), the block sums
    ((max_size - min_size + 1) x (n + 1)), two layers of n + 1, the rows' totals and the k_max + 1 gains, 8 bytes each; the layers'
    choices, 2 bytes each of k_max x (n + 1); the rows' upper counts, 4 bytes each; cost (8) and feasible (1) per K; the cuts, 4 bytes
    each of k_max x (k_max + 1); the total (8) and the broken-chain count (4)."""
    lens = (indptr[1:] - indptr[:-1]).astype(np.int64)
    upper = first.astype(np.int64) + lens - 1 - np.arange(n)
    widest = max(1, int(np.minimum(upper, max_size - 1).max()))
    cells, n1 = int(indptr[n]), n + 1
    return (cells * 4 + n * 16 + (widest * n + (max_size - min_size + 1) * n1 + 2 * n1 + n + k_max + 1) * 8 + k_max * n1 * 2 + n * 4
            + k_max * 9 + k_max * (k_max + 1) * 4 + 12)


# ---- 1: reports are per call -------------------------------------------------------------------------------------------------------------
def test_a_split_call_leaves_the_band_calls_report_alone():
    """ld_split's launches run the banded matrix's epilogue; twk_hip_bandmat_last still answers for the last ld_matrix_band call, and
    twk_hip_split_last for everything the split held."""
    with T.HipLd(0) as eng:
        planted(eng)
        values, first, indptr, nrec, _ = eng.ld_matrix_band(MODE, F, WINDOW, stat=T.STAT_R, fill=-2.0, a0=20, n=250)
        before = eng.bandmat_last()
        assert nrec > 0 and before["band_bytes"] == len(values) * 4 and before["copy_ms"] > 0
        got = eng.ld_split(MODE, F, WINDOW, MIN_SIZE, MAX_SIZE, K_MAX)
        assert got["n_records"] > 0 and len(got["K"]) > 0
        after = eng.bandmat_last()
        print(f"bandmat_last before {before}, behind ld_split {after}; split_last {eng.split_last()}")
        assert after == before and after["copy_ms"] == before["copy_ms"] and after["band_bytes"] == before["band_bytes"]
        first, indptr = eng.bandmat_layout(WINDOW)
        assert int((indptr[1:] - indptr[:-1]).max()) == 41
        last = eng.split_last()
        assert last["bytes"] == split_bytes_closed_form(first, indptr, M, MIN_SIZE, MAX_SIZE, K_MAX)
        assert last["band_ms"] > 0 and last["sums_ms"] > 0 and last["layers_ms"] > 0 and last["backtrack_ms"] > 0


# ---- 2: no state crosses calls -------------------------------------------------------------------------------------------------------------
def kinds(p, annot, bx, by):
    """Every reduce kind, each a call on `eng` -> everything it returns."""
    return [
        ("score", lambda eng: eng.ld_score(MODE, F)),
        ("score_annot", lambda eng: eng.ld_score_annot(MODE, F, annot)),
        ("prune", lambda eng: eng.ld_prune(MODE, F, window=T.OPT_WINDOW, l_window=WINDOW)),
        ("clump", lambda eng: eng.ld_clump(MODE, F, p, 1e-4, 1e-2)),
        ("matrix", lambda eng: eng.ld_matrix(MODE, F, T.STAT_R, -2.0)),
        ("decay", lambda eng: eng.ld_decay(MODE, F, 20000, 50)),
        ("aggregate", lambda eng: eng.ld_aggregate(MODE, F, bx, by, X_BINS, Y_BINS, T.STAT_R)),
        ("matrix_band", lambda eng: eng.ld_matrix_band(MODE, F, WINDOW, stat=T.STAT_DPRIME, fill=float("nan"))),
        ("topk", lambda eng: eng.ld_topk(MODE, F, 5, T.STAT_R2)),
        ("dprime_ci_band", lambda eng: eng.ld_dprime_ci_band(MODE, F, WINDOW)),
        ("blocks", lambda eng: eng.ld_blocks(MODE, F, WINDOW)),
        ("split", split),
        ("relationship", lambda eng: eng.relationship(T.REL_KING, want_counts=True)),
    ]


def run_in_order(eng, calls):
    """The calls in this order with ld_region's records before, between and after -> ({kind: bytes}, the three record arrays)."""
    out, recs = {}, [records(eng)]
    for k, (name, call) in enumerate(calls):
        if k == len(calls) // 2:
            recs.append(records(eng))
        out[name] = blob(call(eng))
    recs.append(records(eng))
    return out, recs


def test_every_kind_in_one_order_and_in_the_reverse_on_a_fresh_context():
    rng = np.random.default_rng(5)
    calls = kinds(standard_p(M), rng.standard_normal((M, 3)), *bins_every_seventh_random(M, X_BINS, Y_BINS))
    with T.HipLd(0) as eng:
        planted(eng)
        forward, recs_f = run_in_order(eng, calls)
    with T.HipLd(0) as eng:
        planted(eng)
        backward, recs_b = run_in_order(eng, calls[::-1])
    print({name: len(b) for name, b in forward.items()}, "records:", len(recs_f[0]) // T.RECORD_DTYPE.itemsize)
    assert len(recs_f[0]) > 100 * T.RECORD_DTYPE.itemsize
    for name, _ in calls:
        assert forward[name] == backward[name], f"{name} differs between the two orders"
    for k, r in enumerate(recs_f + recs_b):
        assert r == recs_f[0], f"record run {k} differs"


# ---- 3: a refused call leaves nothing behind -----------------------------------------------------------------------------------------------
def two_contigs(eng):
    """The planted problem with its second half on a second contig (positions as they are: sorted by (contig, position))."""
    planted(eng)
    data, _ = eng.download()
    meta = eng.meta()
    meta["rid"][HALF:] = 1
    eng.set_problem(N, M)
    eng.upload(data, meta)


def right_calls(eng):
    return {"matrix_band": blob(eng.ld_matrix_band(MODE, F, WINDOW, stat=T.STAT_R, fill=0.0)),
            "dprime_ci_band": blob(eng.ld_dprime_ci_band(MODE, F, WINDOW)),
            "split": blob(split(eng, n=HALF)), "records": records(eng)}


def test_refused_calls_leave_nothing_behind():
    """A capacity one short of the band is refused with E_INVALID when the call object exists and the band is laid out; so is a split
    across two contigs."""
    import ctypes as C
    with T.HipLd(0) as eng:
        two_contigs(eng)
        want = right_calls(eng)
    with T.HipLd(0) as eng:
        two_contigs(eng)
        first, indptr = eng.bandmat_layout(WINDOW)
        nnz = int(indptr[-1])
        f = F._c()
        got = {}
        # ld_matrix_band, its array one float short
        values, fi, ip = np.zeros(nnz, np.float32), np.zeros(M, np.uint32), np.zeros(M + 1, np.uint64)
        rc = eng._lib.twk_hip_ld_matrix_band(eng._ctx, MODE, C.byref(f), 0, M, 0, int(T.OPT_WINDOW), WINDOW, int(T.STAT_R), C.c_float(0.0),
                                             values.ctypes.data, nnz - 1, fi.ctypes.data, ip.ctypes.data, None, None)
        assert rc == -1 and not values.any() and not fi.any() and not ip.any()
        got["matrix_band"] = blob(eng.ld_matrix_band(MODE, F, WINDOW, stat=T.STAT_R, fill=0.0))
        assert records(eng) == want["records"]
        # ld_dprime_ci_band, its arrays one slot short
        lo, hi = np.zeros(nnz, np.uint8), np.zeros(nnz, np.uint8)
        rc = eng._lib.twk_hip_ld_dprime_ci_band(eng._ctx, MODE, C.byref(f), 0, M, 0, WINDOW, lo.ctypes.data, hi.ctypes.data, nnz - 1,
                                                fi.ctypes.data, ip.ctypes.data, None, None)
        assert rc == -1 and not lo.any() and not hi.any() and not fi.any() and not ip.any()
        got["dprime_ci_band"] = blob(eng.ld_dprime_ci_band(MODE, F, WINDOW))
        assert records(eng) == want["records"]
        # ld_split across the two contigs
        with pytest.raises(T.HipError) as ei:
            split(eng, n=M)
        assert ei.value.code == -1
        got["split"] = blob(split(eng, n=HALF))
        got["records"] = records(eng)
    for name in want:
        assert got[name] == want[name], f"{name} differs behind a refused call"
