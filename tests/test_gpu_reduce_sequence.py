"""Score, prune, clump, matrix, decay and aggregate calls share one reduce path in the engine: one kind, one pair of argument buffers per
pipeline slot, one state block, one counters buffer.  What six separate sets of state gave for free is checked here: calls of different
kinds on ONE context, in any order and around failed calls, return what they return alone.

Both inputs run with tile_variants = 128, so that a call has more launches than the pipeline has slots: every slot's argument buffer
is then reused by kinds whose parameter blocks differ in size.  Equality is of bytes; nothing here is compared with a tolerance.
"""
import numpy as np
import pytest

import tomahawk_amd as T
from tests import util
from tests.reduce_cases import bins_every_seventh_random, blob, data_set, standard_p

pytestmark = pytest.mark.gpu

TILE = 128
F = dict(minR2=0.2)
KINDS = ("region", "score", "prune", "clump", "matrix", "decay", "aggregate")
A0, N_SUB = 37, 203
RANGE_BP, N_BINS = 50000, 500          # decay
X_BINS, Y_BINS = 50, 31                # aggregate, bins_every_seventh_random


def call(eng, kind, p, **kw):
    f = T.Filters(**F)
    if kind == "region":
        return eng.ld_all(T.MODE_AUTO, f, tile_variants=TILE)
    if kind == "score":
        return eng.ld_score(T.MODE_AUTO, f, tile_variants=TILE)
    if kind == "prune":
        return eng.ld_prune(T.MODE_AUTO, f, tile_variants=TILE, **kw)
    if kind == "clump":
        return eng.ld_clump(T.MODE_AUTO, f, p, 1e-4, 1e-2, tile_variants=TILE, **kw)
    if kind == "decay":
        return eng.ld_decay(T.MODE_AUTO, f, RANGE_BP, N_BINS, tile_variants=TILE)
    if kind == "aggregate":
        bx, by = bins_every_seventh_random(eng.n_variants, X_BINS, Y_BINS)
        return eng.ld_aggregate(T.MODE_AUTO, f, bx, by, X_BINS, Y_BINS, T.STAT_R, tile_variants=TILE)
    return eng.ld_matrix(T.MODE_AUTO, f, T.STAT_R, -2.0, tile_variants=TILE, **kw)


def bitmap_bytes(n):
    return n * ((n + 63) // 64) * 8


def lasts(eng):
    return eng.prune_last()["bitmap_bytes"], eng.clump_last()["bitmap_bytes"], eng.matrix_last()["matrix_bytes"]


@pytest.mark.parametrize("name", ["plain", "missing"])
def test_kinds_in_any_order_on_one_context(hip, name):
    al = data_set(name)
    M = al.shape[0]
    util.upload(hip, al)
    p = standard_p(M)

    # round 1: records, then every reduce kind; each call has more launches than there are pipeline slots
    first = {}
    for kind in KINDS:
        hip.timing_reset()
        first[kind] = blob(call(hip, kind, p))
        launches = hip.timing()["count_launches"]
        print(f"{name} M={M} {kind}: {launches} count launches, {len(first[kind])} bytes")
        assert launches >= 5, kind
    assert len(first["region"]) > 1000 * T.RECORD_DTYPE.itemsize
    # (prune, then clump and matrix behind it: each getter still answers for its own kind)
    assert lasts(hip) == (bitmap_bytes(M), bitmap_bytes(M), M * M * 4)

    # round 2: the other way round, ending with the records
    for kind in reversed(KINDS):
        assert blob(call(hip, kind, p)) == first[kind], f"{kind} differs in the reverse round"

    # one failed call of every reduce kind (minP < 1: TWK_HIP_E_INVALID) leaves nothing behind
    bad = T.Filters(minR2=0.2, minP=0.5)
    for failing in (lambda: hip.ld_score(T.MODE_AUTO, bad), lambda: hip.ld_prune(T.MODE_AUTO, bad),
                    lambda: hip.ld_clump(T.MODE_AUTO, bad, p), lambda: hip.ld_matrix(T.MODE_AUTO, bad),
                    lambda: hip.ld_decay(T.MODE_AUTO, bad, RANGE_BP, N_BINS),
                    lambda: hip.ld_aggregate(T.MODE_AUTO, bad, *bins_every_seventh_random(M, X_BINS, Y_BINS), X_BINS, Y_BINS, T.STAT_R)):
        with pytest.raises(T.HipError) as ei:
            failing()
        assert ei.value.code == -1
    assert lasts(hip) == (bitmap_bytes(M), bitmap_bytes(M), M * M * 4)
    for kind in KINDS:
        assert blob(call(hip, kind, p)) == first[kind], f"{kind} differs behind the failed calls"

    # a sub-range call behind a whole-range call of another kind is the sub-range call of a fresh context ...
    sub = dict(a0=A0, n=N_SUB)
    for whole, kind in (("clump", "prune"), ("matrix", "clump"), ("prune", "matrix")):
        assert blob(call(hip, whole, p)) == first[whole]
        got = blob(call(hip, kind, p, **sub))
        with T.HipLd(0) as fresh:
            util.upload(fresh, al)
            assert got == blob(call(fresh, kind, p, **sub)), f"sub-range {kind} behind a whole-range {whole}"
    # ... and each getter reports its own kind's last call, whatever ran behind it
    assert lasts(hip) == (bitmap_bytes(M), bitmap_bytes(N_SUB), N_SUB * N_SUB * 4)
    call(hip, "clump", p)
    assert lasts(hip) == (bitmap_bytes(M), bitmap_bytes(M), N_SUB * N_SUB * 4)
    call(hip, "prune", p, **sub)
    assert lasts(hip) == (bitmap_bytes(N_SUB), bitmap_bytes(M), N_SUB * N_SUB * 4)
