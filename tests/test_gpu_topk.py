"""Top-k LD partners (twk_hip_ld_topk, `tomahawk ldscore --top`): for every variant the k partners with the largest |statistic| among
the records `calc` reports with the variant at either end, selected on the GPU.

"Restatement": from records (the engine's own, of ld_region with the same arguments, or the oracle's) in NumPy - the statistic in
float64, astype(float32), both ends of every record, ordered by (|value| descending, partner ascending), cut at k, padded with
(NO_PARTNER, +0.0).  Against the engine's own records the lists must be equal BYTE FOR BYTE: the same d_pair, one rounding.

Against the oracle the bar per entry is test_gpu_matrix's, derived there and not measured -
    bar(v, w) = 1e-6 |want| + floor + 2^-24 |want|
(the record path's own, the cubic's floor, float32's rounding) - and a list is held to what that bar can decide:
  - it has min(k, oracle partners) entries;
  - every listed partner is an oracle partner and its value lies within the bar of the oracle's;
  - no oracle partner that is not listed exceeds the weakest listed one (the oracle's value of it) by more than the two bars.
"""
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import FIELD, MODES, RTOL, STATS, blob, data_set, margin_holds, mosaic140, oracle_records, stat_of
from tests.test_gpu_matrix import oracle_matrix
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

F0 = dict(minR2=0.0)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def lists_of_pairs(a, b, values, M, k):
    """-> (idx uint32[M, k], val float32[M, k]) of the pairs (a[i], b[i]) with the float32 values[i]: both ends count."""
    owner = np.concatenate([a, b]).astype(np.int64)
    partner = np.concatenate([b, a]).astype(np.int64)
    v = np.concatenate([values, values]).astype(np.float32)
    order = np.lexsort((partner, -np.abs(v), owner))          # by owner, then |value| descending, then partner ascending
    owner, partner, v = owner[order], partner[order], v[order]
    rank = np.arange(len(owner)) - np.searchsorted(owner, np.arange(M))[owner] if len(owner) else np.zeros(0, dtype=np.int64)
    keep = rank < k
    idx = np.full((M, k), T.NO_PARTNER, dtype=np.uint32)
    val = np.zeros((M, k), dtype=np.float32)
    idx[owner[keep], rank[keep]] = partner[keep]
    val[owner[keep], rank[keep]] = v[keep]
    return idx, val


def lists_of_records(recs, M, k, stat):
    return lists_of_pairs(recs["idxA"], recs["idxB"], stat_of(recs, stat).astype(np.float32), M, k)


def assert_same_lists(got, want, what):
    gi, gv = got[0], got[1]
    wi, wv = want
    assert gi.dtype == np.uint32 and gv.dtype == np.float32 and gi.shape == gv.shape == wi.shape
    bad = np.argwhere((gi != wi) | (gv.view(np.uint32) != wv.view(np.uint32)))
    if len(bad):
        v = int(bad[0][0])
        print(f"{what}: variant {v}\n got  {gi[v].tolist()} {gv[v].tolist()}\n want {wi[v].tolist()} {wv[v].tolist()}")
    assert len(bad) == 0, f"{what}: {len(bad)} slots differ, first {bad[:4].tolist()}"


def whole(hip, mode, filters, **kw):
    M = hip.n_variants
    return hip.ld_region(mode, filters, 0, M, 0, M, True, **kw)


# ---- 1: the engine's own records, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minR2", [0.0, 0.5])
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("name", ["mosaic250", "plain", "missing"])
def test_topk_equals_own_records(hip, name, mode_key, minR2):
    al = data_set(name)
    M = al.shape[0]
    util.upload(hip, al)
    mode = MODES[mode_key][0]
    if minR2:
        # no record of the unthresholded run lies within 1e-6 relative of the cut-off: the pair set cannot depend on the last bits of r2
        all_recs, _, _ = whole(hip, mode, T.Filters(minR2=0.0))
        assert margin_holds(all_recs["R2"], minR2)
    recs, npairs, _ = whole(hip, mode, T.Filters(minR2=minR2))
    assert len(recs) > (1000 if not minR2 else 40)
    for stat in STATS:
        for k in (1, 3, 16, 32):
            got = hip.ld_topk(mode, T.Filters(minR2=minR2), k, stat=stat)
            assert got[2] == npairs == M * (M - 1) // 2
            assert_same_lists(got, lists_of_records(recs, M, k, stat), f"{name} -{mode_key} minR2={minR2} {FIELD[stat]} k={k}")
    last = hip.topk_last()
    assert last["list_bytes"] == M * 32 * 8 and last["unpack_ms"] > 0


# ---- 2: the oracle ---------------------------------------------------------------------------------------------------------------------
def assert_lists_against_oracle(idx, val, want, has, floor, k, what):
    M = want.shape[0]
    has = has & ~np.eye(M, dtype=bool)
    mag = np.abs(want)
    bar = RTOL * mag + floor + 2.0 ** -24 * mag
    used = idx != T.NO_PARTNER
    n_oracle = has.sum(axis=1)
    assert np.array_equal(used.sum(axis=1), np.minimum(k, n_oracle)), f"{what}: list lengths"
    assert (used[:, :-1] >= used[:, 1:]).all() and (val[~used].view(np.uint32) == 0).all(), f"{what}: padding"
    rows = np.repeat(np.arange(M), k).reshape(M, k)
    r, p = rows[used], idx[used].astype(np.int64)
    assert has[r, p].all(), f"{what}: a listed partner the oracle does not report"
    err = np.abs(val[used].astype(np.float64) - want[r, p])
    print(f"{what}: {int(used.sum())} listed, largest |diff| {err.max():.3g}, closest to the bar {float((err - bar[r, p]).max()):.3g}")
    assert (err <= bar[r, p]).all(), f"{what}: a listed value beyond the bar"
    listed = np.zeros((M, M), dtype=bool)
    listed[r, p] = True
    assert listed.sum() == used.sum(), f"{what}: a partner listed twice"
    full = np.nonzero(n_oracle > k)[0]                      # the variants with an oracle partner that is not listed
    weakest = idx[full, k - 1].astype(np.int64)
    limit = mag[full, weakest] + bar[full, weakest]
    out = has[full] & ~listed[full]
    over = out & (mag[full] - bar[full] > limit[:, None])
    assert not over.any(), f"{what}: an unlisted partner beats the weakest listed one, first (variant, partner) {np.argwhere(over)[:4].tolist()}"


ORACLE_SETS = {"mosaic64": lambda: mosaic140(64), "mosaic250": lambda: mosaic140(250), "mosaic128": lambda: mosaic140(128),
               "mosaic1000": lambda: mosaic140(1000), "random": lambda: util.random_alleles(300, 1000, seed=2024, low_ac=4)}


# (the modes in which existing tests compare the pair sets: test_gpu_matrix's cases 1 and 3)
@pytest.mark.parametrize("name,mode_key", [(n, m) for n in ORACLE_SETS for m in ("p", "u", "auto") if (n, m) != ("random", "auto")])
def test_topk_against_the_oracle(hip, name, mode_key):
    al = ORACLE_SETS[name]()
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    ia, ib, recs = oracle_records(data, mask, variants, N, mode_key)
    root_error = util.double_root_vetter(data, mask, variants, N).root_error
    for stat, k in ((T.STAT_R2, 16), (T.STAT_R, 5)):
        want, has, floor, _ = oracle_matrix(ia, ib, recs, M, stat, 0.0, root_error)
        idx, val, _ = hip.ld_topk(MODES[mode_key][0], T.Filters(**F0), k, stat=stat)
        assert_lists_against_oracle(idx, val, want, has, floor, k, f"{name} -{mode_key} {FIELD[stat]} k={k}")


# ---- 3: ties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_topk_ties_go_to_the_smaller_index(hip, mode_key):
    al = np.array(mosaic140(250))
    lo, hi = 40, 90
    al[lo:hi] = al[lo]                                        # 50 consecutive copies of one variant: r2 = 1 among them
    flat = al.reshape(al.shape[0], -1)
    others = np.r_[0:lo, hi:al.shape[0]]
    assert not ((flat[others] == flat[lo]).all(axis=1) | (flat[others] == 1 - flat[lo]).all(axis=1)).any()      # ... and with nobody else
    util.upload(hip, al)
    idx, val, _ = hip.ld_topk(MODES[mode_key][0], T.Filters(**F0), 16, stat=T.STAT_R2)
    for v in range(lo, hi):
        want = [w for w in range(lo, hi) if w != v][:16]
        assert idx[v].tolist() == want, (v, idx[v].tolist(), val[v].tolist())
        assert (val[v] == np.float32(1.0)).all(), (v, val[v].tolist())


# ---- 4: geometry and determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode_key", [("plain", "u"), ("missing", "auto")])
def test_topk_is_the_same_bytes_for_any_tiling_repeat_and_shard_split(hip, name, mode_key):
    al = data_set(name)
    util.upload(hip, al)
    mode, k = MODES[mode_key][0], 8
    first = hip.ld_topk(mode, T.Filters(**F0), k, stat=T.STAT_R)
    assert (first[0][:, k - 1] != T.NO_PARTNER).all()
    hip.timing_reset()
    for tile in (64, 256, 0):
        assert blob(hip.ld_topk(mode, T.Filters(**F0), k, stat=T.STAT_R, tile_variants=tile)) == blob(first), tile
    assert hip.timing()["count_launches"] >= 20
    assert blob(hip.ld_topk(mode, T.Filters(**F0), k, stat=T.STAT_R)) == blob(first)
    parts = [hip.ld_topk(mode, T.Filters(**F0), k, stat=T.STAT_R, part=p, n_parts=3) for p in range(3)]
    assert sum(p[2] for p in parts) == first[2]
    assert any(blob(p[:2]) != blob(first[:2]) for p in parts)
    merged = T.topk_merge([p[:2] for p in parts], k)
    assert_same_lists(merged, first[:2], f"{name}: 3 shards merged")


@pytest.mark.parametrize("mode_key", ["p", "auto"])
def test_topk_rectangle_lists_rows_and_columns(hip, mode_key):
    al = data_set("missing" if mode_key == "auto" else "plain")
    M = al.shape[0]
    util.upload(hip, al)
    mode = MODES[mode_key][0]
    recs, npairs, _ = hip.ld_region(mode, T.Filters(**F0), 0, 100, 100, 200, False)
    got = hip.ld_topk(mode, T.Filters(**F0), 8, stat=T.STAT_D, a0=0, nA=100, b0=100, nB=200, triangle=False)
    assert got[2] == npairs == 100 * 200
    assert_same_lists(got, lists_of_records(recs, M, 8, T.STAT_D), f"rectangle -{mode_key}")
    idx = got[0]
    assert (idx[:100, 0] >= 100).all() and (idx[:100, 0] < 300).all() and (idx[100:300, 0] < 100).all() and (idx[300:] == T.NO_PARTNER).all()


# ---- 5: window ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_topk_window(hip, mode_key):
    al = data_set("plain")
    M = al.shape[0]
    util.upload(hip, al)                                      # positions 100 apart
    mode = MODES[mode_key][0]
    kw = dict(window=T.OPT_WINDOW, l_window=2000)
    recs, _, _ = whole(hip, mode, T.Filters(**F0), **kw)
    assert 1000 < len(recs) <= M * 20
    idx, val, _ = got = hip.ld_topk(mode, T.Filters(**F0), 32, stat=T.STAT_R2, **kw)
    assert_same_lists(got, lists_of_records(recs, M, 32, T.STAT_R2), f"window -{mode_key}")
    used = idx != T.NO_PARTNER
    away = np.abs(idx.astype(np.int64) - np.arange(M)[:, None])[used]
    assert away.max() <= 20 and away.min() >= 1 and not used.all()


# ---- 6: the smallest shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(1, 4), (2, 4), (257, 4), (33, 4), (20, 32)])
def test_topk_smallest_shapes(hip, n, k):
    al = util.random_alleles(n, 64, seed=100 + n)
    util.upload(hip, al)
    for mode_key in ("p", "u"):
        mode = MODES[mode_key][0]
        got = hip.ld_topk(mode, T.Filters(**F0), k, stat=T.STAT_R)
        assert got[2] == n * (n - 1) // 2
        if n == 1:
            assert (got[0] == T.NO_PARTNER).all() and (got[1].view(np.uint32) == 0).all() and got[0].shape == (1, k)
            continue
        recs, _, _ = whole(hip, mode, T.Filters(**F0))
        assert_same_lists(got, lists_of_records(recs, n, k, T.STAT_R), f"n={n} k={k} -{mode_key}")
        if n == 20:
            assert (got[0][:, 19:] == T.NO_PARTNER).all() and (got[0][:, 0] != T.NO_PARTNER).any()


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------------
def test_topk_refuses_bad_arguments_and_leaves_the_engine_usable(hip):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    util.upload(hip, al)
    f = T.Filters(**F0)
    score = hip.ld_score(T.MODE_AUTO, f)
    recs = hip.ld_region(T.MODE_AUTO, f, 0, 120, 0, 120, True)
    top = hip.ld_topk(T.MODE_AUTO, f, 5)
    for kw in (dict(k=0), dict(k=33), dict(k=5, filters=T.Filters(minR2=0.0, minP=0.5)), dict(k=5, stat=7)):
        kw.setdefault("filters", f)
        with pytest.raises(T.HipError) as ei:
            hip.ld_topk(T.MODE_AUTO, **kw)
        assert ei.value.code == -1, kw          # TWK_HIP_E_INVALID
        assert blob(hip.ld_score(T.MODE_AUTO, f)) == blob(score)
        after = hip.ld_region(T.MODE_AUTO, f, 0, 120, 0, 120, True)
        assert after[0].tobytes() == recs[0].tobytes() and after[1:] == recs[1:] and len(recs[0]) > 1000
        # ... and the other way round: a score, a record call, then the lists
        assert blob(hip.ld_topk(T.MODE_AUTO, f, 5)) == blob(top)
    assert_same_lists(top, lists_of_records(recs[0], 120, 5, T.STAT_R2), "the default statistic is r2")


# ---- 8: the command line ---------------------------------------------------------------------------------------------------------------------
def _top_cli(twk, flags):
    r = subprocess.run([hostlib.CLI_PATH, "ldscore", "-i", twk, "--top", "5", "--top-stat", "r"] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head = [l for l in r.stdout.splitlines() if l.startswith("#")]
    rows = [l.split("\t") for l in r.stdout.splitlines() if l and not l.startswith("#")]
    assert head[-1].lstrip("#").split("\t") == ["contig", "pos", "rank", "partner_contig", "partner_pos", "value"]
    assert "##top=5" in head and "##stat=r" in head
    return head, rows, r.stderr


@pytest.mark.parametrize("flags", [["-p"], ["-u", "-c", "3", "-C", "2"]])
def test_ldscore_top_cli(hip, tmp_path, flags):
    import re
    al = mosaic140(250)
    M, N, _ = al.shape
    rid = np.repeat([0, 1], [80, 60]).astype(np.uint32)
    pos = np.concatenate([np.arange(80) * 100 + 1000, np.arange(60) * 100 + 500]).astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    head, rows, log = _top_cli(twk, flags)
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    util.upload(hip, al, variants)
    mode = T.MODE_PHASED if "-p" in flags else T.MODE_UNPHASED
    kw = {}
    selection = np.arange(M)
    if "-c" in flags:
        fl, tl, fr, tr = (int(x) for x in re.search(r"Using ranges \[(\d+)-(\d+),(\d+)-(\d+)\]", log).groups())
        starts = np.concatenate([[0], np.cumsum([50, 30, 50, 10])])          # blocks of 50 variants that end with their contig
        L = np.arange(starts[fl], starts[tl])
        R = np.arange(starts[fr], starts[tr])
        assert any(l.startswith("##shard=2/3") for l in head)
        if (fl, tl) == (fr, tr):
            kw, selection = dict(a0=int(L[0]), nA=len(L), b0=int(L[0]), nB=len(L), triangle=True), L
        else:
            kw, selection = dict(a0=int(L[0]), nA=len(L), b0=int(R[0]), nB=len(R), triangle=False), np.concatenate([L, R])
    else:
        assert not any(l.startswith("##shard") for l in head)
    idx, val, _ = hip.ld_topk(mode, T.Filters(**F0), 5, stat=T.STAT_R, **kw)
    want = []
    for v in selection:
        for r in range(5):
            if idx[v, r] == T.NO_PARTNER:
                break
            w = int(idx[v, r])
            want.append((str(int(rid[v]) + 1), int(pos[v]) + 1, r + 1, str(int(rid[w]) + 1), int(pos[w]) + 1, val[v, r]))
    assert len(rows) == len(want) > 5 * len(selection) - 5
    for got, w in zip(rows, want):
        assert (got[0], int(got[1]), int(got[2]), got[3], int(got[4])) == w[:5], (got, w)
        assert np.float32(float(got[5])).view(np.uint32) == np.float32(w[5]).view(np.uint32), (got, w)
