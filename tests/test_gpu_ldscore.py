"""LD scores (twk_hip_ld_score, `tomahawk ldscore`): per variant the number of records `calc` reports with the variant at either
end and the sum of their R2, reduced on the GPU.

"Oracle score": the records of oracle.all_pairs (the pinned restatement of the reference) with minP = 1, the window applied here
where one is set, R2 summed and records counted per variant over both ends.  The bar is the record path's own: a record's R2 is
held to 1e-6 relative plus, for records out of the unphased cubic, the record's own floor (tests/util.py cubic_floors with the
record's root error); a sum of non-negative terms inherits exactly that:

    |sum_r2(v) - want(v)| <= 1e-6 want(v) + sum over the cubic records of v of floor_R2(record)

and n(v) must be equal.  The data sets are ones on which existing tests show that engine and oracle report the same pair set
without double-root vetting (smoke(), test_records_with_missing, test_haplotype_block_data_all_modes).
"""
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import MODES, RTOL, mosaic140, oracle_records
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

def oracle_score(ia, ib, recs, M, root_error=None):
    """-> (n uint64[M], sum float64[M], floor float64[M]) from records: the definition, plus the floor term of the bar."""
    n = np.zeros(M, dtype=np.uint64)
    s = np.zeros(M, dtype=np.float64)
    fl = np.zeros(M, dtype=np.float64)
    np.add.at(n, ia, 1); np.add.at(n, ib, 1)
    np.add.at(s, ia, recs["R2"]); np.add.at(s, ib, recs["R2"])
    cubic = np.nonzero((recs["controller"] & 1) == 0)[0]
    for k in cubic:
        w = recs[k]
        total = float(np.sum(w["cnt"]))
        dx = util.D_FLOOR
        if root_error is not None and total > 0:
            dx = min(max(dx, util.ROOT_ERROR_FACTOR * root_error(int(ia[k]), int(ib[k]), float(w["cnt"][0]) / total)[0]), util.DX_CEILING)
        f = util.cubic_floors([float(x) for x in w["cnt"]], w["R"], dx)["R2"]
        fl[ia[k]] += f; fl[ib[k]] += f
    return n, s, fl


def assert_score(got_n, got_s, want_n, want_s, floor, what=""):
    bad_n = np.nonzero(got_n != want_n)[0]
    err = np.abs(got_s - want_s)
    bar = RTOL * want_s + floor
    worst = int(np.argmax(err - bar))
    print(f"{what}: records/variant {int(want_n.min())}..{int(want_n.max())}, score {want_s.min():.6g}..{want_s.max():.6g}, "
          f"largest |diff| {err.max():.3g} (variant {int(np.argmax(err))}), largest floor/score {float(np.max(floor / np.maximum(want_s, 1e-300))):.3g}, "
          f"closest to the bar: variant {worst} diff {err[worst]:.3g} bar {bar[worst]:.3g}")
    assert len(bad_n) == 0, f"{what}: n differs at {bad_n[:8].tolist()}: got {got_n[bad_n[:8]].tolist()} want {want_n[bad_n[:8]].tolist()}"
    assert (err <= bar).all(), f"{what}: sum beyond the bar at {np.nonzero(err > bar)[0][:8].tolist()}"


def check_against_oracle(hip, al, mode_key, minR2=0.0, window=None, what="", **score_kw):
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    ia, ib, want = oracle_records(data, mask, variants, N, mode_key, minR2, window)
    root_error = util.double_root_vetter(data, mask, variants, N).root_error
    wn, ws, fl = oracle_score(ia, ib, want, M, root_error)
    kw = dict(score_kw)
    if window is not None:
        kw.update(window=T.OPT_WINDOW, l_window=window)
    n, s, npairs = hip.ld_score(MODES[mode_key][0], T.Filters(minR2=minR2), **kw)
    assert n.dtype == np.uint64 and s.dtype == np.float64 and n.shape == s.shape == (M,)
    assert_score(n, s, wn, ws, fl, what or f"M={M} N={N} -{mode_key} minR2={minR2}")
    return n, s, npairs, len(want)


# ---- 1: iid data, the smoke() set ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_score_random_300x1000(hip, mode_key):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    n, s, npairs, nrec = check_against_oracle(hip, al, mode_key)
    assert npairs == 300 * 299 // 2 and int(n.sum()) == 2 * nrec and nrec > 44000


# ---- 2: missing genotypes: masked planes, the default mode's two passes over regrouped sets ------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_score_with_missing(hip, mode_key):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    check_against_oracle(hip, al, mode_key)


# ---- 3: real LD -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
@pytest.mark.parametrize("N", [64, 250, 128, 1000])
def test_score_haplotype_blocks(hip, N, mode_key):
    n, s, _, nrec = check_against_oracle(hip, mosaic140(N), mode_key)
    assert nrec > 1000 and s.max() > 1.0


# ---- 4: thresholds: tagging partners ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
@pytest.mark.parametrize("minR2", [0.2, 0.5, 0.8])
def test_score_threshold(hip, minR2, mode_key):
    al = mosaic140(1000)
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    # no record of the unthresholded run lies within 1e-6 relative of the cut-off: the pair set cannot depend on the last bits of r2
    _, _, all_recs = oracle_records(data, mask, variants, N, mode_key, 0.0)
    assert not (np.abs(all_recs["R2"] - minR2) <= 1e-6 * minR2).any()
    n, s, _, nrec = check_against_oracle(hip, al, mode_key, minR2=minR2)
    assert 0 < nrec == int((all_recs["R2"] >= minR2).sum())


# ---- 5: window ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_score_window(hip, mode_key):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    n, s, npairs, nrec = check_against_oracle(hip, al, mode_key, window=2000)
    assert int(n.max()) <= 40 and nrec < 300 * 21


# ---- 6: geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_score_small_tiles(hip, mode_key):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    hip.timing_reset()
    check_against_oracle(hip, al, mode_key, tile_variants=128)
    assert hip.timing()["count_launches"] >= 5          # diagonal and rectangular launches


@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_score_rectangle(hip, mode_key):
    al = util.random_alleles(300, 1000, seed=2024, low_ac=4)
    M, N, _ = al.shape
    data, mask, variants = util.upload(hip, al)
    ia, ib, want = oracle_records(data, mask, variants, N, mode_key)
    inside = (ia >= 50) & (ia < 150) & (ib >= 150) & (ib < 300)
    ia, ib, want = ia[inside], ib[inside], want[inside]
    wn, ws, fl = oracle_score(ia, ib, want, M, util.double_root_vetter(data, mask, variants, N).root_error)
    n, s, npairs = hip.ld_score(MODES[mode_key][0], T.Filters(minR2=0.0), a0=50, nA=100, b0=150, nB=150, triangle=False)
    assert npairs == 100 * 150
    assert_score(n, s, wn, ws, fl, f"rectangle -{mode_key}")
    assert not n[:50].any() and not s[:50].any() and (n[50:] > 0).all()


# ---- 7: shards --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u"])
def test_score_shards_add_up(hip, mode_key):
    al = mosaic140(250)
    M = al.shape[0]
    n1, s1, p1, _ = check_against_oracle(hip, al, mode_key)
    parts = [hip.ld_score(MODES[mode_key][0], T.Filters(minR2=0.0), part=k, n_parts=3) for k in range(3)]
    assert sum(p[2] for p in parts) == p1
    nsum = np.sum([p[0] for p in parts], axis=0, dtype=np.uint64)
    assert np.array_equal(nsum, n1)
    ssum = parts[0][1] + parts[1][1] + parts[2][1]
    assert (np.abs(ssum - s1) <= 2 * M * 2.0 ** -53 * s1).all()
    data, mask, variants = util.upload(hip, al)
    ia, ib, want = oracle_records(data, mask, variants, 250, mode_key)
    wn, ws, fl = oracle_score(ia, ib, want, M, util.double_root_vetter(data, mask, variants, 250).root_error)
    assert_score(nsum, ssum, wn, ws, fl, f"3 shards -{mode_key}")


def score_of_records(recs, M):
    n = np.zeros(M, dtype=np.uint64)
    s = np.zeros(M, dtype=np.float64)
    np.add.at(n, recs["idxA"], 1); np.add.at(n, recs["idxB"], 1)
    np.add.at(s, recs["idxA"], recs["R2"]); np.add.at(s, recs["idxB"], recs["R2"])
    return n, s


def assert_equals_record_path(hip, mode, M, what):
    recs, npairs, _ = hip.ld_all(mode, T.Filters(minR2=0.0))
    rn, rs = score_of_records(recs, M)
    n, s, sp = hip.ld_score(mode, T.Filters(minR2=0.0))
    err = np.abs(s - rs)
    print(f"{what}: {len(recs)} records, largest |score - sum over records| / score {float(np.max(err / np.maximum(rs, 1e-300))):.3g}")
    assert sp == npairs and np.array_equal(n, rn)
    assert (err <= 2 * M * 2.0 ** -53 * rs).all()


# ---- 8: long rows: the count kernel splits tiles along K, several launches ------------------------------------------------------------
def test_score_long_rows(hip):
    M, N = 1024, 100_003
    al = util.mosaic_alleles(M, N, seed=2, n_founders=5, switch=0.05, mut=0.01, miss_rate=0.01, miss_variants=0.3)
    hip.timing_reset()
    check_against_oracle(hip, al, "p", tile_variants=512)
    assert hip.timing()["count_launches"] >= 3
    for key in ("u", "auto"):
        assert_equals_record_path(hip, MODES[key][0], M, f"long rows -{key}")


# ---- 9: the record path's own sums, where the oracle would need the double-root vetter -----------------------------------------
@pytest.mark.parametrize("mode_key", ["p", "u", "auto"])
def test_score_equals_sums_over_own_records_on_hostile_data(hip, mode_key):
    al = util.extreme_alleles(70, 64, 901, miss=True)
    util.upload(hip, al)
    assert_equals_record_path(hip, MODES[mode_key][0], 70, f"hostile -{mode_key}")


# ---- 10: determinism ------------------------------------------------------------------------------------------------------------------
def test_score_runs_are_bit_identical(hip):
    util.upload(hip, mosaic140(250))
    a = hip.ld_score(T.MODE_UNPHASED, T.Filters(minR2=0.0))
    b = hip.ld_score(T.MODE_UNPHASED, T.Filters(minR2=0.0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1].max() > 1.0


# ---- 11: errors -----------------------------------------------------------------------------------------------------------------------
def test_score_refuses_a_fisher_cutoff_and_leaves_the_engine_usable(hip):
    al = util.random_alleles(120, 128, 31, miss_rate=0.08, miss_variants=0.3, low_ac=4)
    util.upload(hip, al)
    before, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    with pytest.raises(T.HipError) as ei:
        hip.ld_score(T.MODE_AUTO, T.Filters(minR2=0.0, minP=0.5))
    assert ei.value.code == -1          # TWK_HIP_E_INVALID
    after, _, _ = hip.ld_all(T.MODE_AUTO, T.Filters(minR2=0.0))
    assert len(before) > 1000 and before.tobytes() == after.tobytes()


# ---- 12: the command line -----------------------------------------------------------------------------------------------------------
def _ldscore_cli(twk, flags):
    r = subprocess.run([hostlib.CLI_PATH, "ldscore", "-i", twk] + list(flags), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head = [l for l in r.stdout.splitlines() if l.startswith("#")]
    rows = [l.split("\t") for l in r.stdout.splitlines() if l and not l.startswith("#")]
    assert head and head[-1].lstrip("#").split("\t") == ["contig", "pos", "n_partners", "sum_r2"]
    return head, rows


@pytest.mark.parametrize("flags,mode_key,window", [(["-p"], "p", None), (["-u", "-w", "3000"], "u", 3000)])
def test_ldscore_cli(hip, tmp_path, flags, mode_key, window):
    al = mosaic140(250)
    M, N, _ = al.shape
    rid = np.repeat([0, 1], [80, 60]).astype(np.uint32)
    pos = np.concatenate([np.arange(80) * 100 + 1000, np.arange(60) * 100 + 500]).astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    data, mask = O.bitvectors_from_alleles(al)
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    ia, ib, want = oracle_records(data, mask, variants, N, mode_key, 0.0, window)
    wn, ws, fl = oracle_score(ia, ib, want, M, util.double_root_vetter(data, mask, variants, N).root_error)
    head, rows = _ldscore_cli(twk, flags)
    assert len(rows) == M
    # contig / pos as `view` prints them for a record's A side: the contig's name, the 1-based position
    assert [r[0] for r in rows] == [str(int(x) + 1) for x in rid] and [int(r[1]) for r in rows] == [int(p) + 1 for p in pos]
    n = np.array([int(r[2]) for r in rows], dtype=np.uint64)
    s = np.array([float(r[3]) for r in rows], dtype=np.float64)
    assert_score(n, s, wn, ws, fl, "cli " + " ".join(flags))
    # the text round-trips: 17 significant digits
    assert all(repr(float(r[3])) == repr(float("%.17g" % float(r[3]))) for r in rows)
