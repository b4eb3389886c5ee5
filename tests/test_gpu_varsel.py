"""Variant subsets (twk_hip_select_variants; `--extract` / `--exclude` / `--maf` / `--max-maf` / `--mac` / `--geno` / `--hwe`): LD over the
variants that pass a list and thresholds, selected on the GPU from the data that is already there, after the sample selection.

THE YARDSTICK IS THE ENGINE ITSELF FED THE SUBSET FROM THE HOST, as in tests/test_gpu_subset.py: a second context that received
alleles[kept] (or alleles[kept][:, keep]) with the kept variants' positions and Hardy-Weinberg P through tests/util.upload.  The
contract is that the two cannot be told apart, so equality is byte for byte everywhere and no parity exemption is used; one comparison
against the oracle ties the pair to the outside.  The thresholds are checked against a NumPy restatement of the header's formulas.
"""
import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5


@pytest.fixture(scope="module")
def other():
    """The context that is fed the subset from the host."""
    eng = T.HipLd(0)
    yield eng
    eng.close()


def state_of(eng):
    """Everything the contract names of a context's data: (counts, data words, mask words, marginals, metadata) as bytes."""
    data, mask = eng.download()
    return ((eng.n_samples, eng.n_variants), data.tobytes(), mask.tobytes(), tuple(m.tobytes() for m in eng.marginals()), eng.meta().tobytes())


def assert_same_state(got, want, what):
    for name, g, w in zip(("counts", "data", "mask", "marginals", "meta"), got, want):
        assert g == w, f"{what}: {name} differs"


def upload_rows(eng, al, kept, hwe=None, keep=None):
    """The host-fed context: rows `kept` of `al` (and samples `keep`) with the positions they have in `al` and the given hwe."""
    sub = al[kept] if keep is None else al[kept][:, keep]
    pos = (np.arange(al.shape[0]) * 100 + 1000)[kept]
    util.upload(eng, np.ascontiguousarray(sub), pos=pos, hwe=None if hwe is None else np.asarray(hwe)[kept])


def variant_lists(M, seed=5):
    """The lists of `make varsel-check` that fit M variants -> {name: ascending int64 indices}."""
    rng = np.random.default_rng(seed)
    out = {"everything": np.arange(M), "the first": np.array([0]), "the last": np.array([M - 1]), "every second": np.arange(0, M, 2)}
    if M >= 130:
        out["rows 0..127"] = np.arange(128)               # the row tile of the engine's padding is 128
        out["rows 127..129"] = np.arange(127, 130)
        out["the last 129"] = np.arange(M - 129, M)
    for density in (0.01, 0.5, 0.99):
        k = np.nonzero(rng.random(M) < density)[0]
        if len(k):
            out[f"random at {density}"] = k
    return out


DATA_SETS = {
    "140x96": lambda: util.random_alleles(140, 96, 11),
    "161x96-missing": lambda: util.random_alleles(161, 96, 12, miss_variants=0.3, miss_rate=0.2),
    "1000x70": lambda: util.random_alleles(1000, 70, 13),
    "5000x64": lambda: util.random_alleles(5000, 64, 14),
}


# ---- 1: bits, metadata and map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DATA_SETS))
def test_selected_bits_metadata_and_map_equal_an_upload_of_the_rows(hip, other, name):
    al = DATA_SETS[name]()
    M, N, _ = al.shape
    hwe = np.random.default_rng(7).choice([1e-5, 1e-3, 0.5, 1.0], size=M)
    util.upload(hip, al, hwe=hwe)
    base = state_of(hip)
    assert hip.variant_selection() == (M, M) and (hip.variant_map() == np.arange(M)).all()
    lists = variant_lists(M)
    want = None
    for what, ids in lists.items():
        for exclude in (False, True):
            kept = np.setdiff1d(np.arange(M), ids) if exclude else ids
            if len(kept) == 0:
                continue                                    # (a selection that keeps nothing is a refusal: test_refusals_change_nothing)
            n_kept = hip.select_variants(ids, exclude=exclude)
            assert n_kept == len(kept) and hip.variant_selection() == (M, len(kept)) and hip.n_variants == len(kept)
            assert (hip.variant_map() == kept).all(), f"{name}, {what}, exclude={exclude}: the map"
            upload_rows(other, al, kept, hwe)
            want = state_of(other)
            assert_same_state(state_of(hip), want, f"{name}, {what}, exclude={exclude}")
            last = hip.select_variants_last()
            assert last["select_ms"] > 0 and last["bytes_written"] > 0 and last["bytes_read"] > 0
    # (`want` is the last selection's, the complement of "random at 0.99": A then B equals B - B is taken from the base)
    hip.select_variants(lists["every second"])
    hip.select_variants(lists["random at 0.99"], exclude=True)
    assert_same_state(state_of(hip), want, f"{name}, A then B")
    assert hip.select_variants(None) == M
    assert hip.variant_selection() == (M, M) and hip.n_variants == M
    assert_same_state(state_of(hip), base, f"{name}, dropped")


def test_selection_beyond_one_scan_block_and_16_bit_indices(hip, other):
    """66,100 variants: more than any one block of the scan covers and than a 16-bit index holds; the state only."""
    al = util.random_alleles(66100, 40, 15)
    M = al.shape[0]
    util.upload(hip, al)
    rng = np.random.default_rng(16)
    for what, ids, exclude in (("random at 0.5", np.nonzero(rng.random(M) < 0.5)[0], False), ("the last 129", np.arange(M - 129, M), False),
                               ("every second, excluded", np.arange(0, M, 2), True)):
        kept = np.setdiff1d(np.arange(M), ids) if exclude else ids
        assert hip.select_variants(ids, exclude=exclude) == len(kept)
        assert (hip.variant_map() == kept).all(), what
        upload_rows(other, al, kept)
        assert_same_state(state_of(hip), state_of(other), what)
    hip.select_variants(None)
    assert hip.n_variants == M


# ---- 2: thresholds against a NumPy restatement ----------------------------------------------------------------------------------------------
def restated(eng, min_maf=0.0, max_maf=0.5, min_mac=0, max_missing=1.0, min_hwe=0.0):
    """The header's rule from what the base returns: one IEEE double multiplication and one comparison per threshold -> bool [M]."""
    _, het, hom, miss = eng.marginals()
    hwe = eng.meta()["hwe"]
    N = eng.n_samples
    called = N - miss.astype(np.int64)
    obs = 2 * called
    alt = het.astype(np.int64) + 2 * hom.astype(np.int64)
    minor = np.minimum(alt, obs - alt)
    return ((minor.astype(np.float64) >= np.float64(min_maf) * obs.astype(np.float64))
            & (minor.astype(np.float64) <= np.float64(max_maf) * obs.astype(np.float64))
            & (minor >= min_mac)
            & (miss.astype(np.float64) <= np.float64(max_missing) * np.float64(N))
            & ~(hwe < min_hwe))


def threshold_alleles():
    """300 x 96 with missing data; rows 0..7 carry one to four ALT alleles (low_ac), row 8 is all REF (monomorphic), rows 9 and 10 sit
    exactly on minor / obs = 0.25 (48 of 192 alleles; with four samples missing, 46 of 184)."""
    al = util.random_alleles(300, 96, 21, miss_variants=0.3, miss_rate=0.2, low_ac=8)
    al[8] = 0
    al[9] = 0
    al[9].reshape(-1)[:48] = 1
    al[10] = 0
    al[10, :4, :] = 2
    al[10].reshape(-1)[8:8 + 46] = 1
    return al


THRESHOLDS = [dict(min_maf=0.05), dict(min_maf=0.2), dict(max_maf=0.1), dict(min_mac=1), dict(max_missing=0.0), dict(max_missing=0.1),
              dict(min_hwe=1e-3), dict(min_maf=0.25), dict(max_maf=0.25), dict(min_maf=0.1, max_missing=0.1, min_hwe=1e-3, min_mac=30)]


def test_thresholds_equal_the_numpy_restatement(hip, other):
    al = threshold_alleles()
    M = al.shape[0]
    hwe = np.random.default_rng(22).choice([1e-5, 1e-3 * (1 - 2 ** -52), 1e-3, 0.5, 1.0], size=M)
    util.upload(hip, al)
    hip.set_hwe(hwe)                                            # values on both sides of 1e-3, and on it
    base = state_of(hip)
    for kw in THRESHOLDS:
        want = restated(hip, **kw)
        kept = np.nonzero(want)[0]
        assert 0 < len(kept) < M, kw                            # a filter that does nothing cannot pass
        assert hip.select_variants(**kw) == len(kept), kw
        assert (hip.variant_map() == kept).all(), kw
        if "min_maf" in kw and kw["min_maf"] == 0.25 or kw.get("max_maf") == 0.25:
            assert want[9] and want[10]                         # equality with the threshold keeps the variant
        if kw.get("min_mac") == 1:
            assert not want[8] and want[:8].all()               # the monomorphic row goes, the singletons stay
        upload_rows(other, al, kept, hwe)
        assert_same_state(state_of(hip), state_of(other), str(kw))
        hip.select_variants(None)
        assert_same_state(state_of(hip), base, f"{kw}, dropped")
    # a list and thresholds: the intersection; as an exclude list: the thresholds less the list
    ids = np.nonzero(np.random.default_rng(23).random(M) < 0.5)[0]
    listed = np.zeros(M, bool)
    listed[ids] = True
    for exclude in (False, True):
        want = restated(hip, min_maf=0.1, max_missing=0.1) & (listed != exclude)
        assert 0 < want.sum() < restated(hip, min_maf=0.1, max_missing=0.1).sum()
        assert hip.select_variants(ids, exclude=exclude, min_maf=0.1, max_missing=0.1) == want.sum()
        assert (hip.variant_map() == np.nonzero(want)[0]).all()
        hip.select_variants(None)


def test_thresholds_are_taken_on_the_kept_samples(hip, other):
    """Samples first, then the variants on the subset's own counts: the restatement is computed from the sample selection's working set."""
    al = util.random_alleles(200, 96, 24, miss_variants=0.3, miss_rate=0.2, low_ac=6)
    keep = np.sort(np.random.default_rng(25).choice(96, size=40, replace=False))
    util.upload(hip, al)
    whole = restated(hip, min_maf=0.2, max_missing=0.1)
    hip.select_samples(keep)
    after_samples = state_of(hip)
    want = restated(hip, min_maf=0.2, max_missing=0.1)
    assert (want != whole).any() and 0 < want.sum() < 200
    kept = np.nonzero(want)[0]
    assert hip.select_variants(min_maf=0.2, max_missing=0.1) == len(kept)
    assert hip.selection() == (96, 40) and hip.variant_selection() == (200, len(kept))
    upload_rows(other, al, kept, keep=keep)
    assert_same_state(state_of(hip), state_of(other), "samples, then variants")
    hip.select_variants(None)
    assert_same_state(state_of(hip), after_samples, "the variant selection dropped: the sample selection stands")
    assert hip.selection() == (96, 40)
    hip.select_samples(None)


# ---- 3: every consumer sees the working set -------------------------------------------------------------------------------------------------
def consumer_outputs(eng):
    """name -> bytes of one call each, on whatever the context holds; the per-variant inputs are sized by its variant count."""
    M = eng.n_variants
    rng = np.random.default_rng(9)
    out = {}
    for mode_key, mode in (("p", T.MODE_PHASED), ("u", T.MODE_UNPHASED), ("auto", T.MODE_AUTO)):
        for minR2 in (0.0, 0.2):
            recs, npairs, nrec = eng.ld_region(mode, T.Filters(minR2=minR2), 0, M, 0, M, True)
            assert npairs == M * (M - 1) // 2 and nrec == len(recs)
            out[f"ld_region -{mode_key} -r {minR2}"] = recs.tobytes()
    f0 = T.Filters(minR2=0.0)
    n, s, _ = eng.ld_score(T.MODE_AUTO, f0)
    out["ld_score"] = n.tobytes() + s.tobytes()
    n, s, _ = eng.ld_score_annot(T.MODE_AUTO, f0, rng.random((M, 2)))
    out["ld_score_annot"] = n.tobytes() + s.tobytes()
    out["ld_matrix"] = eng.ld_matrix(T.MODE_AUTO, f0, stat=T.STAT_R)[0].tobytes()
    values, first, indptr, _, _ = eng.ld_matrix_band(T.MODE_AUTO, f0, 2000)
    out["ld_matrix_band"] = values.tobytes() + first.tobytes() + indptr.tobytes()
    idx, val, _ = eng.ld_topk(T.MODE_AUTO, f0, 4)
    out["ld_topk"] = idx.tobytes() + val.tobytes()
    out["ld_prune"] = eng.ld_prune(T.MODE_AUTO, T.Filters(minR2=0.2))[0].tobytes()
    out["ld_clump"] = eng.ld_clump(T.MODE_AUTO, T.Filters(minR2=0.1), rng.random(M) ** 4, p1=0.05, p2=0.5)[0].tobytes()
    n, s, _ = eng.ld_decay(T.MODE_AUTO, f0, range_bp=20000, n_bins=50)
    out["ld_decay"] = n.tobytes() + s.tobytes()
    bins = (np.arange(M) * 8 // M).astype(np.uint16)
    out["ld_aggregate"] = b"".join(a.tobytes() for a in eng.ld_aggregate(T.MODE_AUTO, f0, bins, bins, 8, 8)[:5])
    out["relationship"] = eng.relationship(stat=T.REL_KING).tobytes()
    return out


CONSUMER_SETS = {
    "161x96-missing": lambda: util.random_alleles(161, 96, 12, miss_variants=0.3, miss_rate=0.2),
    "mosaic140": lambda: util.mosaic_alleles(140, 140, 21),
}
CALLS = [f"ld_region -{m} -r {r}" for m in ("p", "u", "auto") for r in (0.0, 0.2)] + [
    "ld_score", "ld_score_annot", "ld_matrix", "ld_matrix_band", "ld_topk", "ld_prune", "ld_clump", "ld_decay", "ld_aggregate", "relationship"]


@pytest.fixture(scope="module")
def consumer_pair(hip, other):
    """-> {data set: (outputs of the selected context, outputs of the host-fed one)}, computed once: half the samples, then min_maf = 0.1
    and a random exclude list."""
    out = {}
    for name, make in CONSUMER_SETS.items():
        al = make()
        M, N, _ = al.shape
        keep = np.sort(np.random.default_rng(3).choice(N, size=N // 2, replace=False))
        ids = np.nonzero(np.random.default_rng(4).random(M) < 0.2)[0]
        util.upload(hip, al)
        hip.select_samples(keep)
        n_kept = hip.select_variants(ids, exclude=True, min_maf=0.1)
        kept = hip.variant_map().astype(np.int64)
        assert 30 < n_kept < M - len(ids) + 1 and not np.isin(kept, ids).any()
        got = consumer_outputs(hip)
        hip.select_variants(None)
        hip.select_samples(None)
        upload_rows(other, al, kept, keep=keep)
        out[name] = (got, consumer_outputs(other))
    return out


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("name", list(CONSUMER_SETS))
def test_every_consumer_sees_the_working_set(consumer_pair, name, call):
    got, want = consumer_pair[name]
    # (iid genotypes of 48 samples may hold no pair at r2 >= 0.2: the mosaic's record arrays are not empty)
    assert len(want[call]) > 0 or (name != "mosaic140" and call.endswith("-r 0.2"))
    assert got[call] == want[call], f"{name}: {call} differs between the selection and the upload of the rows"


# ---- 4: missing data that leaves ------------------------------------------------------------------------------------------------------------
def test_missing_data_that_leaves_with_the_dropped_variants(hip, other):
    al = util.random_alleles(160, 90, 31, miss_variants=0.4, miss_rate=0.1)
    util.upload(hip, al)
    n_missing = int(hip.meta()["missing"].sum())
    assert 40 < n_missing < 90
    kept = np.nonzero(~(al == 2).any(axis=(1, 2)))[0]
    assert hip.select_variants(max_missing=0.0) == len(kept) == 160 - n_missing
    meta = hip.meta()
    assert not meta["missing"].any() and not meta["an"].any()
    assert not hip.download()[1].any()
    K = len(kept)
    got, _, _ = hip.ld_region(T.MODE_AUTO, T.Filters(minR2=0.0), 0, K, 0, K, True)
    hip.select_variants(None)
    assert hip.meta()["missing"].sum() == n_missing and hip.download()[1].any()
    upload_rows(other, al, kept)
    want, _, _ = other.ld_region(T.MODE_PHASED, T.Filters(minR2=0.0), 0, K, 0, K, True)
    assert len(want) > 1000 and got.tobytes() == want.tobytes()


# ---- 5: against the oracle, once ------------------------------------------------------------------------------------------------------------
def test_selected_records_match_the_oracle(hip):
    al = util.random_alleles(160, 100, 41)
    util.upload(hip, al)
    n_kept = hip.select_variants(np.arange(0, 160, 3), exclude=True, min_maf=0.1)
    kept = hip.variant_map().astype(np.int64)
    assert 60 <= n_kept < 107
    got, npairs, _ = hip.ld_region(T.MODE_PHASED, T.Filters(minR2=0.0), 0, n_kept, 0, n_kept, True)
    hip.select_variants(None)
    sub = np.ascontiguousarray(al[kept])
    data, mask = O.bitvectors_from_alleles(sub)
    variants = O.variants_from_alleles(sub, pos=(np.arange(160) * 100 + 1000)[kept])
    want = O.all_pairs(data, mask, variants, 100, O.settings(minR2=0.0, phased=True), vector_only=True)
    assert npairs == n_kept * (n_kept - 1) // 2 and len(want) > 1000
    util._LAST_UPLOAD.update(data=data, mask=mask, variants=variants, n_samples=100, vet=None)
    util.assert_records_match(got, want, variants, n_samples=100)


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(hip):
    al = util.random_alleles(90, 40, 51, miss_variants=0.3, miss_rate=0.1)
    data, mask, variants = util.upload(hip, al)
    lib, ctx = hip._lib, hip._ctx
    ids = np.arange(3, dtype=np.uint32)
    with T.HipLd(0) as fresh:                                   # before an upload: TWK_HIP_E_STATE
        assert lib.twk_hip_select_variants(fresh._ctx, None, ids.ctypes.data, 3, 0, None) == E_STATE
        assert b"twk_hip_select_variants" in lib.twk_hip_last_error(fresh._ctx)          # says what and where
        fresh.set_problem(40, 90)
        assert lib.twk_hip_select_variants(fresh._ctx, None, ids.ctypes.data, 3, 0, None) == E_STATE
        assert b"nothing was uploaded" in lib.twk_hip_last_error(fresh._ctx)
    first = np.arange(5, 80, 2)
    hip.select_variants(first, min_maf=0.05)
    n_active = hip.n_variants
    before = state_of(hip)
    map_before = hip.variant_map()

    def refused(**kw):
        with pytest.raises(T.HipError) as ei:
            hip.select_variants(**kw)
        assert ei.value.code == E_INVALID, kw
        assert str(ei.value) and lib.twk_hip_last_error(ctx)
        assert hip.variant_selection() == (90, n_active) and hip.n_variants == n_active, kw
        return str(ei.value)

    for bad in ([3, 2, 7], [3, 3, 7], [0, 5, 90], [1, 4, 2 ** 32 - 1]):
        refused(list=bad)
    assert "list[2]" in refused(list=[0, 5, 90])                # the position is named
    assert lib.twk_hip_select_variants(ctx, None, None, 3, 0, None) == E_INVALID          # NULL with a count
    assert b"count of 3" in lib.twk_hip_last_error(ctx)
    assert hip.variant_selection() == (90, n_active)
    nan = float("nan")
    for kw in (dict(min_maf=-0.1), dict(min_maf=0.6), dict(max_maf=0.6), dict(max_maf=-1.0), dict(min_maf=0.3, max_maf=0.2), dict(max_missing=1.5),
               dict(max_missing=-0.1), dict(min_hwe=1.5), dict(min_hwe=-0.1), dict(min_maf=nan), dict(max_maf=nan), dict(max_missing=nan), dict(min_hwe=nan)):
        refused(**kw)
    refused(list=[])                                            # an empty keep list keeps no variant
    refused(list=np.arange(90), exclude=True)                   # and so does excluding everything
    refused(min_mac=10 ** 6)
    with pytest.raises(TypeError):
        hip.select_variants([0.5, 1.5])
    assert (hip.variant_map() == map_before).all()
    assert_same_state(state_of(hip), before, "after the refusals")
    # select_samples, an upload and the generator while a variant selection is active: TWK_HIP_E_STATE, and the selection stands
    for call in (lambda: hip.select_samples([0, 1, 2]), lambda: hip.select_samples(None), lambda: hip.upload(data, util.to_hip_meta(variants), mask),
                 lambda: hip.generate_synthetic(1)):
        with pytest.raises(T.HipError) as ei:
            call()
        assert ei.value.code == E_STATE and "a variant selection is active" in str(ei.value)          # the cause is named
    assert hip.variant_selection() == (90, n_active) and hip.selection() == (40, 40)
    assert len(hip.variant_map(first=n_active)) == 0 and (hip.variant_map(first=n_active - 2) == map_before[-2:]).all()
    assert_same_state(state_of(hip), before, "after the refused calls")
    # set_hwe writes the working set only: the next selection and the drop bring the base's values back
    hip.set_hwe(np.full(n_active, 0.25))
    assert (hip.meta()["hwe"] == 0.25).all()
    hip.select_variants(first, min_maf=0.05)
    assert (hip.meta()["hwe"] == 1.0).all()
    hip.set_hwe([0.5, 0.5], first=3)
    hip.select_variants(None)
    assert (hip.meta()["hwe"] == 1.0).all() and hip.n_variants == 90
    # set_problem clears everything
    hip.select_variants(first)
    hip.set_problem(40, 90)
    assert hip.variant_selection() == (90, 90)
    hip.upload(data, util.to_hip_meta(variants), mask)          # (no selection is active any more)
    assert hip.download()[0].tobytes() == data.tobytes()


# ---- 7: the commands, end to end ------------------------------------------------------------------------------------------------------------
import subprocess                                                # noqa: E402

from tomahawk_amd import hostlib                                 # noqa: E402


def restated_from_alleles(al, min_maf=0.0, max_maf=0.5, min_mac=0, max_missing=1.0):
    """The header's rule from the genotypes themselves (no engine in it) -> bool [M]."""
    N = al.shape[1]
    missing = (al == 2).any(axis=2)
    alt = np.where(missing, 0, al.sum(axis=2)).sum(axis=1).astype(np.int64)
    miss = missing.sum(axis=1).astype(np.int64)
    obs = 2 * (N - miss)
    minor = np.minimum(alt, obs - alt)
    return ((minor.astype(np.float64) >= np.float64(min_maf) * obs.astype(np.float64)) & (minor.astype(np.float64) <= np.float64(max_maf) * obs.astype(np.float64))
            & (minor >= min_mac) & (miss.astype(np.float64) <= np.float64(max_missing) * np.float64(N)))


def subset_hwe(al):
    """The importer's Hardy-Weinberg P of every variant of `al`, over its complete genotypes: what a re-import of these samples carries."""
    complete = (al != 2).all(axis=2)
    alt = np.where(complete, al.sum(axis=2), -1)
    return np.array([hostlib.hwe_exact(int((a == 0).sum()), int((a == 1).sum()), int((a == 2).sum())) for a in alt])


def write_list(path, pos, ids, junk=False):
    """A variant list of the positions of `ids` as the commands print them: CONTIG:POS lines and CONTIG<TAB>POS lines with further columns."""
    with open(path, "w") as fh:
        fh.write("# a list\n\n")
        for k, v in enumerate(ids):
            fh.write(f"1:{int(pos[v]) + 1}\n" if k % 2 else f"1\t{int(pos[v]) + 1}\t0.5\tmore\n")
        if junk:
            fh.write("1:7\n9\t1001\n")                           # a position and a contig the input does not have: counted, no error


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    """A .twk of 150 variants x 90 samples, list files and thresholds that select `kept` of them, the .twk of the kept rows; the same after
    a --keep of 37 samples (thresholds on the subset's counts, the kept rows written with the subset's own Hardy-Weinberg P)."""
    d = tmp_path_factory.mktemp("varsel_cli")
    al = util.mosaic_alleles(150, 90, 61, miss_variants=0.2, miss_rate=0.15)
    M, N, _ = al.shape
    pos, rid = (1000 + 100 * np.arange(M)).astype(np.uint32), np.zeros(M, np.uint32)
    rng = np.random.default_rng(63)
    extract = np.nonzero(rng.random(M) < 0.8)[0]
    exclude = np.nonzero(rng.random(M) < 0.1)[0]
    listed = np.zeros(M, bool)
    listed[extract] = True
    listed[exclude] = False
    thresholds = dict(min_maf=0.1, min_mac=20, max_missing=0.1)
    flags = ["--maf", "0.1", "--mac", "20", "--geno", "0.1"]
    out = dict(dir=d, al=al, pos=pos, flags=flags, full=str(d / "full.twk"), extract=str(d / "extract.txt"), exclude=str(d / "exclude.txt"))
    hostlib.write_twk(out["full"], al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=1, block_size=40)
    write_list(out["extract"], pos, extract[::-1], junk=True)    # (any order: file order comes out)
    write_list(out["exclude"], pos, exclude)
    kept = np.nonzero(listed & restated_from_alleles(al, **thresholds))[0]
    assert 40 < len(kept) < listed.sum()
    out["kept"], out["kept_twk"] = kept, str(d / "kept.twk")
    hostlib.write_twk(out["kept_twk"], np.ascontiguousarray(al[kept]), pos[kept], rid[kept], phased=np.ones(len(kept), np.uint8), n_contigs=1, block_size=40)
    # ... and with a sample list
    keep = np.sort(np.random.default_rng(62).choice(N, size=37, replace=False))
    sub = np.ascontiguousarray(al[:, keep])
    kept_s = np.nonzero(listed & restated_from_alleles(sub, **thresholds))[0]
    assert 30 < len(kept_s) < listed.sum() and set(kept_s) != set(kept)
    out["keep_file"], out["kept_s"], out["kept_s_twk"] = str(d / "keep.txt"), kept_s, str(d / "kept_s.twk")
    with open(out["keep_file"], "w") as fh:
        fh.write("".join(f"S{s}\n" for s in keep))
    hostlib.write_twk(out["kept_s_twk"], np.ascontiguousarray(sub[kept_s]), pos[kept_s], rid[kept_s], phased=np.ones(len(kept_s), np.uint8), n_contigs=1, block_size=40,
                      hwe=subset_hwe(sub[kept_s]))
    assoc = str(d / "assoc.txt")
    with open(assoc, "w") as fh:
        fh.write("#contig\tpos\tP\n" + "".join(f"1\t{int(pos[v]) + 1}\t{float(p)!r}\n" for v, p in enumerate(np.random.default_rng(64).random(M) ** 6)))
    out["assoc"] = assoc
    return out


def run_cli(*args):
    r = subprocess.run([hostlib.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def body(text):
    """The lines of a command's text output without the two that differ from run to run by design (`##tomahawk_<name>Version=`,
    `##tomahawk_<name>Command=..; Date=..`)."""
    return [l for l in text.splitlines() if not l.startswith("##tomahawk_")]


def selections(f):
    """(what, the options that select, the file of the kept rows, the number kept) without and with the sample list."""
    sel = ["--extract", f["extract"], "--exclude", f["exclude"]] + f["flags"]
    return [("variants", sel, f["kept_twk"], len(f["kept"])), ("samples and variants", sel + ["--keep", f["keep_file"]], f["kept_s_twk"], len(f["kept_s"]))]


@pytest.mark.parametrize("cmd", [["ldscore", "-r", "0"], ["clump", "-r", "0.2", "--p1", "0.05", "--p2", "0.5"], ["prune", "-r", "0.3"],
                                 ["lddecay", "-r", "0", "-d", "20000", "-b", "40"]], ids=lambda c: c[0])
def test_cli_text_commands_equal_the_run_on_the_file_of_kept_variants(cli_files, cmd):
    f = cli_files
    extra = ["-a", f["assoc"]] if cmd[0] == "clump" else []
    for what, sel, kept_twk, n_kept in selections(f):
        want = body(run_cli(cmd[0], "-i", kept_twk, *cmd[1:], *extra).stdout)
        r = run_cli(cmd[0], "-i", f["full"], *cmd[1:], *extra, *sel)
        assert len(want) > 10 and body(r.stdout) == want, (cmd, what)
        assert f"Keeping {n_kept} of 150 variants" in r.stderr
        assert "2 listed positions are not among the loaded variants" in r.stderr


def test_cli_calc_equals_calc_of_the_file_of_kept_variants(cli_files):
    f = cli_files
    for k, (what, sel, kept_twk, n_kept) in enumerate(selections(f)):
        a, b = str(f["dir"] / f"calc_kept{k}.two"), str(f["dir"] / f"calc_sel{k}.two")
        run_cli("calc", "-i", kept_twk, "-o", a, "-r", "0.05")
        r = run_cli("calc", "-i", f["full"], "-o", b, "-r", "0.05", *sel)
        assert f"Keeping {n_kept} of 150 variants" in r.stderr
        va, vb = run_cli("view", "-i", a, "-H").stdout, run_cli("view", "-i", b, "-H").stdout
        assert len(va.splitlines()) > 500 and va == vb, what          # positions, flags, counts, statistics: every column of every record
        assert hostlib.read_two(a)[0].tobytes() == hostlib.read_two(b)[0].tobytes()


def test_cli_ldmatrix_and_relationship_equal_the_run_on_the_file_of_kept_variants(cli_files):
    f = cli_files
    for k, (what, sel, kept_twk, n_kept) in enumerate(selections(f)):
        for cmd in (["ldmatrix", "-r", "0"], ["relationship"]):
            a, b = str(f["dir"] / f"{cmd[0]}_kept{k}"), str(f["dir"] / f"{cmd[0]}_sel{k}")
            run_cli(*cmd, "-i", kept_twk, "-o", a)
            run_cli(*cmd, "-i", f["full"], "-o", b, *sel)
            ma, mb = np.load(a + ".npy"), np.load(b + ".npy")
            assert ma.shape == mb.shape and ma.tobytes() == mb.tobytes(), (cmd, what)
            if cmd[0] == "ldmatrix":
                assert ma.shape == (n_kept, n_kept) and open(a + ".variants.tsv").read() == open(b + ".variants.tsv").read()


def test_cli_prune_then_extract(cli_files):
    """PLINK's two-step: `prune --kept-only` writes a list that --extract reads back."""
    f = cli_files
    al, pos = f["al"], f["pos"]
    keep_tsv = str(f["dir"] / "prune_keep.tsv")
    run_cli("prune", "-i", f["full"], "-r", "0.3", "--kept-only", "-o", keep_tsv)
    rows = [l.split("\t") for l in open(keep_tsv).read().splitlines() if not l.startswith("#")]
    flags = [l.split("\t")[2] for l in body(run_cli("prune", "-i", f["full"], "-r", "0.3").stdout) if not l.startswith("#")]
    kept = np.nonzero(np.array(flags) == "1")[0]
    assert 10 < len(kept) < 150 and [int(r[1]) for r in rows] == [int(pos[v]) + 1 for v in kept] and all(r[2] == "1" for r in rows)
    pruned_twk = str(f["dir"] / "pruned.twk")
    hostlib.write_twk(pruned_twk, np.ascontiguousarray(al[kept]), pos[kept], np.zeros(len(kept), np.uint32), phased=np.ones(len(kept), np.uint8), n_contigs=1, block_size=40)
    want = body(run_cli("ldscore", "-i", pruned_twk, "-r", "0").stdout)
    r = run_cli("ldscore", "-i", f["full"], "-r", "0", "--extract", keep_tsv)
    assert len(want) > len(kept) and body(r.stdout) == want
    assert f"Keeping {len(kept)} of 150 variants" in r.stderr


def test_cli_other_commands_take_the_options_and_bad_ones_are_refused(cli_files):
    f = cli_files
    sel = ["--extract", f["extract"], "--max-maf", "0.45", "--hwe", "1e-6"]
    run_cli("ldaggregate", "-i", f["full"], "-r", "0", "-x", "4", "-y", "4", "-m", "0", *sel)
    r = run_cli("scalc", "-i", f["full"], "-I", f"1:{int(f['pos'][70]) + 1}-{int(f['pos'][70]) + 1}", "-o", str(f["dir"] / "scalc.two"), "--geno", "0.1", "--maf", "0.02")
    assert "Keeping " in r.stderr
    bad = str(f["dir"] / "bad.txt")
    with open(bad, "w") as fh:
        fh.write("1:1001\nnot a position\n")
    for args, needle in ((["--extract", bad], "line 2"), (["--maf", "0.6"], "--maf"), (["--geno", "x"], "--geno"), (["--maf", "0.4", "--max-maf", "0.1"], "min_maf")):
        r = subprocess.run([hostlib.CLI_PATH, "ldscore", "-i", f["full"], "-r", "0", *args], capture_output=True, text=True)
        assert r.returncode != 0 and needle in r.stderr, (args, r.stderr[-500:])


def test_cli_chunks_split_the_kept_variants(cli_files):
    """-c / -C: a chunk's L / R split is the kept variants among its first nL - the three chunks' partial scores add up to the whole run's."""
    f = cli_files
    sel = selections(f)[0][1]

    def scores(*extra):
        rows = [l.split("\t") for l in run_cli("ldscore", "-i", f["full"], "-r", "0", *sel, *extra).stdout.splitlines() if not l.startswith("#")]
        return {(r[0], int(r[1])): (int(r[2]), float(r[3])) for r in rows}

    whole = scores()
    assert len(whole) == len(f["kept"])
    n, s = dict.fromkeys(whole, 0), dict.fromkeys(whole, 0.0)
    for part in (1, 2, 3):
        for key, (n_k, s_k) in scores("-c", "3", "-C", part).items():
            n[key] += n_k
            s[key] += s_k
    assert n == {k: v[0] for k, v in whole.items()}
    assert all(abs(s[k] - v[1]) <= 1e-9 * max(1.0, v[1]) for k, v in whole.items())
