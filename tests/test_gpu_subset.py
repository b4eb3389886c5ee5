"""Sample subsets (twk_hip_select_samples, `--keep` / `--remove`): LD over a chosen set of samples, selected on the GPU from the data
that is already there.

THE YARDSTICK IS THE ENGINE ITSELF FED THE SUBSET FROM THE HOST: a second context that received alleles[:, keep] through
tests/util.upload.  The contract is that the two cannot be told apart, so equality is byte for byte everywhere and no parity
exemption is used; one comparison against the oracle (test_selected_records_match_the_oracle) ties the pair to the outside.
"""
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tomahawk_amd import hostlib

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -5


@pytest.fixture(scope="module")
def other():
    """The context that is fed the subset from the host."""
    eng = T.HipLd(0)
    yield eng
    eng.close()


def keep_lists(N, seed=5):
    """The lists of `make subset-check` (csrc/tools/subset_index_check.cpp) that fit N samples -> {name: ascending int64 indices}."""
    rng = np.random.default_rng(seed)
    out = {"everything": np.arange(N), "the first": np.array([0]), "the last": np.array([N - 1]), "every second": np.arange(0, N, 2),
           "3 of the whole": np.array([0, N // 2, N - 1])}
    if N >= 16:
        out["the first 16"] = np.arange(16)
    if N >= 17:
        out["the last 17"] = np.arange(N - 17, N)
    if N >= 33:
        out["the run [15, 33)"] = np.arange(15, 33)
    for density in (0.01, 0.5, 0.99):
        k = np.nonzero(rng.random(N) < density)[0]
        if len(k):
            out[f"random at {density}"] = k
    return out


def state_of(eng):
    """Everything the contract names of a context's data: (data words, mask words, marginals, metadata) as bytes."""
    data, mask = eng.download()
    return (eng.n_samples, data.tobytes(), mask.tobytes(), tuple(m.tobytes() for m in eng.marginals()), eng.meta().tobytes())


def assert_same_state(got, want, what):
    for name, g, w in zip(("n_samples", "data", "mask", "marginals", "meta"), got, want):
        assert g == w, f"{what}: {name} differs"


DATA_SETS = {
    "96x140": lambda: util.random_alleles(96, 140, 11),
    "96x161-missing": lambda: util.random_alleles(96, 161, 12, miss_variants=0.3, miss_rate=0.2),
    "70x1000": lambda: util.random_alleles(70, 1000, 13),
    "64x5000": lambda: util.random_alleles(64, 5000, 14),          # the output rows of the dense lists span several blocks
}


# ---- 1: bits and metadata -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DATA_SETS))
def test_selected_bits_and_metadata_equal_an_upload_of_the_subset(hip, other, name):
    al = DATA_SETS[name]()
    M, N, _ = al.shape
    util.upload(hip, al)
    source = state_of(hip)
    assert hip.selection() == (N, N)
    lists = keep_lists(N)
    for what, keep in lists.items():
        hip.select_samples(keep)
        assert hip.selection() == (N, len(keep)) and hip.n_samples == len(keep)
        util.upload(other, al[:, keep])
        want = state_of(other)
        assert_same_state(state_of(hip), want, f"{name}, {what}")
        meta = hip.meta()
        assert (meta["hwe"] == 1.0).all() and (other.meta()["hwe"] == 1.0).all()
        last = hip.select_last()
        assert last["select_ms"] > 0 and last["bytes_written"] > 0 and 0 < last["bytes_read"] <= M * ((N + 15) // 16) * 4 * 2
    # (`want` is the last list's, "random at 0.99": select A then select B equals select B directly - B is taken from the source)
    hip.select_samples(lists["every second"])
    hip.select_samples(lists["random at 0.99"])
    assert_same_state(state_of(hip), want, f"{name}, A then B")
    hip.select_samples(None)
    assert hip.selection() == (N, N)
    assert_same_state(state_of(hip), source, f"{name}, dropped")


# ---- 2: every consumer sees the working set -------------------------------------------------------------------------------------------------
def consumer_outputs(eng):
    """name -> bytes of one call each, on whatever the context holds."""
    M = eng.n_variants
    out = {}
    for mode_key, mode in (("p", T.MODE_PHASED), ("u", T.MODE_UNPHASED), ("auto", T.MODE_AUTO)):
        for minR2 in (0.0, 0.2):
            recs, npairs, nrec = eng.ld_region(mode, T.Filters(minR2=minR2), 0, M, 0, M, True)
            assert npairs == M * (M - 1) // 2 and nrec == len(recs)
            out[f"ld_region -{mode_key} -r {minR2}"] = recs.tobytes()
    f0 = T.Filters(minR2=0.0)
    n, s, _ = eng.ld_score(T.MODE_AUTO, f0)
    out["ld_score"] = n.tobytes() + s.tobytes()
    out["ld_matrix"] = eng.ld_matrix(T.MODE_AUTO, f0, stat=T.STAT_R)[0].tobytes()
    idx, val, _ = eng.ld_topk(T.MODE_AUTO, f0, 4)
    out["ld_topk"] = idx.tobytes() + val.tobytes()
    out["ld_prune"] = eng.ld_prune(T.MODE_AUTO, T.Filters(minR2=0.2))[0].tobytes()
    n, s, _ = eng.ld_decay(T.MODE_AUTO, f0, range_bp=20000, n_bins=50)
    out["ld_decay"] = n.tobytes() + s.tobytes()
    out["relationship"] = eng.relationship(stat=T.REL_KING).tobytes()
    return out


CONSUMER_SETS = {
    "96x161-missing": lambda: util.random_alleles(96, 161, 12, miss_variants=0.3, miss_rate=0.2),
    "mosaic140": lambda: util.mosaic_alleles(140, 140, 21),
}


@pytest.fixture(scope="module")
def consumer_pair(hip, other):
    """-> {data set: (outputs of the selected context, outputs of the host-subset upload)}, computed once."""
    out = {}
    for name, make in CONSUMER_SETS.items():
        al = make()
        keep = np.sort(np.random.default_rng(3).choice(al.shape[1], size=al.shape[1] // 2, replace=False))
        util.upload(hip, al)
        hip.select_samples(keep)
        got = consumer_outputs(hip)
        hip.select_samples(None)
        util.upload(other, al[:, keep])
        out[name] = (got, consumer_outputs(other))
    return out


CALLS = [f"ld_region -{m} -r {r}" for m in ("p", "u", "auto") for r in (0.0, 0.2)] + ["ld_score", "ld_matrix", "ld_topk", "ld_prune", "ld_decay", "relationship"]


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("name", list(CONSUMER_SETS))
def test_every_consumer_sees_the_working_set(consumer_pair, name, call):
    got, want = consumer_pair[name]
    # (iid genotypes of 80 samples hold no pair at r2 >= 0.2: those record arrays are empty on both sides, the mosaic's are not)
    assert len(want[call]) > 0 or (name != "mosaic140" and call.endswith("-r 0.2"))
    assert got[call] == want[call], f"{name}: {call} differs between the selection and the upload of the subset"


# ---- 3: missing data that leaves ------------------------------------------------------------------------------------------------------------
def test_missing_data_that_leaves_with_the_dropped_samples(hip, other):
    """All missing genotypes sit in samples the list drops: the working set has no missing data, keeps no mask rows, and the default
    mode takes the phased math for every pair, as after a re-import."""
    al = util.random_alleles(80, 150, 31)
    rng = np.random.default_rng(32)
    dropped = np.sort(rng.choice(150, size=40, replace=False))
    keep = np.setdiff1d(np.arange(150), dropped)
    for v in range(0, 80, 3):
        al[v, rng.choice(dropped, size=5, replace=False), :] = 2
    util.upload(hip, al)
    assert hip.meta()["missing"].sum() == 27
    hip.select_samples(keep)
    meta = hip.meta()
    assert not meta["missing"].any() and not meta["an"].any()
    assert not hip.download()[1].any()
    got, _, _ = hip.ld_region(T.MODE_AUTO, T.Filters(minR2=0.0), 0, 80, 0, 80, True)
    hip.select_samples(None)
    assert hip.meta()["missing"].sum() == 27
    util.upload(other, al[:, keep])
    want, _, _ = other.ld_region(T.MODE_PHASED, T.Filters(minR2=0.0), 0, 80, 0, 80, True)
    assert len(want) > 1000 and got.tobytes() == want.tobytes()


# ---- 4: against the oracle, once ------------------------------------------------------------------------------------------------------------
def test_selected_records_match_the_oracle(hip):
    al = util.random_alleles(64, 300, 41)
    keep = np.sort(np.random.default_rng(42).choice(300, size=100, replace=False))
    util.upload(hip, al)
    hip.select_samples(keep)
    got, npairs, _ = hip.ld_region(T.MODE_PHASED, T.Filters(minR2=0.0), 0, 64, 0, 64, True)
    hip.select_samples(None)
    sub = np.ascontiguousarray(al[:, keep])
    data, mask = O.bitvectors_from_alleles(sub)
    variants = O.variants_from_alleles(sub)
    want = O.all_pairs(data, mask, variants, 100, O.settings(minR2=0.0, phased=True), vector_only=True)
    assert npairs == 64 * 63 // 2 and len(want) > 1000
    util.assert_records_match(got, want, variants, n_samples=100)


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(hip):
    al = util.random_alleles(40, 90, 51, miss_variants=0.3, miss_rate=0.1)
    data, mask, variants = util.upload(hip, al)
    lib, ctx = hip._lib, hip._ctx
    with T.HipLd(0) as fresh:                                   # before an upload: TWK_HIP_E_STATE
        ids = np.arange(3, dtype=np.uint32)
        assert lib.twk_hip_select_samples(fresh._ctx, ids.ctypes.data, 3) == E_STATE
        fresh.set_problem(90, 40)
        assert lib.twk_hip_select_samples(fresh._ctx, ids.ctypes.data, 3) == E_STATE
    keep = np.arange(5, 70, 2)
    hip.select_samples(keep)
    before = state_of(hip)
    for bad in ([3, 2, 7], [3, 3, 7], [0, 5, 90], [1, 4, 2 ** 32 - 1], []):
        with pytest.raises(T.HipError) as ei:
            hip.select_samples(bad)
        assert ei.value.code == E_INVALID, bad
    with pytest.raises(T.HipError) as ei:
        hip.select_samples([0, 5, 90])
    assert "keep[2]" in str(ei.value)                           # the position is named
    assert lib.twk_hip_select_samples(ctx, None, 3) == E_INVALID          # NULL with a count
    with pytest.raises(TypeError):
        hip.select_samples([0.5, 1.5])
    assert hip.selection() == (90, len(keep))
    assert_same_state(state_of(hip), before, "after the refusals")
    # an upload, of either kind, and the generator while a selection is active: TWK_HIP_E_STATE, and the selection stands
    with pytest.raises(T.HipError) as ei:
        hip.upload(data, util.to_hip_meta(variants), mask)
    assert ei.value.code == E_STATE
    with pytest.raises(T.HipError) as ei:
        hip.generate_synthetic(1)
    assert ei.value.code == E_STATE
    assert_same_state(state_of(hip), before, "after the refused uploads")
    # set_hwe writes the working set only: the next selection and the drop bring the uploaded values back
    hip.set_hwe(np.full(40, 0.25))
    assert (hip.meta()["hwe"] == 0.25).all()
    hip.select_samples(keep)
    assert (hip.meta()["hwe"] == 1.0).all()
    hip.set_hwe([0.5, 0.5], first=3)
    assert hip.meta()["hwe"].tolist() == [1.0] * 3 + [0.5] * 2 + [1.0] * 35
    hip.select_samples(None)
    assert (hip.meta()["hwe"] == 1.0).all()
    # set_problem clears everything
    hip.select_samples(keep)
    hip.set_problem(90, 40)
    assert hip.selection() == (90, 90)
    hip.upload(data, util.to_hip_meta(variants), mask)          # (no selection is active any more)
    assert hip.download()[0].tobytes() == data.tobytes()


# ---- 6: the commands, end to end ------------------------------------------------------------------------------------------------------------
def subset_hwe(al):
    """The importer's Hardy-Weinberg P of every variant of `al`, over its complete genotypes: what a re-import of these samples carries."""
    complete = (al != 2).all(axis=2)
    alt = np.where(complete, al.sum(axis=2), -1)
    return np.array([hostlib.hwe_exact(int((a == 0).sum()), int((a == 1).sum()), int((a == 2).sum())) for a in alt])


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    """A .twk of 90 samples (the capi helper names them S0, S1, ..), the .twk of a subset of 37 written from the host with the subset's
    own Hardy-Weinberg P, and the --keep / --remove lists that select that subset from the first."""
    d = tmp_path_factory.mktemp("subset_cli")
    al = util.mosaic_alleles(150, 90, 61, miss_variants=0.2, miss_rate=0.15)
    M, N, _ = al.shape
    keep = np.sort(np.random.default_rng(62).choice(N, size=37, replace=False))
    pos, rid = 1000 + 100 * np.arange(M), np.zeros(M, np.uint32)
    full, sub = str(d / "full.twk"), str(d / "sub.twk")
    hostlib.write_twk(full, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=1, block_size=40)
    hostlib.write_twk(sub, np.ascontiguousarray(al[:, keep]), pos, rid, phased=np.ones(M, np.uint8), n_contigs=1, block_size=40,
                      hwe=subset_hwe(al[:, keep]))
    keep_file, remove_file = str(d / "keep.txt"), str(d / "remove.txt")
    with open(keep_file, "w") as fh:
        fh.write("# the population\n\n" + "".join(f"S{s}\n" for s in keep[::-1]))          # (any order: header order comes out)
    with open(remove_file, "w") as fh:
        fh.write("".join(f"S{s}\n" for s in np.setdiff1d(np.arange(N), keep)))
    return dict(dir=d, full=full, sub=sub, keep=keep, keep_file=keep_file, remove_file=remove_file, names=[f"S{s}" for s in keep])


def run_cli(*args):
    r = subprocess.run([hostlib.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def body(text):
    """The lines of a command's text output without the two that differ from run to run by design: `##tomahawk_<name>Version=` and
    `##tomahawk_<name>Command=..; Date=..`.  The command's other `##` lines (##annotations, ##M, ##M_5_50, ##top, ##stat) stay."""
    return [l for l in text.splitlines() if not l.startswith("##tomahawk_")]


def test_cli_ldscore_keep_equals_ldscore_of_the_subset_file(cli_files):
    want = body(run_cli("ldscore", "-i", cli_files["sub"], "-r", "0").stdout)
    assert len(want) >= 150
    assert body(run_cli("ldscore", "-i", cli_files["full"], "-r", "0", "--keep", cli_files["keep_file"]).stdout) == want
    assert body(run_cli("ldscore", "-i", cli_files["full"], "-r", "0", "--remove", cli_files["remove_file"]).stdout) == want
    # keep, then remove: half of the kept samples removed again is the other half kept
    half = str(cli_files["dir"] / "half.txt")
    with open(half, "w") as fh:
        fh.write("".join(name + "\n" for name in cli_files["names"][::2]))
    rest = str(cli_files["dir"] / "rest.txt")
    with open(rest, "w") as fh:
        fh.write("".join(name + "\n" for name in cli_files["names"][1::2]))
    both = body(run_cli("ldscore", "-i", cli_files["full"], "-r", "0", "--keep", cli_files["keep_file"], "--remove", half).stdout)
    assert both == body(run_cli("ldscore", "-i", cli_files["full"], "-r", "0", "--keep", rest).stdout) != want


def test_cli_calc_keep_equals_calc_of_the_subset_file(cli_files):
    d = cli_files["dir"]
    outs = {}
    for what, args in (("sub", ["-i", cli_files["sub"]]), ("keep", ["-i", cli_files["full"], "--keep", cli_files["keep_file"]]),
                       ("remove", ["-i", cli_files["full"], "--remove", cli_files["remove_file"]])):
        outs[what] = str(d / f"calc_{what}.two")
        r = run_cli("calc", *args, "-o", outs[what], "-r", "0.05")
        if what != "sub":
            assert "Samples: 37" in r.stderr and "Keeping 37 of 90 samples" in r.stderr
    views = {what: run_cli("view", "-i", path, "-H").stdout for what, path in outs.items()}
    assert len(views["sub"].splitlines()) > 1000
    assert views["keep"] == views["sub"] and views["remove"] == views["sub"]          # flags, counts, statistics: every column of every record
    recs = {what: hostlib.read_two(path)[0] for what, path in outs.items()}
    assert recs["keep"].tobytes() == recs["sub"].tobytes() == recs["remove"].tobytes()
    assert hostlib.sample_names(outs["keep"]) == cli_files["names"] == hostlib.sample_names(outs["remove"])
    assert hostlib.sample_names(outs["sub"]) == [f"S{s}" for s in range(37)]         # (the helper's own names)


def test_cli_relationship_keep_writes_the_kept_names(cli_files, hip):
    prefix = str(cli_files["dir"] / "rel")
    run_cli("relationship", "-i", cli_files["full"], "--keep", cli_files["keep_file"], "-o", prefix)
    assert open(prefix + ".samples.tsv").read().splitlines() == cli_files["names"]
    prefix_sub, prefix_rm = str(cli_files["dir"] / "rel_sub"), str(cli_files["dir"] / "rel_rm")
    run_cli("relationship", "-i", cli_files["sub"], "-o", prefix_sub)
    run_cli("relationship", "-i", cli_files["full"], "--remove", cli_files["remove_file"], "-o", prefix_rm)
    m = np.load(prefix + ".npy")
    assert m.shape == (37, 37) and m.tobytes() == np.load(prefix_sub + ".npy").tobytes() == np.load(prefix_rm + ".npy").tobytes()
    assert open(prefix_rm + ".samples.tsv").read() == open(prefix + ".samples.tsv").read()


def test_cli_other_commands_take_the_options(cli_files):
    """prune, ldmatrix, lddecay and ldscore --annot / --top through the one option table: each equals its run on the subset file."""
    d = cli_files["dir"]
    annot = str(d / "annot.tsv")
    with open(annot, "w") as fh:
        fh.write("contig\tpos\tall\todd\n" + "".join(f"1\t{1001 + 100 * v}\t1\t{v & 1}\n" for v in range(150)))
    for cmd in (["prune", "-r", "0.3"], ["lddecay", "-r", "0", "-d", "20000", "-b", "40"], ["ldscore", "-r", "0", "--annot", annot],
                ["ldscore", "-r", "0", "--top", "3"]):
        want = body(run_cli(cmd[0], "-i", cli_files["sub"], *cmd[1:]).stdout)
        got = body(run_cli(cmd[0], "-i", cli_files["full"], "--keep", cli_files["keep_file"], *cmd[1:]).stdout)
        assert len(want) > 10 and got == want, cmd
        if "--annot" in cmd:          # the regression's denominators are the kept samples': 2 x 37 alleles less the missing ones
            assert any(l.startswith("##M_5_50=") for l in want)
    for what, args in (("sub", ["-i", cli_files["sub"]]), ("keep", ["-i", cli_files["full"], "--keep", cli_files["keep_file"]])):
        run_cli("ldmatrix", *args, "-r", "0", "-o", str(d / f"mx_{what}"))
    assert np.load(str(d / "mx_keep.npy")).tobytes() == np.load(str(d / "mx_sub.npy")).tobytes()
