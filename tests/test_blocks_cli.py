"""Haplotype blocks: `tomahawk blocks` against the binding, and the parts that need no GPU - the host check of the plain C++ header and
the kernels' resources by their metadata."""
import os
import re
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import blocks_cases as BC
from tests import util
from tests.reduce_cases import mosaic140
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0 = T.Filters(minR2=0.0)


def test_make_blocks_check_passes():
    """The scan against a long double restatement, the byte stores lane by lane, the prefix counts, the candidates against the contract,
    the sort key's order and the walk with lanes running ahead (csrc/tools/blocks_check.cpp), under ASan and UBSan."""
    r = subprocess.run(["make", "-C", ROOT, "blocks-check"], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"^blocks-check: (\d+) cases, (\d+) bad$", r.stdout, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, r.stdout[-500:]


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_block_kernels_use_no_scratch_memory_and_spill_nothing():
    """The kernels as `make hip` compiles them, by their metadata alone: what DESIGN 3.18 states.  The bounds' kernel - the pair function
    and the likelihood scan behind it, both out of line - is given at most 168 VGPRs: three waves a SIMD."""
    names = util.reduce_kernels_fit("k_ld_dprime_ci_band")
    assert len(names) == 1, names
    others = {n: util.kernel_resources(b) for n, b in util.engine_kernels().items() if "k_blocks_" in n or "k_ci_informative" in n}
    assert len(others) >= 7, sorted(others)      # prefix, candidates x 2, flatten, walk x 2, informative
    assert all(scratch == 0 and spills == 0 for _, scratch, spills in others.values()), others


def test_blocks_usage_and_refusals_need_no_device():
    r = subprocess.run([hostlib.CLI_PATH, "blocks"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage:  tomahawk blocks" in r.stderr and "--ci-out PREFIX" in r.stderr
    for args, what in ((["-c", "2"], "a block needs every pair inside it"), (["-P", "0.5"], "Fisher's exact test is not run"), (["--ci-out", ""], "--ci-out wants a prefix")):
        r = subprocess.run([hostlib.CLI_PATH, "blocks", "-i", "none.twk"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr and "Calling" not in r.stderr, (args, r.stderr)
    # the list of commands stays as recorded (tests/golden/cli_transcript.json): blocks is reached by its name only
    r = subprocess.run([hostlib.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert "blocks" not in r.stderr


@pytest.mark.gpu
def test_blocks_cli_agrees_with_the_binding(hip, tmp_path):
    al = mosaic140(250)
    M, N, _ = al.shape
    h = 83
    rid = np.repeat([0, 1], [h, M - h]).astype(np.uint32)
    pos = BC.positions(M)
    pos[h:] -= pos[h] - 500
    pos = pos.astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    out, prefix = str(tmp_path / "blocks.tsv"), str(tmp_path / "ci")
    r = subprocess.run([hostlib.CLI_PATH, "blocks", "-i", twk, "-o", out, "-p", "-w", "20000", "--ci-out", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    util.upload(hip, al, variants)
    block_of, first, last, n_strong, n_recomb, n_cand, n_inf, _ = hip.ld_blocks(T.MODE_PHASED, F0, 20000)
    assert len(first) > 10
    lines = open(out).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    rows = [l.split("\t") for l in lines if not l.startswith("#")]
    assert f"##blocks={len(first)},candidates={n_cand},informative={n_inf},total={M}" in head
    assert "##thresholds=strong_lo=70,strong_hi=98,recomb_hi=90,strong_lo_2=80,strong_lo_34=50,inform_permille=950,max_span_2=20000,max_span_3=30000" in head
    assert head[-1] == "#contig\tfirst_pos\tlast_pos\tspan\tvariants\tstrong\trecombinant"
    want = [[str(int(rid[a]) + 1), str(int(pos[a]) + 1), str(int(pos[b]) + 1), str(int(pos[b]) - int(pos[a])), str(int(b - a + 1)), str(int(s)), str(int(c))]
            for a, b, s, c in zip(first, last, n_strong, n_recomb)]
    assert rows == want
    # the bounds' files: the binding's bytes, through the band writer
    lo, hi, bfirst, indptr, _, _ = hip.ld_dprime_ci_band(T.MODE_PHASED, F0, 20000)
    got = {name: np.load(f"{prefix}.{name}.npy") for name in ("lo", "hi", "indptr", "first")}
    assert got["lo"].dtype == np.uint8 and got["hi"].dtype == np.uint8
    assert np.array_equal(got["lo"], lo) and np.array_equal(got["hi"], hi) and (lo != BC.NONE).sum() == 2 * n_inf
    assert got["indptr"].dtype == np.int64 and np.array_equal(got["indptr"], indptr.astype(np.int64))
    assert got["first"].dtype == np.int32 and np.array_equal(got["first"], bfirst.astype(np.int32))
    vrows = [l.split("\t") for l in open(prefix + ".variants.tsv").read().splitlines()]
    assert [x[0] for x in vrows] == [str(int(x) + 1) for x in rid] and [int(x[1]) for x in vrows] == [int(p) + 1 for p in pos]
    # the window defaults to 200,000 bases
    r = subprocess.run([hostlib.CLI_PATH, "blocks", "-i", twk, "-p"], capture_output=True, text=True, timeout=300)
    wide = hip.ld_blocks(T.MODE_PHASED, F0)
    assert r.returncode == 0 and "##window=200000 bases" in r.stdout
    assert len([l for l in r.stdout.splitlines() if not l.startswith("#")]) == len(wide[1])
