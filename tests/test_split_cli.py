"""LD splitting: `tomahawk ldsplit` against the binding, and the parts that need no GPU - option parsing and refusals, and the kernels'
resources by their metadata.  (The host check of the index arithmetic runs from tests/test_split_cpu.py.)"""
import os
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from oracle import oracle as O
from tests import util
from tests.reduce_cases import mosaic140
from tomahawk_amd import hostlib

F0 = T.Filters(minR2=0.0)


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_split_kernels_use_no_scratch_memory_and_spill_nothing():
    """The kernels as `make hip` compiles them, by their metadata alone: what DESIGN 3.19 states.  The layer kernel - the one that runs
    k_max times - is given at most 64 VGPRs, so that eight waves a SIMD can hide its loads of W."""
    seen = {n: util.kernel_resources(b) for n, b in util.engine_kernels().items() if "k_split_" in n}
    assert len(seen) == 4, sorted(seen)      # prefix, sums, layer, backtrack
    assert all(scratch == 0 and spills == 0 for _, scratch, spills in seen.values()), seen
    (layer,) = (v for n, v in seen.items() if "k_split_layer" in n)
    assert layer[0] <= 64, seen


def test_ldsplit_usage_and_refusals_need_no_device():
    r = subprocess.run([hostlib.CLI_PATH, "ldsplit"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage:  tomahawk ldsplit" in r.stderr and "--max-blocks INT" in r.stderr
    sizes = ["--min-size", "5", "--max-size", "9", "--max-blocks", "3"]
    for args, what in ((["--min-size", "0"], "--min-size wants an integer between 1 and 65535"),
                       (["--max-size", "65536"], "--max-size wants an integer between 1 and 65535"),
                       (["--max-blocks", "1025"], "--max-blocks wants an integer between 1 and 1024"),
                       (["--max-blocks", "x"], "--max-blocks wants an integer"),
                       (["-B", "0"], "-B wants an integer between 1 and 1024"),
                       (["--min-size", "5"], "A split needs --min-size, --max-size and --max-blocks"),
                       (["--min-size", "5", "--max-size", "4", "--max-blocks", "3", "-w", "100", "-o", "x"], "Cannot have --min-size above --max-size"),
                       (sizes + ["-o", "x"], "A split needs a window in bases (-w)"),
                       (sizes + ["-w", "100"], "-o wants a prefix"),
                       (sizes + ["-w", "100", "-o", "-"], "-o wants a prefix"),
                       (sizes + ["-w", "100", "-o", "x", "-B", "4"], "more blocks (-B) than --max-blocks"),
                       (["-c", "2"], "a block sum needs every pair inside the block"),
                       (["-P", "0.5"], "Fisher's exact test is not run"),
                       (["--ci-out", "x"], "unrecognized option '--ci-out'")):
        r = subprocess.run([hostlib.CLI_PATH, "ldsplit", "-i", "none.twk"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr and "Calling" not in r.stderr, (args, r.stderr)
    # the list of commands stays as recorded (tests/golden/cli_transcript.json): ldsplit is reached by its name only
    r = subprocess.run([hostlib.CLI_PATH], capture_output=True, text=True, timeout=60)
    assert "ldsplit" not in r.stderr


def rows_of(path):
    lines = open(path).read().splitlines()
    return [l for l in lines if l.startswith("#")], [l.split("\t") for l in lines if not l.startswith("#")]


@pytest.mark.gpu
def test_ldsplit_cli_agrees_with_the_binding(hip, tmp_path):
    al = mosaic140(250)
    M = al.shape[0]
    h = 83
    rid = np.repeat([0, 1], [h, M - h]).astype(np.uint32)
    pos = (np.arange(M, dtype=np.int64) * 100 + 1000)
    pos[h:] -= pos[h] - 500
    pos = pos.astype(np.uint32)
    twk = str(tmp_path / "in.twk")
    hostlib.write_twk(twk, al, pos, rid, phased=np.ones(M, np.uint8), n_contigs=2, block_size=50)
    prefix = str(tmp_path / "split")
    sizes = dict(min_size=8, max_size=30, k_max=7)
    r = subprocess.run([hostlib.CLI_PATH, "ldsplit", "-i", twk, "-o", prefix, "-p", "-w", "3000", "--min-size", "8", "--max-size", "30", "--max-blocks", "7", "-B", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    variants = O.variants_from_alleles(al, pos=pos, rid=rid, phase=1)
    util.upload(hip, al, variants)
    want_costs, want_blocks = [], []
    for c, (a0, n) in enumerate(((0, h), (h, M - h))):
        got = hip.ld_split(T.MODE_PHASED, F0, 3000, a0=a0, n=n, **sizes)
        assert 4 in got["K"] and len(got["K"]) >= 3
        for K, cuts in zip(got["K"], got["cuts"]):
            cost = int(got["cost"][K - 1])
            want_costs.append([str(c + 1), str(K), format(cost / 2.0 ** 32, ".17g"), format(float(cost) / float(got["total"]), ".17g"),
                               str(int((np.diff(cuts.astype(np.int64)) ** 2).sum()))])
        cuts = got["cuts"][got["K"].index(4)].astype(np.int64) + a0
        for i in range(4):
            a, b = cuts[i], cuts[i + 1] - 1
            want_blocks.append([str(c + 1), str(i + 1), str(int(pos[a]) + 1), str(int(pos[b]) + 1), str(int(b - a + 1))])
    head, rows = rows_of(prefix + ".costs.tsv")
    assert "##sizes=min_size=8,max_size=30,max_blocks=7" in head and "##window=3000 bases" in head
    assert head[-1] == "#contig\tK\tcost\tcost_fraction\tsum_squared_sizes"
    assert rows == want_costs
    head, rows = rows_of(prefix + ".blocks.tsv")
    assert head[-1] == "#contig\tblock\tfirst_pos\tlast_pos\tvariants"
    assert rows == want_blocks
    # a k that one contig cannot be split into: an error that names the contig, and no blocks file
    other = str(tmp_path / "other")
    r = subprocess.run([hostlib.CLI_PATH, "ldsplit", "-i", twk, "-o", other, "-p", "-w", "3000", "--min-size", "8", "--max-size", "30", "--max-blocks", "7", "-B", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Cannot split the contig of 1 (83 variants) into 2 blocks of 8 to 30 variants" in r.stderr
    assert not os.path.exists(other + ".blocks.tsv")
