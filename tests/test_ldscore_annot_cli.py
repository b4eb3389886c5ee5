"""Partitioned LD scores, the parts that need no GPU: `tomahawk ldscore --annot`'s annotation file and the host check of the term."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def test_make_annot_check_passes():
    """The term against llrint, the split and a whole block of the kernel against the double loop (csrc/tools/annot_term_check.cpp)."""
    r = subprocess.run(["make", "-C", ROOT, "annot-check"], capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"^annot-check: (\d+) cases, (\d+) bad$", r.stdout, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, r.stdout[-500:]


def test_the_short_flag_and_the_usage_stay_as_they_were():
    """The annotation file has long names only (--annot, --self): `ldscore -a` stays getopt's unknown option, `--assoc` stays refused,
    and the usage text - recorded byte for byte in tests/golden/cli_transcript.json - does not change."""
    r = _run("ldscore", "-i", "absent.twk", "-a", "1")
    assert r.returncode == 1 and "invalid option -- 'a'" in r.stderr and "annotation" not in r.stderr
    r = _run("ldscore", "-i", "absent.twk", "--assoc=1")
    assert r.returncode == 1 and "Unrecognized option: a" in r.stderr
    # ... and the long names belong to ldscore alone
    for cmd in ("prune", "lddecay"):
        r = _run(cmd, "-i", "absent.twk", "--annot", "x")
        assert r.returncode == 1 and "Unrecognized option" in r.stderr and "Calling" not in r.stderr


@pytest.fixture(scope="module")
def tiny_twk(tmp_path_factory):
    al = util.random_alleles(12, 16, seed=5)
    path = str(tmp_path_factory.mktemp("annot") / "tiny.twk")
    hostlib.write_twk(path, al, np.arange(12, dtype=np.uint32) * 100 + 1000, np.zeros(12, np.uint32), phased=np.ones(12, np.uint8), n_contigs=1, block_size=50)
    return path


def _refused(twk, tmp_path, text, what, line=None):
    """The annotation file `text` is refused with `what` (and its line) before the input is opened or a device touched."""
    path = str(tmp_path / "annot.txt")
    with open(path, "w") as fh:
        fh.write(text)
    r = _run("ldscore", "-i", twk, "--annot", path)
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert what in r.stderr, r.stderr
    if line is not None:
        assert f"{path}:{line}: " in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr and "Samples" not in r.stderr


HEAD = "contig\tpos\tcoding\tweight\n"


def test_the_same_variant_twice_is_refused(tiny_twk, tmp_path):
    _refused(tiny_twk, tmp_path, "## a comment\n" + HEAD + "1\t1001\t1\t0.5\n1\t1101\t0\t0.25\n1\t1001\t0\t1\n", "1:1001 is named twice", 5)


def test_a_short_row_is_refused(tiny_twk, tmp_path):
    _refused(tiny_twk, tmp_path, HEAD + "1\t1001\t1\t0.5\n1\t1101\t0\n", "expected 4 columns, found 3", 3)
    # ... and so is a row that lacks the SNP and CM columns its header announces
    _refused(tiny_twk, tmp_path, "CHR BP SNP CM coding\n1 1001 rs1 0 1\n1 1101 1\n", "expected 5 columns, found 3", 3)


def test_a_number_that_is_none_is_refused(tiny_twk, tmp_path):
    _refused(tiny_twk, tmp_path, HEAD + "1\t1001\t1\tnan\n", "not a finite annotation of at most 65536 in magnitude: nan", 2)
    _refused(tiny_twk, tmp_path, HEAD + "1\t1001\tinf\t1\n", "not a finite annotation of at most 65536 in magnitude: inf", 2)
    _refused(tiny_twk, tmp_path, HEAD + "1\t1001\tyes\t1\n", "not a finite annotation of at most 65536 in magnitude: yes", 2)


def test_an_annotation_beyond_the_range_is_refused(tiny_twk, tmp_path):
    _refused(tiny_twk, tmp_path, HEAD + "1\t1001\t65536\t-65536\n1\t1101\t1\t65537\n", "not a finite annotation of at most 65536 in magnitude: 65537", 3)


def test_too_many_and_no_columns_are_refused(tiny_twk, tmp_path):
    names = "\t".join(f"c{k}" for k in range(257))
    _refused(tiny_twk, tmp_path, "contig\tpos\t" + names + "\n", "must be between 1 and 256, not 257", 1)
    _refused(tiny_twk, tmp_path, "#contig\tpos\n1\t1001\n", "must be between 1 and 256, not 0", 1)
    _refused(tiny_twk, tmp_path, "CHR\tBP\tSNP\tCM\n", "must be between 1 and 256, not 0", 1)


def test_a_category_named_twice_is_refused(tiny_twk, tmp_path):
    _refused(tiny_twk, tmp_path, "contig\tpos\tcoding\tweight\tcoding\n1\t1001\t1\t1\t1\n", "the annotation coding is named twice", 1)


def test_a_missing_annotation_file_is_refused(tiny_twk, tmp_path):
    r = _run("ldscore", "-i", tiny_twk, "--annot", str(tmp_path / "absent.txt"))
    assert r.returncode == 1 and r.stdout == ""
    assert "Failed to open the annotation file: " + str(tmp_path / "absent.txt") in r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr


def test_self_without_an_annotation_file_is_refused(tiny_twk):
    r = _run("ldscore", "-i", tiny_twk, "--self")
    assert r.returncode == 1 and "--self needs an annotation file (--annot)" in r.stderr and "Calling" not in r.stderr


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_annot_kernel_uses_no_scratch_memory_and_runs_three_waves_a_simd():
    """The kernel as `make hip` compiles it, by its metadata alone: what DESIGN 3.13 states."""
    names = util.reduce_kernels_fit("k_ld_annot")
    assert len(names) == 1, names
    body = util.engine_kernels()[names[0]]
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", body).group(1)) <= 160 * 1024 // 3          # three blocks a CU
