"""LD decay, the parts that need no GPU: the `tomahawk lddecay` command line and the host check of the bin arithmetic."""
import os
import re
import subprocess

import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def test_lddecay_without_arguments_prints_its_usage():
    r = _run("lddecay")
    assert r.returncode == 1
    assert "Usage:  tomahawk lddecay [options] -i <in.twk> [-o <out.tsv>]" in r.stderr
    for flag in ("-i FILE", "-o FILE", "-d INT", "-b INT", "-t INT", "-c INT", "-C INT", "-p ", "-u ", "-r FLOAT", "-w INT", "-I STRING", "-P FLOAT",
                 "--engine-option"):
        assert flag in r.stderr, flag
    assert "(default: 10000000, or the -w window when only -w is given)" in r.stderr          # the reference's range
    assert "(default: 1000)" in r.stderr                                                      # ... and its number of bins
    assert "(default: 0)" in r.stderr                                                         # -r: a decay curve has no cut-off
    assert "From <TAB> To <TAB> Mean <TAB> Frequency <TAB> Sum" in r.stderr
    assert r.stdout == ""


def test_help_lists_lddecay_and_decay_stays_the_references():
    r = _run()
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    at = [k for k, l in enumerate(lines) if re.match(r"\s+ldmatrix\s+\S", l)]
    assert len(at) == 1 and re.match(r"\s+lddecay\s+\S", lines[at[0] + 1])
    r = _run("decay")
    assert r.returncode == 1 and "Illegal command" in r.stderr
    assert "`ldmatrix`, `lddecay`" in r.stderr and "aggregate/decay/... are the reference's" in r.stderr


def _refused(r, what):
    assert r.returncode == 1
    assert what in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr and r.stdout == ""


def test_bad_bins_ranges_and_a_fisher_cutoff_are_refused_before_any_device_is_touched(tmp_path):
    """Refused while the options are parsed: the input does not exist and is never asked for."""
    base = ("lddecay", "-i", str(tmp_path / "absent.twk"))
    _refused(_run(*base, "-b", "0"), "The number of bins (-b) must be between 1 and 4096")
    _refused(_run(*base, "-b", "4097"), "The number of bins (-b) must be between 1 and 4096")
    _refused(_run(*base, "-b", "ten"), "must be a non-negative integer")
    _refused(_run(*base, "-d", "0"), "The range (-d) must be between 1 and 4294967295")
    _refused(_run(*base, "-d", "500", "-b", "1000"), "cannot be smaller than the number of bins")
    _refused(_run(*base, "-b", "1000", "-d", "999"), "a bin would be 0 bases wide")
    _refused(_run(*base, "-w", "500"), "cannot be smaller than the number of bins")          # only -w given: it is the range
    _refused(_run(*base, "-P", "0.5"), "cutoff P-value below 1")
    # the same flags with good values get as far as the input
    r = _run(*base, "-d", "1000", "-b", "1000", "-P", "1")
    assert r.returncode == 1 and "Failed to open file" in r.stderr
    assert "cutoff P-value" not in r.stderr and "number of bins" not in r.stderr and "range (-d" not in r.stderr
    # -d and -b belong to lddecay alone
    r = _run("ldscore", "-i", str(tmp_path / "absent.twk"), "-b", "10")
    assert r.returncode == 1 and "Calling" not in r.stderr


def test_make_decay_check_passes():
    """The bin index, the quantisation and the host conversion against their naive restatement (csrc/tools/decay_bin_check.cpp)."""
    r = subprocess.run(["make", "-C", ROOT, "decay-check"], capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "decay_bin_check: ok" in r.stdout



@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_decay_kernels_use_no_scratch_memory_and_run_three_waves_a_simd():
    """The decay kernels as `make hip` compiles them, by their metadata alone: what DESIGN 3.10 states."""
    names = util.reduce_kernels_fit("k_ld_decay")
    assert len(names) == 1, names
