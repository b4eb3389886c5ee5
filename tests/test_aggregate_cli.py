"""LD aggregate, the parts that need no GPU: the `tomahawk ldaggregate` command line and the host check of the bin arithmetic."""
import os
import re
import subprocess

import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def test_ldaggregate_without_arguments_prints_its_usage():
    r = _run("ldaggregate")
    assert r.returncode == 1
    assert "Usage:  tomahawk ldaggregate [options] -i <in.twk> [-o <out.tsv>]" in r.stderr
    for flag in ("-i FILE", "-o FILE", "-x INT", "-y INT", "-s STRING", "-R STRING", "-m INT", "-t INT", "-c INT", "-C INT", "-p ", "-u ", "-r FLOAT",
                 "-w INT", "-I STRING", "-P FLOAT", "--engine-option"):
        assert flag in r.stderr, flag
    assert r.stderr.count("(default: 1000)") == 2                      # -x and -y: the reference's
    assert "r2, r (signed), D or Dprime (default: r2)" in r.stderr
    assert "mean, count (or n), min, max, sd or total (default: mean)" in r.stderr
    assert "prints 0 (default: 5)" in r.stderr                         # -m: the reference's -c
    assert "(default: 0)" in r.stderr                                  # -r: a heat map has no cut-off
    assert "x rows of y" in r.stderr
    assert r.stdout == ""


def test_help_lists_ldaggregate_after_lddecay_and_aggregate_stays_the_references():
    r = _run()
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    at = [k for k, l in enumerate(lines) if re.match(r"\s+lddecay\s+\S", l)]
    assert len(at) == 1 and re.match(r"\s+ldaggregate\s+\S", lines[at[0] + 1])
    before = [k for k, l in enumerate(lines) if re.match(r"\s+ldmatrix\s+\S", l)]
    assert before == [at[0] - 1]
    r = _run("aggregate")
    assert r.returncode == 1 and "Illegal command" in r.stderr
    assert "`lddecay`, `ldaggregate`, `concat`" in r.stderr and "aggregate/decay/... are the reference's" in r.stderr
    r = _run("decay")
    assert r.returncode == 1 and "Illegal command" in r.stderr


def _refused(r, what):
    assert r.returncode == 1
    assert what in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr and r.stdout == ""


def test_bad_bins_statistics_reductions_and_a_fisher_cutoff_are_refused_before_any_device_is_touched(tmp_path):
    """Refused while the options are parsed: the input does not exist and is never asked for."""
    base = ("ldaggregate", "-i", str(tmp_path / "absent.twk"))
    _refused(_run(*base, "-x", "0"), "The number of x bins (-x) must be between 1 and 4096")
    _refused(_run(*base, "-x", "4097"), "The number of x bins (-x) must be between 1 and 4096")
    _refused(_run(*base, "-x", "ten"), "must be a non-negative integer")
    _refused(_run(*base, "-y", "0"), "The number of y bins (-y) must be between 1 and 4096")
    _refused(_run(*base, "-y", "4097"), "The number of y bins (-y) must be between 1 and 4096")
    _refused(_run(*base, "-y", "-3"), "must be a non-negative integer")
    _refused(_run(*base, "-s", "R2"), "Unknown statistic (-s): R2")
    _refused(_run(*base, "-s", "p"), "Unknown statistic (-s): p")
    _refused(_run(*base, "-R", "median"), "Unknown reduction (-R): median")
    _refused(_run(*base, "-m", "-1"), "The minimum count (-m) must be a non-negative integer")
    _refused(_run(*base, "-m", "few"), "The minimum count (-m) must be a non-negative integer")
    _refused(_run(*base, "-P", "0.5"), "cutoff P-value below 1")
    # the same flags with good values get as far as the input
    r = _run(*base, "-x", "1", "-y", "4096", "-s", "Dprime", "-R", "sd", "-m", "0", "-P", "1")
    assert r.returncode == 1 and "Failed to open file" in r.stderr
    assert "cutoff P-value" not in r.stderr and "bins (-" not in r.stderr and "Unknown" not in r.stderr
    for red in ("mean", "count", "n", "min", "max", "sd", "total"):
        r = _run(*base, "-R", red)
        assert r.returncode == 1 and "Failed to open file" in r.stderr, red
    # -x, -y, -R and -m belong to ldaggregate alone
    for flag in ("-x", "-y", "-R", "-m"):
        r = _run("lddecay", "-i", str(tmp_path / "absent.twk"), flag, "10")
        assert r.returncode == 1 and "Calling" not in r.stderr, flag


def test_make_aggregate_check_passes():
    """Packing, quantisation, split, host conversion and the landscape against their naive restatement (csrc/tools/aggregate_bin_check.cpp)."""
    r = subprocess.run(["make", "-C", ROOT, "aggregate-check"], capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "aggregate_bin_check: ok" in r.stdout


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_aggregate_kernels_use_no_scratch_memory_and_run_three_waves_a_simd():
    """The aggregate kernels as `make hip` compiles them, by their metadata alone: what DESIGN 3.11 states."""
    names = util.reduce_kernels_fit("k_ld_aggregate")
    assert len(names) == 2 and any("k_ld_aggregate_init" in n for n in names), names
