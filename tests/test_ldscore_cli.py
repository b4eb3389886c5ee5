"""LD scores, the parts that need no GPU: the `tomahawk ldscore` command line, the C ABI's declaration, the score kernels as compiled."""
import os
import re
import subprocess

import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def test_ldscore_without_arguments_prints_its_usage():
    r = _run("ldscore")
    assert r.returncode == 1
    assert "Usage:  tomahawk ldscore [options] -i <in.twk>" in r.stderr
    for flag in ("-i FILE", "-o FILE", "-t INT", "-p ", "-u ", "-r FLOAT", "-w INT", "-I STRING", "-c INT", "-C INT"):
        assert flag in r.stderr, flag
    assert r.stdout == ""


def test_help_lists_ldscore():
    r = _run()
    assert r.returncode == 1 and re.search(r"^\s+ldscore\s+\S", r.stderr, re.M)
    r = _run("no-such-command")
    assert r.returncode == 1 and "`ldscore`" in r.stderr


def test_a_fisher_cutoff_is_refused_before_any_device_is_touched(tmp_path):
    """-P below 1: refused while the options are parsed - the input file does not even exist, and no HIP message appears."""
    r = _run("ldscore", "-i", str(tmp_path / "absent.twk"), "-P", "0.5")
    assert r.returncode == 1
    assert "cutoff P-value below 1" in r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and r.stdout == ""
    assert _run("ldscore", "-i", str(tmp_path / "absent.twk"), "-P", "1").stderr.count("cutoff P-value") == 0


def test_header_declares_the_entry_point_and_the_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"^int twk_hip_ld_score\(twk_hip_ctx\* ctx, int mode, const twk_hip_filters\* filters,", header, re.M)
    assert re.search(r"uint64_t\* n_partners, double\* sum_r2, uint64_t\* n_pairs\);", header)
    assert re.search(r"^#define TWK_HIP_ABI_VERSION 5$", header, re.M)
    import tomahawk_amd as T
    lib = T.load_library()
    assert lib.twk_hip_abi_version() == 5 and hasattr(lib, "twk_hip_ld_score")
    # the call sequence is checked without a device: no context -> TWK_HIP_E_INVALID
    assert lib.twk_hip_ld_score(None, 1, None, 0, 1, 0, 1, 1, 0, 1, 0, 0, 0, None, None, None) == -1
    assert "bool Score(const twk_ld_settings& settings);" in open(os.path.join(ROOT, "include", "twk_ld.h")).read()


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_score_kernels_use_no_scratch_memory():
    """The score kernels as `make hip` compiles them: the record d_pair fills is never stored (only `keep` and R2 are used), so no
    kernel of the score path may have a private segment or spill a vector register."""
    seen = []
    for name, body in util.engine_kernels().items():
        if "k_ld_score" not in name:
            continue
        seen.append(name)
        _, scratch, spills = util.kernel_resources(body)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert len(seen) >= 2 and any("fold" in n for n in seen), seen
