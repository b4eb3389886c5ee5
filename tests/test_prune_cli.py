"""LD pruning, the parts that need no GPU: the `tomahawk prune` command line, the C ABI's declaration, the prune kernels as compiled."""
import os
import re
import subprocess

import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def test_prune_without_arguments_prints_its_usage():
    r = _run("prune")
    assert r.returncode == 1
    assert "Usage:  tomahawk prune [options] -i <in.twk>" in r.stderr
    for flag in ("-i FILE", "-o FILE", "-t INT", "-p ", "-u ", "-r FLOAT", "-w INT", "-I STRING", "-P FLOAT"):
        assert flag in r.stderr, flag
    assert "(default: 0.1)" in r.stderr          # -r: calc's default
    assert "-c INT" not in r.stderr and "-C INT" not in r.stderr
    assert "contig <TAB> pos <TAB> keep" in r.stderr
    assert r.stdout == ""


def test_help_lists_prune_next_to_ldscore():
    r = _run()
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    at = [k for k, l in enumerate(lines) if re.match(r"\s+ldscore\s+\S", l)]
    assert len(at) == 1 and re.match(r"\s+prune\s+\S", lines[at[0] + 1])
    r = _run("no-such-command")
    assert r.returncode == 1 and "`ldscore`, `prune`" in r.stderr


def test_a_fisher_cutoff_is_refused_before_any_device_is_touched(tmp_path):
    """-P below 1: refused while the options are parsed - the input file does not even exist, and no HIP message appears."""
    r = _run("prune", "-i", str(tmp_path / "absent.twk"), "-P", "0.5")
    assert r.returncode == 1
    assert "cutoff P-value below 1" in r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and r.stdout == ""
    assert _run("prune", "-i", str(tmp_path / "absent.twk"), "-P", "1").stderr.count("cutoff P-value") == 0


@pytest.mark.parametrize("flags", [["-c", "2", "-C", "4"], ["-c", "1"], ["-C", "1"]])
def test_a_part_of_the_pair_space_is_refused_before_any_device_is_touched(tmp_path, flags):
    r = _run("prune", "-i", str(tmp_path / "absent.twk"), *flags)
    assert r.returncode == 1
    assert "the walk needs every pair" in r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and r.stdout == ""


def test_header_declares_the_entry_point_and_the_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"^int twk_hip_ld_prune\(twk_hip_ctx\* ctx, int mode, const twk_hip_filters\* filters, uint32_t a0, uint32_t n, uint32_t tile_variants,", header, re.M)
    assert re.search(r"int32_t window, uint32_t l_window, uint8_t\* keep, uint64_t\* n_kept, uint64_t\* n_edges, uint64_t\* n_pairs\);", header)
    assert re.search(r"^#define TWK_HIP_ABI_VERSION 5$", header, re.M)
    assert re.search(r"\(still 5: twk_hip_ld_prune", header)
    import tomahawk_amd as T
    lib = T.load_library()
    assert lib.twk_hip_abi_version() == 5 and hasattr(lib, "twk_hip_ld_prune")
    # the call sequence is checked without a device: no context -> TWK_HIP_E_INVALID
    assert lib.twk_hip_ld_prune(None, 1, None, 0, 1, 0, 0, 0, None, None, None, None) == -1
    assert lib.twk_hip_prune_last(None, None, None) == -1
    assert hasattr(T.HipLd, "ld_prune")
    assert "bool Prune(const twk_ld_settings& settings);" in open(os.path.join(ROOT, "include", "twk_ld.h")).read()


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_prune_kernels_use_no_scratch_memory():
    """The prune kernels as `make hip` compiles them: the record d_pair fills is never stored (only `keep` is used), so no kernel of
    the prune path may have a private segment or spill a vector register."""
    seen = []
    for name, body in util.engine_kernels().items():
        if "k_ld_prune" not in name:
            continue
        seen.append(name)
        vgprs, scratch, spills = util.kernel_resources(body)
        print(name, "vgprs", vgprs, "scratch", scratch, "spills", spills)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert any("mask" in n for n in seen) and sum("walk" in n for n in seen) == 2, seen
