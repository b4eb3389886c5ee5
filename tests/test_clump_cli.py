"""LD clumping, the parts that need no GPU: the `tomahawk clump` command line, the C ABI's declaration, the clump kernels as compiled."""
import os
import re
import subprocess

import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def _assoc(tmp_path, text):
    path = str(tmp_path / "assoc.txt")
    with open(path, "w") as fh:
        fh.write(text)
    return path


def test_clump_without_arguments_prints_its_usage():
    r = _run("clump")
    assert r.returncode == 1
    assert "Usage:  tomahawk clump [options] -i <in.twk> -a <assoc.txt>" in r.stderr
    for flag in ("-i FILE", "-a FILE", "-1 FLOAT", "-2 FLOAT", "-o FILE", "-t INT", "-p ", "-u ", "-r FLOAT", "-w INT", "-I STRING", "-P FLOAT"):
        assert flag in r.stderr, flag
    assert "(default: 0.1)" in r.stderr          # -r: calc's default, so that calc's flags mean calc's pairs
    assert "(default: 1e-4)" in r.stderr and "(default: 1e-2)" in r.stderr
    assert "the same flags as calc mean the same pairs in LD" in r.stderr
    assert "-c INT" not in r.stderr and "-C INT" not in r.stderr
    assert "contig <TAB> pos <TAB> P <TAB> index_contig <TAB> index_pos" in r.stderr
    assert "##clumps=" in r.stderr
    assert r.stdout == ""


def test_help_lists_clump_after_prune():
    r = _run()
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    at = [k for k, l in enumerate(lines) if re.match(r"\s+prune\s+\S", l)]
    assert len(at) == 1 and re.match(r"\s+clump\s+\S", lines[at[0] + 1])
    r = _run("no-such-command")
    assert r.returncode == 1 and "`ldscore`, `prune`, `clump`" in r.stderr


def _refused(r, what):
    assert r.returncode == 1
    assert what in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr and r.stdout == ""


def test_a_fisher_cutoff_is_refused_before_any_device_is_touched(tmp_path):
    """-P below 1: refused while the options are parsed - neither the input nor the association file exists."""
    base = ("clump", "-i", str(tmp_path / "absent.twk"), "-a", str(tmp_path / "absent.txt"))
    _refused(_run(*base, "-P", "0.5"), "cutoff P-value below 1")
    assert _run(*base, "-P", "1").stderr.count("cutoff P-value") == 0


@pytest.mark.parametrize("flags", [["-c", "2", "-C", "4"], ["-c", "1"], ["-C", "1"]])
def test_a_part_of_the_pair_space_is_refused_before_any_device_is_touched(tmp_path, flags):
    _refused(_run("clump", "-i", str(tmp_path / "absent.twk"), "-a", str(tmp_path / "absent.txt"), *flags), "the walk needs every pair")


def test_thresholds_are_checked_while_the_options_are_parsed(tmp_path):
    base = ("clump", "-i", str(tmp_path / "absent.twk"), "-a", str(tmp_path / "absent.txt"))
    _refused(_run(*base, "-1", "0.5", "-2", "0.1"), "cannot be above the secondary threshold")
    _refused(_run(*base, "-1", "1.5"), "must be a P-value in [0, 1]")
    _refused(_run(*base, "-2", "nan"), "must be a P-value in [0, 1]")
    _refused(_run("clump", "-i", str(tmp_path / "absent.twk")), "No association file specified")


def test_a_missing_association_file_is_refused_before_any_device_is_touched(tmp_path):
    _refused(_run("clump", "-i", str(tmp_path / "absent.twk"), "-a", str(tmp_path / "absent.txt")), "Failed to open the association file")


def test_a_duplicate_key_is_refused_before_any_device_is_touched(tmp_path):
    a = _assoc(tmp_path, "#contig pos P\n1\t1001\t0.5\n1 1101 1e-6 extra\n2\t1001\t0.25\n1\t1001\t0.125\n")
    r = _run("clump", "-i", str(tmp_path / "absent.twk"), "-a", a)
    _refused(r, "1:1001 is named twice")
    assert "assoc.txt:5" in r.stderr          # the line is named


@pytest.mark.parametrize("bad", ["1.5", "-0.1", "abc", "0.5x"])
def test_a_p_value_outside_0_1_is_refused_before_any_device_is_touched(tmp_path, bad):
    a = _assoc(tmp_path, f"1\t1001\t0.5\n1\t1101\tNA\n1\t1201\tnan\n1\t1301\t{bad}\n")
    r = _run("clump", "-i", str(tmp_path / "absent.twk"), "-a", a)
    _refused(r, "not a P value in [0, 1]")
    assert "assoc.txt:4" in r.stderr


def test_a_well_formed_association_file_gets_as_far_as_the_input(tmp_path):
    """NA / nan, '#' lines, spaces and further columns are all accepted: the next complaint is about the absent .twk."""
    a = _assoc(tmp_path, "#contig pos P beta\n\n1\t1001\t0.5\t0.1\n1 1101 NA\n1\t1201\tnan\n2  77   1e-8   x y z\n1\t1301\t0\n1\t1401\t1\n")
    r = _run("clump", "-i", str(tmp_path / "absent.twk"), "-a", a)
    assert r.returncode == 1 and "assoc.txt" not in r.stderr and "absent.twk" in r.stderr and r.stdout == ""


def test_header_declares_the_entry_points_and_the_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"^#define TWK_HIP_NO_CLUMP 0xFFFFFFFFu$", header, re.M)
    assert re.search(r"^int twk_hip_ld_clump\(twk_hip_ctx\* ctx, int mode, const twk_hip_filters\* filters, uint32_t a0, uint32_t n, uint32_t tile_variants,", header, re.M)
    assert re.search(r"int32_t window, uint32_t l_window, const double\* p, double p1, double p2,", header)
    assert re.search(r"uint32_t\* index_of, uint64_t\* n_clumps, uint64_t\* n_members, uint64_t\* n_edges, uint64_t\* n_pairs\);", header)
    assert re.search(r"^int twk_hip_clump_last\(const twk_hip_ctx\* ctx, double\* walk_ms, uint64_t\* bitmap_bytes\);", header, re.M)
    assert re.search(r"^#define TWK_HIP_ABI_VERSION 5$", header, re.M)
    assert re.search(r"\(still 5: twk_hip_ld_clump / twk_hip_clump_last", header)
    import tomahawk_amd as T
    lib = T.load_library()
    assert lib.twk_hip_abi_version() == 5 and hasattr(lib, "twk_hip_ld_clump") and hasattr(lib, "twk_hip_clump_last")
    # the call sequence is checked without a device: no context -> TWK_HIP_E_INVALID
    assert lib.twk_hip_ld_clump(None, 1, None, 0, 1, 0, 0, 0, None, 1e-4, 1e-2, None, None, None, None, None) == -1
    assert lib.twk_hip_clump_last(None, None, None) == -1
    assert hasattr(T.HipLd, "ld_clump") and hasattr(T.HipLd, "clump_last") and T.NO_CLUMP == 0xFFFFFFFF
    twk_ld = open(os.path.join(ROOT, "include", "twk_ld.h")).read()
    assert "bool Clump(const twk_ld_settings& settings, const twk_clump_settings& clump);" in twk_ld and "struct twk_clump_settings {" in twk_ld


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_clump_kernels_use_no_scratch_memory():
    """The clump kernels as `make hip` compiles them: the record d_pair fills is never stored (only `keep` is used) and the mask
    kernel carries one more word than prune's across its row loop, so no kernel of the clump path may have a private segment or
    spill a vector register.  Only the kernels' metadata is read."""
    seen = []
    for name, body in util.engine_kernels().items():
        if "k_ld_clump" not in name:
            continue
        assert "k_ld_prune" not in name
        seen.append(name)
        vgprs, scratch, spills = util.kernel_resources(body)
        print(name, "vgprs", vgprs, "scratch", scratch, "spills", spills)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert sum("mask" in n for n in seen) == 1 and sum("walk" in n for n in seen) == 2, seen
