"""The LD matrix, the parts that need no GPU: the `tomahawk ldmatrix` command line, the C ABI's declaration, the fill's index
arithmetic played on the host (`make matrix-check`), the matrix kernels as compiled."""
import os
import re
import subprocess

import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def test_ldmatrix_without_arguments_prints_its_usage():
    r = _run("ldmatrix")
    assert r.returncode == 1
    assert "Usage:  tomahawk ldmatrix [options] -i <in.twk> -o <PREFIX>" in r.stderr
    for flag in ("-i FILE", "-o PREFIX", "-s STRING", "-f FLOAT", "-T ", "-t INT", "-p ", "-u ", "-r FLOAT", "-w INT", "-I STRING", "-P FLOAT"):
        assert flag in r.stderr, flag
    assert re.search(r"-r FLOAT .*\(default: 0\)", r.stderr)          # not calc's 0.1 ...
    assert "calc's 0.1 would punch holes into a matrix meant for fine-mapping" in r.stderr          # ... and the usage says why
    assert re.search(r"-s STRING .*r, r2, D or Dprime \(default: r\)", r.stderr)
    assert re.search(r"-f FLOAT .*\(default: 0\)", r.stderr)
    assert "-c INT" not in r.stderr and "-C INT" not in r.stderr
    for name in ("PREFIX.npy", "PREFIX.ld", "PREFIX.variants.tsv"):
        assert name in r.stderr, name
    assert r.stdout == ""


def test_help_lists_ldmatrix_after_clump():
    r = _run()
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    at = [k for k, l in enumerate(lines) if re.match(r"\s+clump\s+\S", l)]
    assert len(at) == 1 and re.match(r"\s+ldmatrix\s+\S", lines[at[0] + 1])
    r = _run("no-such-command")
    assert r.returncode == 1 and "`ldscore`, `prune`, `clump`, `ldmatrix`" in r.stderr


def _refused(r, what):
    assert r.returncode == 1
    assert what in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr and r.stdout == ""


def _base(tmp_path):
    return ("ldmatrix", "-i", str(tmp_path / "absent.twk"), "-o", str(tmp_path / "out"))


def test_a_fisher_cutoff_is_refused_before_any_device_is_touched(tmp_path):
    """-P below 1: refused while the options are parsed - the input does not exist."""
    _refused(_run(*_base(tmp_path), "-P", "0.5"), "cutoff P-value below 1")
    assert _run(*_base(tmp_path), "-P", "1").stderr.count("cutoff P-value") == 0


@pytest.mark.parametrize("flags", [["-c", "2", "-C", "4"], ["-c", "1"], ["-C", "1"]])
def test_a_part_of_the_pair_space_is_refused_before_any_device_is_touched(tmp_path, flags):
    _refused(_run(*_base(tmp_path), *flags), "the matrix needs every pair")


@pytest.mark.parametrize("stat", ["R", "rsq", "dprime", ""])
def test_an_unknown_statistic_is_refused_while_the_options_are_parsed(tmp_path, stat):
    _refused(_run(*_base(tmp_path), "-s", stat), "Unknown statistic (-s)")


@pytest.mark.parametrize("fill", ["abc", "0.5x", ""])
def test_a_fill_that_is_no_number_is_refused_while_the_options_are_parsed(tmp_path, fill):
    _refused(_run(*_base(tmp_path), "-f", fill), "The fill value (-f) must be a number")


def test_well_formed_options_get_as_far_as_the_input(tmp_path):
    """Every statistic, a NaN fill and -T are accepted: the next complaint is about the absent .twk.  No output without -o."""
    for stat in ("r", "r2", "D", "Dprime"):
        r = _run(*_base(tmp_path), "-s", stat, "-f", "nan", "-T", "-u", "-w", "3000")
        assert r.returncode == 1 and "absent.twk" in r.stderr and "(-s)" not in r.stderr and "(-f)" not in r.stderr and r.stdout == ""
    _refused(_run("ldmatrix", "-i", str(tmp_path / "absent.twk")), "No output prefix specified")
    assert not os.path.exists(str(tmp_path / "out.npy")) and not os.path.exists(str(tmp_path / "out.variants.tsv"))


def test_header_declares_the_entry_points_and_the_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"^int twk_hip_ld_matrix\(twk_hip_ctx\* ctx, int mode, const twk_hip_filters\* filters,$", header, re.M)
    assert re.search(r"uint32_t a0, uint32_t n, uint32_t tile_variants, int32_t window, uint32_t l_window,$", header, re.M)
    assert re.search(r"int32_t stat, float fill, float\* out, uint64_t ld,$", header, re.M)
    assert re.search(r"uint64_t\* n_records, uint64_t\* n_pairs\);$", header, re.M)
    assert re.search(r"^int twk_hip_matrix_last\(const twk_hip_ctx\* ctx, double\* copy_ms, uint64_t\* matrix_bytes\);", header, re.M)
    assert re.search(r"^enum \{ TWK_HIP_STAT_R = 0, TWK_HIP_STAT_R2 = 1, TWK_HIP_STAT_D = 2, TWK_HIP_STAT_DPRIME = 3 \};$", header, re.M)
    assert re.search(r"^#define TWK_HIP_ABI_VERSION 5$", header, re.M)
    assert "THE DIAGONAL is 1.0f for R, R2 and DPRIME" in header and "the function invents none" in header
    import tomahawk_amd as T
    lib = T.load_library()
    assert lib.twk_hip_abi_version() == 5 and hasattr(lib, "twk_hip_ld_matrix") and hasattr(lib, "twk_hip_matrix_last")
    # the call sequence is checked without a device: no context -> TWK_HIP_E_INVALID
    assert lib.twk_hip_ld_matrix(None, 1, None, 0, 1, 0, 0, 0, 0, 0.0, None, 1, None, None) == -1
    assert lib.twk_hip_matrix_last(None, None, None) == -1
    assert hasattr(T.HipLd, "ld_matrix") and hasattr(T.HipLd, "matrix_last")
    assert (T.STAT_R, T.STAT_R2, T.STAT_D, T.STAT_DPRIME) == (0, 1, 2, 3)
    twk_ld = open(os.path.join(ROOT, "include", "twk_ld.h")).read()
    assert "bool Matrix(const twk_ld_settings& settings, const twk_matrix_settings& matrix);" in twk_ld and "struct twk_matrix_settings {" in twk_ld


def test_index_arithmetic_of_the_fill_played_on_the_host():
    """`make matrix-check`: every lane of every block of every launch of the listed geometries through the kernel's own slot arithmetic
    and guards (csrc/hip/ld_matrix_index.h), built with plain g++ - every off-diagonal entry of the slice written exactly once from
    each side, nothing outside it touched, the transposed write-out free of bank conflicts and in runs of consecutive floats."""
    r = subprocess.run(["make", "-C", ROOT, "matrix-check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(r"^matrix-check: (\d+) cases, 0 bad$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 7, r.stdout[-2000:]
    for case in ("n=203 a0=37 tiles of 128", "n=300 a0=0 one tile of 384", "n=64 ", "n=65 ", "n=1 ", "regrouped n=140"):
        assert re.search(r"^\s+" + re.escape(case) + r".*\bok$", r.stdout, re.M), case
    assert "BAD" not in r.stdout
    # the header the program includes is the one the kernel includes, and it has no HIP in it
    index = open(os.path.join(ROOT, "tomahawk_amd", "csrc", "hip", "ld_matrix_index.h")).read()
    assert "hip_runtime" not in index and "__global__" not in index
    assert '#include "ld_matrix_index.h"' in open(os.path.join(ROOT, "tomahawk_amd", "csrc", "hip", "ld_matrix.hip.h")).read()
    assert '#include "../hip/ld_matrix_index.h"' in open(os.path.join(ROOT, "tomahawk_amd", "csrc", "tools", "matrix_index_check.cpp")).read()


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_matrix_kernels_use_no_scratch_memory():
    """The matrix kernels as `make hip` compiles them: the pair runs out of line and returns its statistic in two registers, so no
    kernel of the matrix path may have a private segment or spill a vector register; there is one fill kernel; and the score, prune
    and clump kernels are still there under their names.  Only the kernels' metadata is read."""
    seen, others = [], set()
    for name, body in util.engine_kernels().items():
        for k in ("k_ld_score", "k_ld_prune", "k_ld_clump"):
            if k in name:
                others.add(name)
        if "k_ld_matrix" not in name:
            continue
        seen.append(name)
        vgprs, scratch, spills = util.kernel_resources(body)
        print(name, "vgprs", vgprs, "scratch", scratch, "spills", spills)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert sum("k_ld_matrix_fill" in n for n in seen) == 1 and sum("k_ld_matrix_diag" in n for n in seen) == 1 and len(seen) == 2, seen
    # (the mangled names carry the kernels' parameter types: nothing of the three older paths was renamed or re-typed)
    assert others == {"_ZN3twk10k_ld_scoreEPKNS_9ScoreArgsE", "_ZN3twk15k_ld_score_foldEPKdPKjjjmmjS3_jPdPy",
                      "_ZN3twk15k_ld_prune_maskEPKNS_9PruneArgsE", "_ZN3twk15k_ld_prune_walkILb1EEEvPKyjjjPyPhS3_", "_ZN3twk15k_ld_prune_walkILb0EEEvPKyjjjPyPhS3_",
                      "_ZN3twk15k_ld_clump_maskEPKNS_9ClumpArgsE", "_ZN3twk15k_ld_clump_walkILb1EEEvPKyjjjPKjjPyPjS5_", "_ZN3twk15k_ld_clump_walkILb0EEEvPKyjjjPKjjPyPjS5_"}, sorted(others)
