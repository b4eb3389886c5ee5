"""The sample relationship matrix, the parts that need no GPU: the `tomahawk relationship` command line, the C ABI's declaration, the
index header played on the host (`make relate-check`), the transposition and epilogue kernels as compiled."""
import os
import re
import subprocess

import pytest

from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def test_relationship_without_arguments_prints_its_usage():
    r = _run("relationship")
    assert r.returncode == 1
    assert "Usage:  tomahawk relationship -i <in.twk> [-I interval ...] [-s ibs|ibs0|king] [-f fill] [-o PREFIX [-T]]" in r.stderr
    for flag in ("-i FILE", "-I STRING", "-s STRING", "-f FLOAT", "-o PREFIX", "-T ", "-t INT"):
        assert flag in r.stderr, flag
    assert re.search(r"-s STRING .*ibs, ibs0 or king \(default: king\)", r.stderr)
    assert re.search(r"-f FLOAT .*\(default: nan\)", r.stderr)
    for formula in ("(n + ibs2 - ibs0) / (2 n)", "ibs0 / n", "(hethet - 2 ibs0) / (het_a + het_b)"):
        assert formula in r.stderr, formula
    # the reference's command of the same name is not reproduced, and the usage says so
    assert "The reference's `relationship` is not reproduced" in r.stderr
    for name in ("PREFIX.npy", "PREFIX.tsv", "PREFIX.samples.tsv"):
        assert name in r.stderr, name
    for flag in ("-p ", "-u ", "-r FLOAT", "-w INT", "-c INT", "-C INT", "-P FLOAT"):
        assert flag not in r.stderr, flag
    assert r.stdout == ""


def test_help_and_the_illegal_command_line_name_relationship():
    r = _run()
    assert r.returncode == 1
    lines = r.stderr.splitlines()
    at = [k for k, l in enumerate(lines) if re.match(r"\s+relationship\s+\S", l)]
    assert len(at) == 1 and re.match(r"\s+scalc\s+\S", lines[at[0] - 1])
    r = _run("no-such-command")
    assert r.returncode == 1 and "`scalc`, `relationship`, `ldscore`" in r.stderr


def _refused(r, what):
    assert r.returncode == 1
    assert what in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr and r.stdout == ""
    assert len([l for l in r.stderr.splitlines() if "ERROR" in l]) == 1          # one line each


@pytest.mark.parametrize("flags,what", [(["-p"], "(-p)"), (["-u"], "(-u)"), (["-r", "0.2"], "(-r)"), (["-w", "1000"], "(-w)"),
                                        (["-c", "3"], "(-c)"), (["-C", "1"], "(-C)"), (["-P", "1"], "(-P)"), (["-P", "0.5"], "(-P)")])
def test_flags_without_a_meaning_here_are_refused_before_any_device_or_input_is_touched(tmp_path, flags, what):
    """The input does not exist: the refusal comes while the options are parsed."""
    _refused(_run("relationship", "-i", str(tmp_path / "absent.twk"), *flags), what)


@pytest.mark.parametrize("flags,what", [(["-s", "KING"], "Unknown statistic (-s)"), (["-s", "ibs1"], "Unknown statistic (-s)"), (["-s", ""], "Unknown statistic (-s)"),
                                        (["-f", "abc"], "The fill value (-f) must be a number"), (["-f", "0.5x"], "The fill value (-f) must be a number"),
                                        (["-T"], "-T names the file written for -o PREFIX")])
def test_malformed_options_are_refused_while_the_options_are_parsed(tmp_path, flags, what):
    _refused(_run("relationship", "-i", str(tmp_path / "absent.twk"), *flags), what)


def test_well_formed_options_get_as_far_as_the_input(tmp_path):
    for stat in ("ibs", "ibs0", "king"):
        r = _run("relationship", "-i", str(tmp_path / "absent.twk"), "-s", stat, "-f", "nan", "-I", "1:100-200", "-o", str(tmp_path / "out"), "-T")
        assert r.returncode == 1 and "absent.twk" in r.stderr and "(-s)" not in r.stderr and "(-f)" not in r.stderr and r.stdout == ""
    r = _run("relationship", "-i", str(tmp_path / "absent.twk"), "-f", "-7")
    assert r.returncode == 1 and "absent.twk" in r.stderr and "(-f)" not in r.stderr
    assert not os.path.exists(str(tmp_path / "out.npy")) and not os.path.exists(str(tmp_path / "out.samples.tsv"))


def test_header_declares_the_entry_points_and_the_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"^typedef struct \{ uint32_t n, ibs0, ibs2, hethet, het_a, het_b; \} twk_hip_rel_counts;$", header, re.M)
    assert re.search(r"^int twk_hip_relationship\(twk_hip_ctx\* ctx,$", header, re.M)
    assert re.search(r"^\s+const uint32_t\* variants, uint32_t n_use,", header, re.M)
    assert re.search(r"^\s+uint32_t sA0, uint32_t nSA, uint32_t sB0, uint32_t nSB,", header, re.M)
    assert re.search(r"^\s+int32_t stat, double fill,$", header, re.M)
    assert re.search(r"^\s+double\* out, uint64_t ld,", header, re.M) and re.search(r"^\s+twk_hip_rel_counts\* counts, uint64_t ld_counts,", header, re.M)
    assert re.search(r"^\s+uint64_t\* n_sample_pairs\);$", header, re.M)
    assert re.search(r"^int twk_hip_relationship_last\(const twk_hip_ctx\* ctx, int32_t\* planes_per_sample, double\* transpose_ms, uint64_t\* plane_bytes\);$", header, re.M)
    assert re.search(r"^enum \{ TWK_HIP_REL_IBS = 0, TWK_HIP_REL_IBS0 = 1, TWK_HIP_REL_KING = 2 \};$", header, re.M)
    assert re.search(r"^#define TWK_HIP_ABI_VERSION 5$", header, re.M)
    assert "(still 5: twk_hip_relationship / twk_hip_relationship_last" in header
    assert "The reference's `relationship` (lib/relationship.h) is NOT reproduced" in header
    import tomahawk_amd as T
    lib = T.load_library()
    assert lib.twk_hip_abi_version() == 5 and hasattr(lib, "twk_hip_relationship") and hasattr(lib, "twk_hip_relationship_last")
    # the call sequence is checked without a device: no context -> TWK_HIP_E_INVALID
    assert lib.twk_hip_relationship(None, None, 0, 0, 1, 0, 1, 2, 0.0, None, 0, None, 0, None) == -1
    assert lib.twk_hip_relationship_last(None, None, None, None) == -1
    assert hasattr(T.HipLd, "relationship") and hasattr(T.HipLd, "relationship_last")
    assert (T.REL_IBS, T.REL_IBS0, T.REL_KING) == (0, 1, 2) and T.REL_COUNTS_DTYPE.itemsize == 24
    assert T.REL_COUNTS_DTYPE.names == ("n", "ibs0", "ibs2", "hethet", "het_a", "het_b")
    twk_ld = open(os.path.join(ROOT, "include", "twk_ld.h")).read()
    assert "bool Relationship(const twk_ld_settings& settings, const twk_relationship_settings& rel);" in twk_ld and "struct twk_relationship_settings {" in twk_ld


def test_index_header_played_on_the_host():
    """`make relate-check`: the transposition lane by lane against a naive one (every live word written once, padding bits and rows zero, the
    last partial word right), the counts from plane products against counted genotypes, every lane of the epilogue over a count matrix that
    holds only the tiles on or above the diagonal - built with g++ -fsanitize=address,undefined and run as a stand-alone program."""
    r = subprocess.run(["make", "-C", ROOT, "relate-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "-fsanitize=address,undefined" in r.stdout
    m = re.search(r"^relate-check: (\d+) cases, 0 bad$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 12, r.stdout[-2000:]
    for case, planes in (("1 x 1", 2), ("2 x 1", 2), ("3 x 63", 2), ("17 x 64", 2), ("16 x 65", 2), ("43 x 1023 missing", 3), ("44 x 1024 missing", 3),
                         ("64 x 1024", 2), ("129 x 1025", 2), ("300 x 2100 missing", 3), ("300 x 1000 of 3100 from 37 by 3 missing", 3),
                         ("40 x 30 of 90 from 0 by 3: no missing left", 2)):
        assert re.search(r"^\s+" + re.escape(case) + r"\s+P=%d .*\bok$" % planes, r.stdout, re.M), case
    assert "BAD" not in r.stdout + r.stderr
    # 43 samples x 3 planes = 129 rows: two tiles (+ the overhang tile); 64 x 2 = 128: exactly one
    assert re.search(r"^\s+43 x 1023 missing\s+P=3 W=32 rows=384 ", r.stdout, re.M) and re.search(r"^\s+64 x 1024\s+P=2 W=32 rows=256 ", r.stdout, re.M)
    # the header the program includes is the one the kernels and the engine's host code include, and it has no HIP in it
    hip_dir = os.path.join(ROOT, "tomahawk_amd", "csrc", "hip")
    index = open(os.path.join(hip_dir, "ld_relate_index.h")).read()
    assert "hip_runtime" not in index and "__global__" not in index
    assert '#include "ld_relate_index.h"' in open(os.path.join(hip_dir, "ld_relate.hip.h")).read()
    assert '#include "ld_relate.hip.h"' in open(os.path.join(hip_dir, "twk_hip.hip")).read()
    assert '#include "../hip/ld_relate_index.h"' in open(os.path.join(ROOT, "tomahawk_amd", "csrc", "tools", "relate_index_check.cpp")).read()


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_relate_kernels_use_no_scratch_memory():
    """The transposition and the epilogue as `make hip` compiles them, from the code object's metadata alone: no private segment, no spilled
    vector register; one kernel of each; and the count kernel they share with the variant paths is still there under its name."""
    seen = {}
    for name, body in util.engine_kernels().items():
        if "k_relate" in name:
            seen[name] = util.kernel_resources(body)
            print(name, "vgprs %d scratch %d spills %d" % seen[name])
    assert sum("k_relate_transpose" in n for n in seen) == 1 and sum("k_relate_epilogue" in n for n in seen) == 1 and len(seen) == 2, sorted(seen)
    for name, (vgprs, scratch, spills) in seen.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert vgprs <= 128, (name, vgprs)          # (four waves a SIMD: neither kernel has a reason to hold more)
    assert any("k_count_list_t" in n for n in util.engine_kernels())
