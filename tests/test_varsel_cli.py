"""Variant subsets, the parts that need no GPU: the ABI's declarations and exports, the predicate and the row gather's walk played on the
host (`make varsel-check`), the resolution of `--extract` / `--exclude` list files against a set of variants
(csrc/host/twk_variant_list.h through hostlib), and the commands' refusals that come before any device work."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["twk_hip_select_variants", "twk_hip_variant_selection", "twk_hip_variant_map", "twk_hip_select_variants_last"]


def test_the_header_declares_the_entry_points_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"#define\s+TWK_HIP_ABI_VERSION\s+5\b", text)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    m = re.search(r"typedef struct \{([^}]*)\} twk_hip_variant_filter;", text)
    assert m and [f for f in re.findall(r"\b(min_maf|max_maf|min_mac|_pad|max_missing|min_hwe)\b", m.group(1))] == ["min_maf", "max_maf", "min_mac", "_pad", "max_missing", "min_hwe"]
    # behind the sample-subset section, before the compute entry points
    assert text.index("twk_hip_select_last(") < text.index("twk_hip_select_variants(") < text.index("/* ---- compute")


def test_the_library_exports_the_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "tomahawk_amd", "lib", "libtwk_hip.so"))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    assert hasattr(hostlib.lib(), "twk_resolve_variants")


def test_predicate_and_gather_walk_against_their_restatements():
    """`make varsel-check`: csrc/hip/ld_varsel_index.h built with g++ under AddressSanitizer and UBSan - the predicate against a
    restatement with the equality boundary of every threshold, the word counts against a sample-by-sample loop, every block and lane of
    the row gather against a row-by-row copy and an array of write counts with a border."""
    r = subprocess.run(["make", "-C", ROOT, "varsel-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(r"varsel-check: (\d+) gather cases, (\d+) bad", r.stdout)
    assert m and int(m.group(1)) >= 100 and int(m.group(2)) == 0, r.stdout[-2000:]
    assert re.search(r"predicate: \d+ random cases and the boundaries, 0 bad", r.stdout)


# ---- the list-file resolver -----------------------------------------------------------------------------------------------------------------
CONTIGS = ["1", "2", "HLA:A"]
RID = np.array([0, 0, 0, 0, 0, 1, 1, 1, 2, 2], dtype=np.uint32)
POS = np.array([999, 1099, 1099, 1199, 1299, 999, 1099, 1199, 49, 59], dtype=np.uint32)          # stored: the commands print pos + 1


def write(tmp_path, name, text):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_both_line_forms(tmp_path):
    ids, absent = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", "1:1000\n2\t1100\n1 1300\n2:1200\n"))
    assert ids.dtype == np.uint32 and ids.tolist() == [0, 4, 6, 7] and absent == 0          # ascending, whatever the file's order


def test_comments_blank_lines_line_ends_and_extra_columns(tmp_path):
    text = "# a list\n\n#contig\tpos\tkeep\n1\t1000\t1\n   \n  1:1200  \r\n2\t1000\t0.25\tmore columns\n1:1300 trailing words\n"
    ids, absent = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", text))
    assert ids.tolist() == [0, 3, 4, 5] and absent == 0


def test_a_contig_name_with_a_colon_takes_the_last_one(tmp_path):
    ids, _ = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", "HLA:A:50\nHLA:A\t60\n"))
    assert ids.tolist() == [8, 9]


def test_a_contig_pos_line_with_a_numeric_further_column(tmp_path):
    """`1:1000 1` reads both ways - CONTIG:POS with a keep flag behind it, or the contig "1:1000" at position 1: the header's contig names
    settle it, and the whole first column wins where it names a contig itself."""
    ids, absent = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", "1:1000 1\n2:1100\t0\tmore\nHLA:A 50\n"))
    assert ids.tolist() == [0, 6, 8] and absent == 0
    ids, absent = hostlib.resolve_variants(["1", "1:1000"], np.array([0, 1], np.uint32), np.array([999, 0], np.uint32), write(tmp_path, "m.txt", "1:1000 1\n"))
    assert ids.tolist() == [1] and absent == 0
    ids, absent = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "n.txt", "7:1000 1\n"))
    assert ids.tolist() == [] and absent == 1


def test_every_variant_at_a_listed_position_matches_and_a_position_twice_counts_once(tmp_path):
    ids, absent = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", "1:1100\n1\t1100\n"))
    assert ids.tolist() == [1, 2] and absent == 0


def test_absent_positions_are_counted(tmp_path):
    ids, absent = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", "1:1000\n1:7\n1:7\n3:1000\nX\t5\n2:1101\n"))
    assert ids.tolist() == [0] and absent == 4          # 1:7 once, the unknown contigs 3 and X, 2:1101


def test_an_empty_list_matches_nothing(tmp_path):
    ids, absent = hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", "# nothing\n"))
    assert ids.tolist() == [] and absent == 0


@pytest.mark.parametrize("line", ["rs12345", "1:", ":1000", "1:10x0", "1\tabc", "1:-5", "1:12345678901234567890"])
def test_an_unparsable_line_is_named(tmp_path, line):
    with pytest.raises(ValueError, match=r"line 3 of the variant list"):
        hostlib.resolve_variants(CONTIGS, RID, POS, write(tmp_path, "l.txt", "1:1000\n# fine so far\n" + line + "\n1:1100\n"))


def test_an_unreadable_file(tmp_path):
    with pytest.raises(ValueError, match=r"Cannot read the variant list"):
        hostlib.resolve_variants(CONTIGS, RID, POS, str(tmp_path / "nothing-here.txt"))


# ---- the commands, as far as they go without a device -----------------------------------------------------------------------------------------
def test_the_cli_refuses_bad_lists_and_thresholds_before_any_device_work(tmp_path):
    """No GPU here: a command that got as far as the device would fail with the device's error, not with the option's."""
    twk = str(tmp_path / "in.twk")
    al = (np.random.default_rng(1).random((20, 12, 2)) < 0.3).astype(np.int8)
    hostlib.write_twk(twk, al, 1000 + 100 * np.arange(20), np.zeros(20, np.uint32), phased=np.ones(20, np.uint8), n_contigs=1, block_size=10)
    bad = write(tmp_path, "bad.txt", "1:1001\nnot a position\n")
    assoc = write(tmp_path, "assoc.txt", "1\t1001\t0.5\n")
    commands = (["ldscore"], ["calc", "-o", str(tmp_path / "out")], ["prune"], ["clump", "-a", assoc], ["ldmatrix", "-o", str(tmp_path / "m")], ["lddecay"],
                ["ldaggregate"], ["relationship"], ["scalc", "-I", "1:1500", "-o", str(tmp_path / "s")])
    for cmd in commands:
        for option in ("--extract", "--exclude"):
            r = subprocess.run([hostlib.CLI_PATH, cmd[0], "-i", twk, option, bad] + cmd[1:], capture_output=True, text=True)
            assert r.returncode == 1 and "[ERROR]" in r.stderr and "line 2 of the variant list (" + option in r.stderr and "HIP" not in r.stderr, (cmd, r.stderr)
        for args, needle in ((["--maf", "0.6"], "--maf"), (["--max-maf", "-1"], "--max-maf"), (["--mac", "-3"], "--mac"), (["--mac", "1.5"], "--mac"), (["--mac", "1e3"], "--mac"),
                             (["--geno", "1.5"], "--geno"),
                             (["--hwe", "nan"], "--hwe")):
            r = subprocess.run([hostlib.CLI_PATH, cmd[0], "-i", twk] + cmd[1:] + args, capture_output=True, text=True)
            assert r.returncode == 1 and needle in r.stderr and "HIP" not in r.stderr, (cmd, args, r.stderr)


def test_window_mode_over_several_gpus_refuses_the_options_before_any_device_is_touched(tmp_path):
    """Every GPU of a windowed multi-GPU run holds its own band and halo: no one context holds the variant set.  No GPU here either: the
    refusal must come before a device is asked for."""
    twk = str(tmp_path / "in.twk")
    al = (np.random.default_rng(2).random((30, 12, 2)) < 0.3).astype(np.int8)
    hostlib.write_twk(twk, al, 1000 + 100 * np.arange(30), np.zeros(30, np.uint32), phased=np.ones(30, np.uint8), n_contigs=1, block_size=10)
    for env in ({"TWK_HIP_GPUS": "2"}, {"TWK_HIP_PART": "0/2"}):
        r = subprocess.run([hostlib.CLI_PATH, "calc", "-i", twk, "-o", str(tmp_path / "out"), "-w", "1000", "--maf", "0.1"], capture_output=True, text=True,
                           env=dict(os.environ, **env))
        assert r.returncode == 1 and "need one context that holds the command's whole variant set" in r.stderr and "[ERROR][HIP]" not in r.stderr, (env, r.stderr)
