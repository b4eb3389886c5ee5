"""Sample subsets, the parts that need no GPU: the selection kernel's table, compress and split played on the host (`make subset-check`),
and the resolution of `--keep` / `--remove` against a header's sample names (csrc/host/twk_sample_list.h through hostlib)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [f"S{i}" for i in range(12)]


def test_selection_table_compress_and_split_against_a_field_by_field_gather():
    """`make subset-check`: csrc/hip/ld_subset_index.h built with g++ under AddressSanitizer and UBSan - every block and lane of the
    split by output words against a gather that moves one 2-bit field at a time, for source sizes 1 .. 5000 and the keep lists
    everything / one sample / every second / runs / random densities: every output word stored exactly once (write counts with a
    border), the padding zero, nothing ORed outside a block's window."""
    r = subprocess.run(["make", "-C", ROOT, "subset-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.search(r"subset-check: (\d+) cases, (\d+) bad", r.stdout)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) == 0, r.stdout[-2000:]


def write(tmp_path, name, text):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def test_keep_only(tmp_path):
    keep = write(tmp_path, "keep.txt", "S7\nS2\nS11\n")          # the file's order does not matter: header order comes out
    got = hostlib.resolve_samples(NAMES, keep=keep)
    assert got.dtype == np.uint32 and got.tolist() == [2, 7, 11]


def test_remove_only(tmp_path):
    remove = write(tmp_path, "remove.txt", "S0\nS5\n")
    assert hostlib.resolve_samples(NAMES, remove=remove).tolist() == [1, 2, 3, 4, 6, 7, 8, 9, 10, 11]


def test_keep_then_remove(tmp_path):
    keep = write(tmp_path, "keep.txt", "S1\nS2\nS3\nS4\n")
    remove = write(tmp_path, "remove.txt", "S3\nS9\n")           # S9 is in the header and not kept: removing it changes nothing
    assert hostlib.resolve_samples(NAMES, keep=keep, remove=remove).tolist() == [1, 2, 4]


def test_neither_option_keeps_everything():
    assert hostlib.resolve_samples(NAMES).tolist() == list(range(12))


def test_comments_blank_lines_and_line_ends(tmp_path):
    keep = write(tmp_path, "keep.txt", "# a population\n\nS3\r\n   \n  S4  \n#S5\nS6")
    assert hostlib.resolve_samples(NAMES, keep=keep).tolist() == [3, 4, 6]


def test_a_name_that_is_not_in_the_header_is_named(tmp_path):
    keep = write(tmp_path, "keep.txt", "S1\nNA12878\nNA12879\n")
    with pytest.raises(ValueError, match=r'"NA12878".*line 2.*not in the input\'s header'):
        hostlib.resolve_samples(NAMES, keep=keep)
    with pytest.raises(ValueError, match=r'"NA12878".*--remove'):
        hostlib.resolve_samples(NAMES, remove=keep)


def test_a_name_twice_in_one_file(tmp_path):
    keep = write(tmp_path, "keep.txt", "S1\nS2\nS1\n")
    with pytest.raises(ValueError, match=r'"S1" is listed twice.*line 3'):
        hostlib.resolve_samples(NAMES, keep=keep)
    # ... the same name in both files is keep, then remove: no error
    assert hostlib.resolve_samples(NAMES, keep=write(tmp_path, "k.txt", "S1\nS2\n"), remove=write(tmp_path, "r.txt", "S1\n")).tolist() == [2]


def test_an_unreadable_file(tmp_path):
    with pytest.raises(ValueError, match=r"Cannot read the sample list \(--keep\)"):
        hostlib.resolve_samples(NAMES, keep=str(tmp_path / "nothing-here.txt"))
    with pytest.raises(ValueError, match=r"Cannot read the sample list \(--remove\)"):
        hostlib.resolve_samples(NAMES, remove=str(tmp_path / "nothing-here.txt"))


def test_an_empty_result(tmp_path):
    with pytest.raises(ValueError, match="No sample is left"):
        hostlib.resolve_samples(NAMES, keep=write(tmp_path, "k.txt", "S1\n"), remove=write(tmp_path, "r.txt", "S1\n"))
    with pytest.raises(ValueError, match="No sample is left"):
        hostlib.resolve_samples(NAMES, keep=write(tmp_path, "empty.txt", "# nobody\n"))


def test_the_cli_refuses_a_bad_list_before_any_device_work(tmp_path):
    """No GPU here: a command that got as far as the device would fail with the device's error, not with the list's."""
    twk = str(tmp_path / "in.twk")
    al = (np.random.default_rng(1).random((20, 12, 2)) < 0.3).astype(np.int8)
    hostlib.write_twk(twk, al, 1000 + 100 * np.arange(20), np.zeros(20, np.uint32), phased=np.ones(20, np.uint8), n_contigs=1, block_size=10)
    keep = write(tmp_path, "keep.txt", "S1\nNOBODY\n")
    for cmd in (["ldscore"], ["calc", "-o", str(tmp_path / "out")], ["prune"], ["relationship"], ["scalc", "-I", "1:1500", "-o", str(tmp_path / "s")]):
        r = subprocess.run([hostlib.CLI_PATH, cmd[0], "-i", twk, "--keep", keep] + cmd[1:], capture_output=True, text=True)
        assert r.returncode == 1 and '[ERROR]' in r.stderr and 'Sample "NOBODY"' in r.stderr and "HIP" not in r.stderr, (cmd, r.stderr)
