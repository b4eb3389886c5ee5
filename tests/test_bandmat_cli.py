"""The banded LD matrix, the parts that need no GPU: `tomahawk ldmatrix --band`'s option handling, the C ABI's declaration, the layout
and the fill's index arithmetic played on the host (`make bandmat-check`), the band kernels as compiled, the NumPy helpers."""
import os
import re
import subprocess

import numpy as np
import pytest

import tomahawk_amd as T
from tests import util
from tomahawk_amd import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([hostlib.CLI_PATH] + list(args), capture_output=True, text=True, timeout=120)


def _refused(r, what):
    assert r.returncode == 1
    assert what in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Unpacking" not in r.stderr and "absent.twk" not in r.stderr and r.stdout == ""


def _base(tmp_path, command="ldmatrix"):
    return (command, "-i", str(tmp_path / "absent.twk"), "-o", str(tmp_path / "out"))


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_band_without_a_window_is_refused_before_the_input_is_opened(tmp_path):
    _refused(_run(*_base(tmp_path), "--band"), "--band stores the columns inside the window: it needs one (-w)")
    _refused(_run(*_base(tmp_path), "--band", "-u", "-s", "r2"), "it needs one (-w)")


def test_band_as_text_is_refused_before_the_input_is_opened(tmp_path):
    _refused(_run(*_base(tmp_path), "--band", "-w", "1000", "-T"), "--band has no text form (-T)")
    _refused(_run(*_base(tmp_path), "-T", "-w", "1000", "--band"), "--band has no text form (-T)")


def test_band_with_a_window_gets_as_far_as_the_input(tmp_path):
    for extra in ([], ["-u", "-s", "Dprime", "-f", "nan"], ["--windowBases=1000"]):
        r = _run(*_base(tmp_path), "--band", "-w", "1000", *extra)
        assert r.returncode == 1 and "absent.twk" in r.stderr and "--band" not in r.stderr and r.stdout == "", r.stderr
    for name in ("out.values.npy", "out.indptr.npy", "out.first.npy", "out.variants.tsv", "out.npy"):
        assert not os.path.exists(str(tmp_path / name))


@pytest.mark.parametrize("command", ["prune", "ldscore", "clump", "lddecay"])
def test_band_belongs_to_ldmatrix_alone(tmp_path, command):
    r = _run(*_base(tmp_path, command), "--band", "-w", "1000")
    assert r.returncode == 1 and "Unrecognized option: --band" in r.stderr and "absent.twk" not in r.stderr
    # the usage text is pinned by the recorded transcript: --band is not in it; and the long names next to it still resolve
    r = _run("ldmatrix")
    assert r.returncode == 1 and "Usage:  tomahawk ldmatrix [options] -i <in.twk> -o <PREFIX>" in r.stderr and "--band" not in r.stderr
    r = _run("lddecay", "-i", str(tmp_path / "absent.twk"), "--bins", "10")
    assert r.returncode == 1 and "absent.twk" in r.stderr and "ambiguous" not in r.stderr


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_abi_version_is_unchanged():
    header = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"^int twk_hip_bandmat_layout\(twk_hip_ctx\* ctx, uint32_t a0, uint32_t n, uint32_t l_window, uint32_t\* first, uint64_t\* row_ptr\);$", header, re.M)
    assert re.search(r"^int twk_hip_ld_matrix_band\(twk_hip_ctx\* ctx, int mode, const twk_hip_filters\* filters,$", header, re.M)
    assert re.search(r"int32_t stat, float fill, float\* values, uint64_t capacity, uint32_t\* first, uint64_t\* row_ptr,$", header, re.M)
    assert re.search(r"^int twk_hip_bandmat_last\(const twk_hip_ctx\* ctx, double\* copy_ms, uint64_t\* band_bytes\);$", header, re.M)
    assert re.search(r"^#define TWK_HIP_ABI_VERSION 5$", header, re.M)
    assert re.search(r"\(still 5: twk_hip_bandmat_layout / twk_hip_ld_matrix_band / twk_hip_bandmat_last", header)
    lib = T.load_library()
    assert lib.twk_hip_abi_version() == 5
    for name in ("twk_hip_bandmat_layout", "twk_hip_ld_matrix_band", "twk_hip_bandmat_last"):
        assert hasattr(lib, name), name
    # the call sequence is checked without a device: no context -> TWK_HIP_E_INVALID
    assert lib.twk_hip_bandmat_layout(None, 0, 1, 1000, None, None) == -1
    assert lib.twk_hip_ld_matrix_band(None, 1, None, 0, 1, 0, int(T.OPT_WINDOW), 1000, 0, 0.0, None, 0, None, None, None, None) == -1
    assert lib.twk_hip_bandmat_last(None, None, None) == -1
    for name in ("bandmat_layout", "ld_matrix_band", "bandmat_last"):
        assert hasattr(T.HipLd, name), name
    twk_ld = open(os.path.join(ROOT, "include", "twk_ld.h")).read()
    assert re.search(r"struct twk_matrix_settings \{[^}]*\bbool band = false;", twk_ld)


# ---- the index arithmetic ----------------------------------------------------------------------------------------------------------------
def test_layout_and_index_arithmetic_played_on_the_host():
    """`make bandmat-check`: the layout against its O(n^2) definition, then every lane of every block of every launch of the listed
    geometries through the kernel's own slot arithmetic, guards and dead-block test (csrc/hip/ld_bandmat_index.h), under
    AddressSanitizer and UBSan."""
    r = subprocess.run(["make", "-C", ROOT, "bandmat-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "-fsanitize=address,undefined -fno-sanitize-recover=undefined" in r.stdout
    m = re.search(r"^bandmat-check: (\d+) cases, 0 bad$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 15, r.stdout[-3000:]
    for case in ("n=203 a0=37 tiles of 128", "n=300 band narrower than a wave (+-20)", "n=700 band wider than a column block (+-300)",
                 "three contigs of 97, 105 and 98 variants", "clustered and duplicated positions", "gaps wider than the window (rows of length 1)",
                 "window 0", "window beyond the span", "n=1 ", "n=64 ", "n=65 ", "regrouped n=140", "unsorted positions and contigs are refused"):
        assert re.search(r"^\s+" + re.escape(case) + r".*\bok$", r.stdout, re.M), case
    assert "BAD" not in r.stdout
    # a dead block is met where the band is narrow, and none where the band is the dense matrix
    assert re.search(r"band narrower than a wave \(\+-20\), tiles of 128 .* [1-9]\d* dead blocks  ok$", r.stdout, re.M)
    assert re.search(r"window beyond the span.* 0 dead blocks  ok$", r.stdout, re.M)
    # the header the program includes is the one the kernel includes, and it has no HIP in it
    hip_dir = os.path.join(ROOT, "tomahawk_amd", "csrc", "hip")
    index = open(os.path.join(hip_dir, "ld_bandmat_index.h")).read()
    assert "hip_runtime" not in index and "__global__" not in index
    assert '#include "ld_bandmat_index.h"' in open(os.path.join(hip_dir, "ld_bandmat.hip.h")).read()
    assert '#include "../hip/ld_bandmat_index.h"' in open(os.path.join(ROOT, "tomahawk_amd", "csrc", "tools", "bandmat_index_check.cpp")).read()


# ---- the kernels as compiled ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_bandmat_kernels_use_no_scratch_memory():
    """The band kernels as `make hip` compiles them: no private segment, no spilled vector register, one fill kernel and one diagonal
    kernel; the fill kernel's allocation lets a SIMD hold three waves (168 VGPRs in granules of 8).  Only the metadata is read."""
    seen = {n: util.kernel_resources(b) for n, b in util.engine_kernels().items() if "k_ld_bandmat" in n}
    for name, (vgprs, scratch, spills) in seen.items():
        print(name, "vgprs", vgprs, "scratch", scratch, "spills", spills)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert sum("k_ld_bandmat_fill" in n for n in seen) == 1 and sum("k_ld_bandmat_diag" in n for n in seen) == 1 and len(seen) == 2, sorted(seen)
    (fill_vgprs,) = (v[0] for n, v in seen.items() if "k_ld_bandmat_fill" in n)
    assert -(-fill_vgprs // 8) * 8 <= 168
    assert not any("k_ld_matrix" in n for n in seen)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"k_ld_bandmat_fill[^\n]*\b%d VGPRs" % fill_vgprs, design), fill_vgprs


# ---- the NumPy helpers ---------------------------------------------------------------------------------------------------------------------
def test_band_to_dense_and_band_to_csr_on_a_hand_made_band():
    # 4 variants with the symmetric bands {0, 1}, {0, 1, 2}, {1, 2} and {3}
    first = np.array([0, 0, 1, 3], dtype=np.uint32)
    indptr = np.array([0, 2, 5, 7, 8], dtype=np.uint64)
    values = np.array([1.0, 0.5, 0.5, 1.0, -0.25, -0.25, 1.0, 1.0], dtype=np.float32)
    data, indices, ptr = T.band_to_csr(values, first, indptr)
    assert data.dtype == np.float32 and np.array_equal(data, values)
    assert indices.dtype == np.int64 and indices.tolist() == [0, 1, 0, 1, 2, 1, 2, 3]
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 2, 5, 7, 8]
    dense = T.band_to_dense(values, first, indptr, fill=-2.0)
    want = np.array([[1.0, 0.5, -2, -2], [0.5, 1.0, -0.25, -2], [-2, -0.25, 1.0, -2], [-2, -2, -2, 1.0]], dtype=np.float32)
    assert dense.dtype == np.float32 and np.array_equal(dense, want)
    assert np.isnan(T.band_to_dense(values, first, indptr, fill=float("nan"))[0, 3])
    assert T.band_to_dense(values, first, indptr)[0, 2] == 0.0
    # the CSR arrays multiply like the dense matrix with zeros outside the band
    x = np.array([1.0, 2.0, 3.0, 4.0])
    y = np.zeros(4)
    np.add.at(y, np.repeat(np.arange(4), np.diff(ptr)), data.astype(np.float64) * x[indices])
    assert np.allclose(y, T.band_to_dense(values, first, indptr, fill=0.0).astype(np.float64) @ x)
    # an empty band and arrays that do not belong together
    d0, i0, p0 = T.band_to_csr(np.zeros(0, np.float32), np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    assert len(d0) == 0 and len(i0) == 0 and p0.tolist() == [0] and T.band_to_dense(d0, np.zeros(0, np.uint32), p0).shape == (0, 0)
    with pytest.raises(ValueError):
        T.band_to_csr(values[:-1], first, indptr)
    with pytest.raises(ValueError):
        T.band_to_csr(values, first[:-1], indptr)
    with pytest.raises(ValueError):
        T.band_to_dense(values, np.array([0, 0, 1, 4], dtype=np.uint32), indptr)
