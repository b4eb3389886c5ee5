"""Top-k LD partners, the parts that need no GPU: the header, `tomahawk ldscore --top`'s refusals, the host check of the key and the
cascade, the kernel's resources and topk_merge."""
import ctypes as C
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


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "twk_hip.h")).read()
    assert re.search(r"^int twk_hip_ld_topk\(twk_hip_ctx\* ctx, int mode, const twk_hip_filters\* filters,", text, re.M)
    assert re.search(r"^int twk_hip_topk_last\(const twk_hip_ctx\* ctx, double\* unpack_ms, uint64_t\* list_bytes\);", text, re.M)
    assert "#define TWK_HIP_TOPK_MAX 32" in text and "#define TWK_HIP_NO_PARTNER 0xFFFFFFFFu" in text
    assert "#define TWK_HIP_ABI_VERSION 5" in text
    lib = T.load_library()
    assert lib.twk_hip_abi_version() == 5
    assert T.NO_PARTNER == 0xFFFFFFFF


def test_a_null_context_is_refused():
    lib = T.load_library()
    assert lib.twk_hip_ld_topk(None, 0, None, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, T.STAT_R2, 5, None, None, None) == -1
    assert lib.twk_hip_topk_last(None, None, None) == -1


@pytest.fixture(scope="module")
def tiny_twk(tmp_path_factory):
    al = util.random_alleles(12, 16, seed=5)
    path = str(tmp_path_factory.mktemp("topk") / "tiny.twk")
    hostlib.write_twk(path, al, np.arange(12, dtype=np.uint32) * 100 + 1000, np.zeros(12, np.uint32), phased=np.ones(12, np.uint8), n_contigs=1, block_size=50)
    return path


@pytest.mark.parametrize("flags,what", [
    (["--top", "0"], "must be an integer between 1 and 32: 0"),
    (["--top", "33"], "must be an integer between 1 and 32: 33"),
    (["--top", "-1"], "must be an integer between 1 and 32: -1"),
    (["--top", "five"], "must be an integer between 1 and 32: five"),
    (["--top-stat", "r"], "--top-stat needs a number of partners to list (--top)"),
    (["--top", "5", "--top-stat", "rho"], "Unknown statistic (--top-stat): rho - one of r, r2, D, Dprime"),
    (["--top", "5", "--annot", "absent.txt"], "--top lists partners and takes no annotation file (--annot)"),
])
def test_parse_time_refusals_touch_nothing(tiny_twk, flags, what):
    r = _run("ldscore", "-i", tiny_twk, *flags)
    assert r.returncode == 1 and r.stdout == "", r.stderr
    assert what in r.stderr, r.stderr
    assert "HIP" not in r.stderr and "Opening" not in r.stderr and "Calling" not in r.stderr


def test_the_usage_stays_as_it_was_and_the_names_belong_to_ldscore():
    usage = _run("ldscore").stderr
    assert "Usage:  tomahawk ldscore [options] -i <in.twk> [-o <out.tsv>]" in usage and "--top" not in usage and "partner_pos" not in usage
    for cmd in ("prune", "lddecay", "ldmatrix"):
        for flags in (["--top", "5"], ["--top-stat", "r"]):
            r = _run(cmd, "-i", "absent.twk", *flags)
            assert r.returncode == 1 and "Unrecognized option: " + flags[0] in r.stderr and "Calling" not in r.stderr


def test_make_topk_check_passes():
    """The key against its definition, the cascade under random interleavings and the kernel's two levels against a sort
    (csrc/tools/topk_key_check.cpp)."""
    r = subprocess.run(["make", "-C", ROOT, "topk-check"], capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"^topk-check: (\d+) cases, (\d+) bad$", r.stdout, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, r.stdout[-500:]


@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not installed")
def test_topk_kernels_use_no_scratch_memory():
    """The kernels as `make hip` compiles them, by their metadata alone: no private segment, no spilled register."""
    seen = {n: util.kernel_resources(b) for n, b in util.engine_kernels().items() if "k_ld_topk" in n}
    assert seen, "no k_ld_topk kernel in the engine"
    assert all(scratch == 0 and spills == 0 for _, scratch, spills in seen.values()), seen


def _merge_restated(lists, k):
    M = lists[0][0].shape[0]
    idx = np.full((M, k), T.NO_PARTNER, dtype=np.uint32)
    val = np.zeros((M, k), dtype=np.float32)
    for v in range(M):
        entries = [(int(i[v, s]), np.float32(x[v, s])) for i, x in lists for s in range(i.shape[1]) if i[v, s] != T.NO_PARTNER]
        entries.sort(key=lambda e: (-abs(float(e[1])), e[0]))
        for s, (p, x) in enumerate(entries[:k]):
            idx[v, s], val[v, s] = p, x
    return idx, val


def test_topk_merge_agrees_with_a_restatement():
    rng = np.random.default_rng(9)
    M = 40
    for k, widths in ((4, (4, 4, 4)), (8, (3, 8)), (5, (2, 1)), (1, (1, 1, 1, 1))):
        # every shard lists its own partners (disjoint pair sets): variant v's candidates are dealt out over the shards
        lists = [(np.full((M, w), T.NO_PARTNER, dtype=np.uint32), np.zeros((M, w), dtype=np.float32)) for w in widths]
        for v in range(M):
            partners = rng.permutation(200)[:int(rng.integers(0, sum(widths) + 1))]
            values = (rng.integers(-4, 5, len(partners)) / 4.0).astype(np.float32)          # few distinct values: ties, +x against -x, zeros
            fill = [0] * len(widths)
            for p, x in zip(partners, values):
                s = int(rng.integers(len(widths)))
                if fill[s] < widths[s]:
                    lists[s][0][v, fill[s]], lists[s][1][v, fill[s]] = p, x
                    fill[s] += 1
        idx, val = T.topk_merge(lists, k)
        widx, wval = _merge_restated(lists, k)
        assert idx.dtype == np.uint32 and val.dtype == np.float32 and idx.shape == val.shape == (M, k)
        assert np.array_equal(idx, widx) and np.array_equal(val.view(np.uint32), wval.view(np.uint32)), (k, widths)
    # -0.0 keeps its sign, padding is +0.0
    idx, val = T.topk_merge([(np.array([[7]], dtype=np.uint32), np.array([[-0.0]], dtype=np.float32))], 2)
    assert idx.tolist() == [[7, T.NO_PARTNER]] and val.view(np.uint32).tolist() == [[0x80000000, 0]]
