"""ctypes binding of the C ABI in include/twk_hip.h (lib/libtwk_hip.so).

Fails loudly when the HIP library is missing or no device is usable: there is
no CPU path behind these calls.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtwk_hip.so")

ABI_VERSION = 5                 # TWK_HIP_ABI_VERSION of include/twk_hip.h (struct layouts below)
MODE_PHASED, MODE_UNPHASED, MODE_AUTO = 1, 2, 3
# option bits of twk_hip_tile_desc.window / the `window` argument of ld_all / ld_region (TWK_HIP_OPT_*)
OPT_WINDOW, OPT_KEEP_LOW_AC, OPT_REF_COMPAT, OPT_R2_SCREEN = 1, 2, 4, 8
NO_CLUMP = 0xFFFFFFFF      # TWK_HIP_NO_CLUMP: ld_clump's index_of for a variant in no clump
NO_PARTNER = 0xFFFFFFFF    # TWK_HIP_NO_PARTNER: ld_topk's idx for a slot that is not used
NO_BLOCK = 0xFFFFFFFF      # TWK_HIP_NO_BLOCK: ld_blocks' block_of for a variant in no block
TOPK_MAX = 32              # TWK_HIP_TOPK_MAX
STAT_R, STAT_R2, STAT_D, STAT_DPRIME = 0, 1, 2, 3      # TWK_HIP_STAT_*: the statistic ld_matrix fills in
REL_IBS, REL_IBS0, REL_KING = 0, 1, 2      # TWK_HIP_REL_*: the statistic relationship fills in
E_INVALID, E_OVERFLOW, E_STATE = -1, -4, -5      # TWK_HIP_E_*

# twk_hip_record (include/twk_hip.h): 104 bytes
RECORD_DTYPE = np.dtype([("idxA", "<u4"), ("idxB", "<u4"), ("flags", "<u4"), ("_pad", "<u4"),
                         ("cnt", "<f8", (4,)), ("D", "<f8"), ("Dprime", "<f8"), ("R", "<f8"),
                         ("R2", "<f8"), ("P", "<f8"), ("ChiSqFisher", "<f8"), ("ChiSqModel", "<f8")])
assert RECORD_DTYPE.itemsize == 104

# twk_hip_rle_desc: 16 bytes
RLE_DESC_DTYPE = np.dtype([("offset", "<u8"), ("n_runs", "<u4"), ("width", "u1"), ("missing", "u1"), ("_pad", "<u2")])
assert RLE_DESC_DTYPE.itemsize == 16

# twk_hip_variant_meta: 32 bytes
META_DTYPE = np.dtype([("ac", "<u4"), ("an", "<u4"), ("pos", "<u4"), ("rid", "<u4"),
                       ("missing", "<u4"), ("_pad", "<u4"), ("hwe", "<f8")])
assert META_DTYPE.itemsize == 32

# twk_hip_rel_counts: 24 bytes
REL_COUNTS_DTYPE = np.dtype([("n", "<u4"), ("ibs0", "<u4"), ("ibs2", "<u4"), ("hethet", "<u4"), ("het_a", "<u4"), ("het_b", "<u4")])
assert REL_COUNTS_DTYPE.itemsize == 24


class _Filters(C.Structure):
    _fields_ = [("minR2", C.c_double), ("maxR2", C.c_double), ("minDprime", C.c_double),
                ("maxDprime", C.c_double), ("minP", C.c_double)]


class _Tile(C.Structure):
    _fields_ = [("rowA0", C.c_uint32), ("nA", C.c_uint32), ("rowB0", C.c_uint32), ("nB", C.c_uint32),
                ("diag", C.c_int32), ("window", C.c_int32), ("l_window", C.c_uint32), ("_pad", C.c_uint32)]


class _VariantFilter(C.Structure):      # twk_hip_variant_filter
    _fields_ = [("min_maf", C.c_double), ("max_maf", C.c_double), ("min_mac", C.c_uint32), ("_pad", C.c_uint32),
                ("max_missing", C.c_double), ("min_hwe", C.c_double)]


class _Timing(C.Structure):
    _fields_ = [("count_ms", C.c_double), ("stats_ms", C.c_double), ("count_launches", C.c_uint64),
                ("stats_launches", C.c_uint64), ("row_pairs", C.c_uint64), ("variant_pairs", C.c_uint64),
                ("words_per_row", C.c_uint64), ("fused_launches", C.c_uint64), ("candidates", C.c_uint64),
                ("list_ms", C.c_double), ("list_launches", C.c_uint64), ("list_pairs", C.c_uint64),
                ("probe_ms", C.c_double), ("probe_launches", C.c_uint64), ("probe_pairs", C.c_uint64),
                ("count_shader_cycles", C.c_uint64), ("count_wall_ticks", C.c_uint64),
                ("three_launches", C.c_uint64), ("three_row_pairs", C.c_uint64), ("recount_candidates", C.c_uint64),
                ("outlier_launches", C.c_uint64), ("finish_ms", C.c_double), ("two_launches", C.c_uint64),
                ("prefix_launches", C.c_uint64), ("prefix_chunks", C.c_uint64), ("prefix_chunks_full", C.c_uint64),
                ("carrier_launches", C.c_uint64), ("one_launches", C.c_uint64), ("uz_launches", C.c_uint64), ("uz_row_pairs", C.c_uint64), ("uz_split_units", C.c_uint64)]


class _PlanEnv(C.Structure):         # twk_hip_plan_env
    _fields_ = [("n_samples", C.c_uint32), ("planes_per_variant", C.c_int32), ("k_chunks", C.c_uint32), ("resident_blocks", C.c_uint32),
                ("screen", C.c_int32), ("fused", C.c_int32), ("phased_math", C.c_int32), ("band_launch", C.c_int32), ("band_reverse", C.c_int32),
                ("_pad", C.c_int32), ("band_work_log2", C.c_int64), ("band_max_launches", C.c_int64), ("minR2", C.c_double)]


TILE_DTYPE = np.dtype([("rowA0", "<u4"), ("nA", "<u4"), ("rowB0", "<u4"), ("nB", "<u4"), ("diag", "<i4"), ("window", "<i4"),
                       ("l_window", "<u4"), ("one", "<u4")])       # twk_hip_tile_desc


def plan_region(meta, n_samples, a0, nA, b0, nB, triangle=True, part=0, n_parts=1, tile_variants=0, window=0, l_window=0,
                popc=None, screen=0, minR2=0.1, planes_per_variant=1, k_chunks=1, fused=False, phased_math=True,
                resident_blocks=512, band_launch=True, band_reverse=True, band_work_log2=19, band_max_launches=8,
                het=None, hom=None, two_margin=0.0, carrier=False, one=False, one_rows=0, walk_fine=False):
    """The engine's planner (twk_hip_plan_region: host arithmetic, needs no GPU) -> dict(tiles=TILE_DTYPE array, n_band_launches,
    row_begin, row_end, n_pairs, lo, hi, two_end).  meta: META_DTYPE per position of the index space.  het / hom (both or neither): het and
    hom-alt carriers per position - the two-product walk of an unscreened UnphasedMath call (twk_hip_plan_region_two), whose triangle is cut
    at row two_end; two_margin 0: the engine's.  carrier: the walk's two-product launches contract the row variants' carrier planes H | Q
    (twk_hip_plan_region_two_operand; the engine's option "carrier" on rows of more than 128 K chunks) - off: their H planes.  one (with
    carrier): the rows in front of the cut in blocks of one_rows variants (0: the engine's default), each block's columns up to its one_end as
    launches with tiles["one"] set (twk_hip_plan_region_two_form; the engine's options "one" and "one_rows").  walk_fine (with carrier): the fine
    walk's plan (twk_hip_plan_region_walk; the engine's option "walk_fine" where it applies) - staircase borders inside a row block: also
    two_last, side (per launch: 0 the whole rectangle, 1 the columns in front of its rows' borders, 2 those from them on), behind (per launch: a
    two-product launch behind the cut) and stair (per row: its border, 0: none)."""
    lib = load_library()
    meta = np.ascontiguousarray(meta, dtype=META_DTYPE)
    env = _PlanEnv(n_samples, planes_per_variant, k_chunks, resident_blocks, screen, int(fused), int(phased_math), int(band_launch),
                   int(band_reverse), 0, band_work_log2, band_max_launches, float(minR2))
    pc = None if popc is None else np.ascontiguousarray(popc, dtype=np.uint32)
    lo = np.zeros(nA, dtype=np.uint32); hi = np.zeros(nA, dtype=np.uint32)
    n_tiles, n_bands, r0, r1, pairs = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    two_end, two_last = C.c_uint32(0), C.c_uint32(0)
    stair = np.zeros(nA, dtype=np.uint32)
    ht = None if het is None else np.ascontiguousarray(het, dtype=np.uint32)
    hm = None if hom is None else np.ascontiguousarray(hom, dtype=np.uint32)
    cap = 1024
    while True:
        tiles = np.zeros(cap, dtype=TILE_DTYPE)
        notes = np.zeros(cap, dtype=np.uint8)
        rc = lib.twk_hip_plan_region_walk(C.byref(env), meta.ctypes.data, None if pc is None else pc.ctypes.data,
                                          None if ht is None else ht.ctypes.data, None if hm is None else hm.ctypes.data, float(two_margin), int(bool(carrier)), int(bool(one)), int(one_rows),
                                          int(bool(walk_fine)), len(meta), a0, nA, b0, nB,
                                          int(bool(triangle)), part, n_parts, tile_variants, window, l_window, tiles.ctypes.data, cap,
                                          C.byref(n_tiles), C.byref(n_bands), C.byref(r0), C.byref(r1), C.byref(pairs), lo.ctypes.data, hi.ctypes.data, C.byref(two_end),
                                          C.byref(two_last), notes.ctypes.data, stair.ctypes.data)
        if rc == -4 and n_tiles.value > cap:
            cap = n_tiles.value
            continue
        if rc != 0:
            raise HipError(rc, "twk_hip_plan_region", lib.twk_hip_strerror(rc).decode())
        break
    return dict(tiles=tiles[:n_tiles.value], n_band_launches=n_bands.value, row_begin=r0.value, row_end=r1.value, n_pairs=pairs.value, lo=lo, hi=hi,
                two_end=two_end.value, two_last=two_last.value, side=notes[:n_tiles.value] & 3, behind=(notes[:n_tiles.value] >> 2) & 1, stair=stair)


class Plant(C.Structure):            # twk_hip_plant: LD planted in the synthetic input (include/twk_hip.h)
    _fields_ = [("n_planted", C.c_uint32), ("half", C.c_uint32), ("mult", C.c_uint32), ("offset", C.c_uint32), ("max_eps", C.c_double)]

    @classmethod
    def spread(cls, n_variants: int, n_planted: int | None = None, max_eps: float = 0.3, mult: int = 2_654_435_761, offset: int = 12_345):
        """Copies whose sources are scattered over the whole data set: j = (k mult + offset) mod half with the golden-ratio prime
        2^32 / phi - coprime with every half it does not divide, and far from a small multiple of any half in sight, so that
        neighbouring copies have sources far apart."""
        import math
        half = n_variants // 2
        assert half < 2 or math.gcd(mult, half) == 1, (mult, half)
        return cls(half if n_planted is None else n_planted, half, mult, offset % max(half, 1), max_eps)

    @classmethod
    def near(cls, n_variants: int, distance: int, n_planted: int | None = None, max_eps: float = 0.3):
        """Copies at a fixed odd distance in front of their sources (window runs): copy 2k + 1 <- source 2k + 1 + distance."""
        assert distance % 2 == 1
        half = n_variants // 2
        return cls(half if n_planted is None else n_planted, half, 1, (distance + 1) // 2, max_eps)


class _LaunchStat(C.Structure):      # twk_hip_launch_stat
    _fields_ = [("ms", C.c_double), ("shader_mhz", C.c_double), ("xcd_finish_spread_us", C.c_double), ("row_pairs", C.c_uint64),
                ("candidates", C.c_uint64), ("words_per_row", C.c_uint32), ("kind", C.c_uint32), ("outlier", C.c_uint32), ("uz", C.c_uint32),
                ("prefix_chunks", C.c_uint64), ("prefix_chunks_full", C.c_uint64), ("carrier", C.c_uint32), ("one", C.c_uint32)]


@dataclass
class Filters:
    """twk_ld_settings filter defaults (reference lib/core.cpp:304)."""
    minR2: float = 0.1
    maxR2: float = 100.0
    minDprime: float = 0.0
    maxDprime: float = 100.0
    minP: float = 1.0

    def _c(self) -> _Filters:
        return _Filters(self.minR2, self.maxR2, self.minDprime, self.maxDprime, self.minP)


@dataclass
class BlockParams:
    """twk_hip_block_params: the thresholds of ld_blocks (percent, permille, base pairs), Gabriel et al.'s by default."""
    strong_lo: int = 70
    strong_hi: int = 98
    recomb_hi: int = 90
    strong_lo_2: int = 80
    strong_lo_34: int = 50
    inform_permille: int = 950
    max_span_2: int = 20000
    max_span_3: int = 30000

    def as_tuple(self):
        return (self.strong_lo, self.strong_hi, self.recomb_hi, self.strong_lo_2, self.strong_lo_34, self.inform_permille,
                self.max_span_2, self.max_span_3)


class HipError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str = ""):
        super().__init__(f"{what}: error {code}" + (f" ({detail})" if detail else ""))
        self.code = code


_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)
_lib = None


def load_library() -> C.CDLL:
    """Load lib/libtwk_hip.so (built by `make hip` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `make hip` (no CPU fallback exists)")
    lib = C.CDLL(LIB_PATH)
    p = C.c_void_p
    lib.twk_hip_abi_version.restype = C.c_int
    if lib.twk_hip_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {lib.twk_hip_abi_version()}, this binding was written for {ABI_VERSION}: rebuild (`make hip`)")
    lib.twk_hip_device_count.restype = C.c_int
    lib.twk_hip_strerror.restype = C.c_char_p
    lib.twk_hip_strerror.argtypes = [C.c_int]
    lib.twk_hip_last_error.restype = C.c_char_p
    lib.twk_hip_last_error.argtypes = [p]
    lib.twk_hip_ctx_create.argtypes = [C.c_int, C.POINTER(p)]
    lib.twk_hip_ctx_destroy.argtypes = [p]
    lib.twk_hip_set_problem.argtypes = [p, C.c_uint32, C.c_uint32]
    lib.twk_hip_upload_bitvectors.argtypes = [p, C.c_uint32, C.c_uint32, p, p, C.c_size_t, p]
    lib.twk_hip_upload_rle.argtypes = [p, C.c_uint32, C.c_uint32, p, C.c_size_t, p, p]
    lib.twk_hip_download_bitvectors.argtypes = [p, C.c_uint32, C.c_uint32, p, p, C.c_size_t]
    lib.twk_hip_host_alloc.argtypes = [C.c_size_t, C.POINTER(p)]
    lib.twk_hip_host_free.argtypes = [p]
    lib.twk_hip_generate_synthetic.argtypes = [p, C.c_uint64]
    lib.twk_hip_generate_synthetic_range.argtypes = [p, C.c_uint64, C.c_uint32]
    lib.twk_synth_bitvector.restype = C.c_uint32
    lib.twk_synth_bitvector.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, p]
    lib.twk_hip_generate_synthetic_planted.argtypes = [p, C.c_uint64, C.c_uint32, C.POINTER(Plant)]
    lib.twk_synth_planted_bitvector.restype = C.c_uint32
    lib.twk_synth_planted_bitvector.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(Plant), p]
    lib.twk_synth_plant_source.argtypes = [C.c_uint64, C.POINTER(Plant), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    lib.twk_hip_get_marginals.argtypes = [p, p, p, p, p]
    lib.twk_hip_select_samples.argtypes = [p, p, C.c_uint32]
    lib.twk_hip_selection.argtypes = [p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.twk_hip_get_meta.argtypes = [p, C.c_uint32, C.c_uint32, p]
    lib.twk_hip_set_hwe.argtypes = [p, C.c_uint32, C.c_uint32, p]
    lib.twk_hip_select_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_select_variants.argtypes = [p, C.POINTER(_VariantFilter), p, C.c_uint32, C.c_int32, C.POINTER(C.c_uint32)]
    lib.twk_hip_variant_selection.argtypes = [p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.twk_hip_variant_map.argtypes = [p, C.c_uint32, C.c_uint32, p]
    lib.twk_hip_select_variants_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_count_tile.argtypes = [p, C.c_int, C.POINTER(_Tile), p]
    lib.twk_hip_ld_tile.argtypes = [p, C.c_int, C.POINTER(_Tile), C.POINTER(_Filters), p, C.c_uint64,
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_all.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_int32, C.c_uint32, _SINK, p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_region.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, _SINK, p,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_score.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p, p,
                                     C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_score_annot.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p, C.c_uint32,
                                           C.c_uint64, p, p, C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_decay.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, p, p,
                                     C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_aggregate.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_int32, p, p,
                                         C.c_uint32, C.c_uint32, p, p, p, p, p, C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_prune.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_prune_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_clump.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p,
                                     C.c_double, C.c_double, p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)]
    lib.twk_hip_clump_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_matrix.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                      C.c_int32, C.c_float, p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_matrix_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_bandmat_layout.argtypes = [p, C.c_uint32, C.c_uint32, C.c_uint32, p, p]
    lib.twk_hip_ld_matrix_band.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                           C.c_int32, C.c_float, p, C.c_uint64, p, p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_bandmat_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_dprime_ci_band.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              p, p, C.c_uint64, p, p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_blocks.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, p,
                                      p, p, p, p, p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_blocks_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_blocks_stages.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.twk_hip_ld_split.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_uint32, p, p, p, p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.twk_hip_split_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_ld_topk.argtypes = [p, C.c_int, C.POINTER(_Filters), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, p, p,
                                    C.POINTER(C.c_uint64)]
    lib.twk_hip_topk_last.argtypes = [p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_relationship.argtypes = [p, p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_double,
                                         p, C.c_uint64, p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.twk_hip_relationship_last.argtypes = [p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.twk_hip_shard_rows.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32,
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.twk_hip_plan_region.argtypes = [p, p, p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.c_int32, C.c_uint32, p, C.c_uint32, p, p, p, p, p, p, p]
    lib.twk_hip_plan_region_two.argtypes = [p, p, p, p, p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                            C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p, C.c_uint32, p, p, p, p, p, p, p, p]
    lib.twk_hip_plan_region_two_operand.argtypes = [p, p, p, p, p, C.c_double, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                                    C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p, C.c_uint32, p, p, p, p, p, p, p, p]
    lib.twk_hip_plan_region_two_form.argtypes = [p, p, p, p, p, C.c_double, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                                 C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p, C.c_uint32, p, p, p, p, p, p, p, p]
    lib.twk_hip_plan_region_walk.argtypes = [p, p, p, p, p, C.c_double, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, p, C.c_uint32, p, p, p, p, p, p, p, p, p, p, p]
    lib.twk_hip_launch_log.argtypes = [p, p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    lib.twk_hip_fisher_exact.argtypes = [p, p, C.c_uint64, p, C.c_int32, C.POINTER(C.c_float)]
    lib.twk_hip_set_device_sink.argtypes = [p, C.c_int]
    lib.twk_hip_device_records.argtypes = [p, C.POINTER(p), C.POINTER(C.c_uint64)]
    lib.twk_hip_set_option.argtypes = [p, C.c_char_p, C.c_int64]
    lib.twk_hip_get_option.argtypes = [p, C.c_char_p, C.POINTER(C.c_int64)]
    lib.twk_hip_gather_records.argtypes = [C.POINTER(p), C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    lib.twk_hip_gather_backend.restype = C.c_char_p
    lib.twk_hip_drain_device_sink.argtypes = [p, _SINK, p, C.POINTER(C.c_uint64)]
    lib.twk_hip_option_describe.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_char_p)]
    lib.twk_hip_timing_reset.argtypes = [p]
    lib.twk_hip_timing_get.argtypes = [p, C.POINTER(_Timing)]
    _lib = lib
    return lib


def option_table():
    """The engine's option table (twk_hip_option_describe: needs no device) -> list of (key, default, lowest, highest, meaning)."""
    lib = load_library()
    out, i = [], 0
    while True:
        key, doc = C.c_char_p(), C.c_char_p()
        d, lo, hi = C.c_int64(), C.c_int64(), C.c_int64()
        if lib.twk_hip_option_describe(i, C.byref(key), C.byref(d), C.byref(lo), C.byref(hi), C.byref(doc)) != 0:
            return out
        out.append((key.value.decode(), d.value, lo.value, hi.value, doc.value.decode()))
        i += 1


def option_table_markdown() -> str:
    """... as the table INTEGRATION.md 1 carries between its `<!-- engine options -->` markers (tests/test_docs_consistency.py)."""
    def num(x):
        for k in (20, 30, 32, 40):
            if x == 1 << k:
                return f"2^{k}"
        return str(x)
    rows = ["| key | default | range | meaning |", "|---|---|---|---|"]
    rows += [f"| `{k}` | {num(d)} | {num(lo)} .. {num(hi)} | {doc} |" for k, d, lo, hi, doc in option_table()]
    return "\n".join(rows)


GATHER_SELF_LOOP = 1


def gather_backend() -> str:
    """What twk_hip_gather_records moves records with: "rccl <version>" or "unavailable (<why>)"."""
    return load_library().twk_hip_gather_backend().decode()


def gather_records(engines, dst: int = 0, self_loop: bool = False):
    """One process, one HipLd per GPU, each with its device sink on: gather their survivors into engines[dst]'s sink over RCCL
    (twk_hip_gather_records) -> (records now held by engines[dst], milliseconds of the transfers)."""
    lib = load_library()
    arr = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
    n, ms = C.c_uint64(0), C.c_double(0.0)
    rc = lib.twk_hip_gather_records(arr, len(engines), dst, GATHER_SELF_LOOP if self_loop else 0, C.byref(n), C.byref(ms))
    engines[dst]._check(rc, "twk_hip_gather_records")
    return n.value, ms.value


def device_count() -> int:
    return load_library().twk_hip_device_count()


def shard_rows(n_variants: int, part: int, n_parts: int, n_cols: int | None = None, triangle: bool = True):
    """Row band [r0, r1) and pair count of shard `part` (the partition ld_all uses). Host-only."""
    r0, r1, n = C.c_uint32(), C.c_uint32(), C.c_uint64()
    rc = load_library().twk_hip_shard_rows(n_variants, n_variants if n_cols is None else n_cols, int(triangle), part,
                                           n_parts, C.byref(r0), C.byref(r1), C.byref(n))
    if rc != 0:
        raise HipError(rc, "twk_hip_shard_rows")
    return r0.value, r1.value, n.value


def band_to_csr(values, first, indptr):
    """The banded LD matrix (HipLd.ld_matrix_band, or `ldmatrix --band`'s three files) as the arrays of a CSR matrix of shape (n, n):
    -> (data, indices int64[nnz], indptr int64[n + 1]); data is `values` itself - the band stores both orientations, row by row - and
    row u's indices are first[u], first[u] + 1, ...  scipy.sparse.csr_matrix((data, indices, indptr), shape=(n, n)) takes them as
    they are.  Plain NumPy."""
    indptr = np.asarray(indptr).astype(np.int64)
    first = np.asarray(first).astype(np.int64)
    values = np.asarray(values)
    n = len(first)
    if len(indptr) != n + 1 or (n and indptr[0] != 0) or (np.diff(indptr) < 0).any() or int(indptr[-1]) != len(values):
        raise ValueError("band_to_csr: first, indptr and values do not describe one band")
    lens = np.diff(indptr)
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    indices = np.arange(len(values), dtype=np.int64) - indptr[:-1][row] + first[row]
    return values, indices, indptr


def band_to_dense(values, first, indptr, fill=0.0):
    """The banded LD matrix scattered into a dense (n, n) array of values' dtype preset to `fill`: what HipLd.ld_matrix returns for the
    same window and fill.  Plain NumPy; for tests and small regions - the band exists because the dense matrix does not fit."""
    data, indices, indptr = band_to_csr(values, first, indptr)
    n = len(indptr) - 1
    if len(indices) and (indices.min() < 0 or indices.max() >= n):
        raise ValueError("band_to_dense: a band reaches beyond the matrix")
    out = np.full((n, n), fill, dtype=data.dtype)
    out[np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)), indices] = data
    return out


def _topk_keys(idx, val):
    """ld_topk's lists as the 64-bit keys whose unsigned order is the lists' order (csrc/hip/ld_topk_key.h); 0 for a slot not used."""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    bits = np.ascontiguousarray(val, dtype=np.float32).view(np.uint32).astype(np.uint64)
    key = (bits & np.uint64(0x7FFFFFFF)) << np.uint64(33) | (~idx).astype(np.uint64) << np.uint64(1) | bits >> np.uint64(31)
    return np.where(idx == np.uint32(NO_PARTNER), np.uint64(0), key)


def topk_merge(lists, k: int):
    """The lists of several ld_topk calls over disjoint pair sets - shards (part / n_parts), regions - merged into the lists of their
    union: per variant the entries of all of them under ld_topk's order (|value| as float32 descending, ties to the smaller partner
    index), cut at k, padded with (NO_PARTNER, +0.0).  lists: (idx, val) pairs, each (M, k_i).  Plain NumPy.
    -> (idx uint32[M, k], val float32[M, k])."""
    keys = np.concatenate([_topk_keys(i, v) for i, v in lists], axis=1)
    keys = np.sort(keys, axis=1)[:, ::-1]
    if keys.shape[1] < k:
        keys = np.concatenate([keys, np.zeros((keys.shape[0], k - keys.shape[1]), dtype=np.uint64)], axis=1)
    keys = np.ascontiguousarray(keys[:, :k])
    used = keys != 0
    idx = np.where(used, ~(keys >> np.uint64(1)).astype(np.uint32), np.uint32(NO_PARTNER)).astype(np.uint32)
    bits = ((keys >> np.uint64(33)).astype(np.uint32) | ((keys & np.uint64(1)).astype(np.uint32) << np.uint32(31)))
    val = np.where(used, bits, np.uint32(0)).astype(np.uint32).view(np.float32)
    return idx, val


def words64(n_samples: int) -> int:
    return (2 * n_samples + 63) // 64


def synth_bitvector(seed: int, n_samples: int, v: int, plant: "Plant | None" = None) -> tuple[np.ndarray, int]:
    """Host twin of the device generator (twk_synth_bitvector / twk_synth_planted_bitvector)."""
    out = np.zeros(words64(n_samples), dtype=np.uint64)
    ac = load_library().twk_synth_planted_bitvector(seed, n_samples, v, None if plant is None else C.byref(plant), out.ctypes.data)
    return out, int(ac)


def plant_source(seed: int, plant: "Plant", v: int):
    """-> (source variant, flip probability) when global variant v is a planted copy, else None (twk_synth_plant_source)."""
    src, eps = C.c_uint32(0), C.c_double(0.0)
    if load_library().twk_synth_plant_source(seed, C.byref(plant), v, C.byref(src), C.byref(eps)):
        return int(src.value), float(eps.value)
    return None


class HipLd:
    """One engine context on one GPU (twk_hip_ctx)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.twk_hip_ctx_create(device, C.byref(self._ctx))
        if rc != 0:
            raise HipError(rc, "twk_hip_ctx_create", self._lib.twk_hip_strerror(rc).decode())
        self.n_samples = 0
        self.n_variants = 0
        self.device = device
        self._sink_on = False
        self._defaults = {}

    # ---- switches (twk_hip_set_option: the library reads no environment variable) ----
    def get_option(self, key: str) -> int:
        v = C.c_int64(0)
        self._check(self._lib.twk_hip_get_option(self._ctx, key.encode(), C.byref(v)), f"twk_hip_get_option({key})")
        return int(v.value)

    def set_option(self, key: str, value: int):
        self._defaults.setdefault(key, self.get_option(key))
        self._check(self._lib.twk_hip_set_option(self._ctx, key.encode(), int(value)), f"twk_hip_set_option({key})")

    def unset_option(self, key: str):
        """Back to the value the context was created with."""
        if key in self._defaults:
            self._check(self._lib.twk_hip_set_option(self._ctx, key.encode(), self._defaults[key]), f"twk_hip_set_option({key})")

    def close(self):
        if self._ctx:
            self._lib.twk_hip_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            detail = self._lib.twk_hip_last_error(self._ctx).decode() or self._lib.twk_hip_strerror(rc).decode()
            raise HipError(rc, what, detail)

    # ---- input ----
    def set_problem(self, n_samples: int, n_variants: int):
        self._check(self._lib.twk_hip_set_problem(self._ctx, n_samples, n_variants), "twk_hip_set_problem")
        self.n_samples, self.n_variants = n_samples, n_variants

    def upload(self, data: np.ndarray, meta: np.ndarray, mask: np.ndarray | None = None, first: int = 0):
        """data/mask: uint64 [count, stride64] reference-layout bitvectors; meta: META_DTYPE[count]."""
        data = np.ascontiguousarray(data, dtype=np.uint64)
        meta = np.ascontiguousarray(meta, dtype=META_DTYPE)
        assert data.ndim == 2 and data.shape[0] == meta.shape[0]
        mptr = None
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint64)
            assert mask.shape == data.shape
            mptr = mask.ctypes.data
        self._check(self._lib.twk_hip_upload_bitvectors(self._ctx, first, data.shape[0], data.ctypes.data, mptr,
                                                        data.shape[1], meta.ctypes.data), "twk_hip_upload_bitvectors")

    def upload_rle(self, run_bytes: np.ndarray, desc: np.ndarray, meta: np.ndarray, first: int = 0):
        """Run-length genotype words as stored in a .twk block (uint8 buffer) + RLE_DESC_DTYPE[count]:
        expanded to bitvector + mask by a HIP kernel (twk_hip_upload_rle)."""
        run_bytes = np.ascontiguousarray(run_bytes, dtype=np.uint8)
        desc = np.ascontiguousarray(desc, dtype=RLE_DESC_DTYPE)
        meta = np.ascontiguousarray(meta, dtype=META_DTYPE)
        assert desc.shape == meta.shape
        self._check(self._lib.twk_hip_upload_rle(self._ctx, first, len(desc), run_bytes.ctypes.data, run_bytes.size,
                                                 desc.ctypes.data, meta.ctypes.data), "twk_hip_upload_rle")

    def download(self, first: int = 0, count: int | None = None):
        """-> (data, mask) uint64 [count, words64] in the reference layout, as held on the device."""
        count = self.n_variants - first if count is None else count
        w = words64(self.n_samples)
        data = np.zeros((count, w), dtype=np.uint64)
        mask = np.zeros((count, w), dtype=np.uint64)
        self._check(self._lib.twk_hip_download_bitvectors(self._ctx, first, count, data.ctypes.data, mask.ctypes.data, w),
                    "twk_hip_download_bitvectors")
        return data, mask

    def generate_synthetic(self, seed: int = 42, first_variant: int = 0, plant: "Plant | None" = None):
        """Synthetic benchmark input for global variants [first_variant, first_variant + n_variants); plant: LD pairs planted in it."""
        self._check(self._lib.twk_hip_generate_synthetic_planted(self._ctx, seed, first_variant, None if plant is None else C.byref(plant)),
                    "twk_hip_generate_synthetic_planted")

    def marginals(self):
        M = self.n_variants
        ac, het, hom, miss = (np.zeros(M, dtype=np.uint32) for _ in range(4))
        self._check(self._lib.twk_hip_get_marginals(self._ctx, ac.ctypes.data, het.ctypes.data, hom.ctypes.data,
                                                    miss.ctypes.data), "twk_hip_get_marginals")
        return ac, het, hom, miss

    # ---- sample subsets (twk_hip_select_samples: the data stays on the device as uploaded, the context works on the kept samples) ----
    def select_samples(self, keep):
        """keep: strictly ascending sample indices into the data as uploaded (any integer array-like), or None to drop the selection.
        Afterwards the context is a problem of len(keep) samples: n_samples, download(), marginals(), meta() and every compute call
        are those of the subset.  A second call selects from the uploaded data again."""
        if keep is None:
            self._check(self._lib.twk_hip_select_samples(self._ctx, None, 0), "twk_hip_select_samples")
        else:
            k = np.asarray(keep)
            if k.size and not np.issubdtype(k.dtype, np.integer):
                raise TypeError("select_samples: sample indices must be integers")
            if k.size and (k.min() < 0 or k.max() > 0xFFFFFFFF):
                raise HipError(E_INVALID, "twk_hip_select_samples", "a sample index outside 0 .. 2^32 - 1")
            k = np.ascontiguousarray(k.reshape(-1), dtype=np.uint32)
            buf = k if k.size else np.zeros(1, dtype=np.uint32)          # (an empty list is the engine's to refuse: not NULL, which drops)
            self._check(self._lib.twk_hip_select_samples(self._ctx, buf.ctypes.data, k.size), "twk_hip_select_samples")
        self.n_samples = self.selection()[1]

    def selection(self):
        """-> (samples of the data as uploaded, samples of the working set); equal when no selection is active."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.twk_hip_selection(self._ctx, C.byref(a), C.byref(b)), "twk_hip_selection")
        return int(a.value), int(b.value)

    def meta(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """-> META_DTYPE[count]: the working set's metadata as the engine holds it (after a selection: ac, an, missing recomputed)."""
        count = self.n_variants - first if count is None else count
        out = np.zeros(count, dtype=META_DTYPE)
        self._check(self._lib.twk_hip_get_meta(self._ctx, first, count, out.ctypes.data), "twk_hip_get_meta")
        return out

    def set_hwe(self, hwe, first: int = 0):
        """Overwrite the Hardy-Weinberg P of variants [first, first + len(hwe)) of the working set."""
        h = np.ascontiguousarray(hwe, dtype=np.float64).reshape(-1)
        self._check(self._lib.twk_hip_set_hwe(self._ctx, first, h.size, h.ctypes.data), "twk_hip_set_hwe")

    def select_last(self) -> dict:
        """Of the last selection: the kernel's time and the bytes of genotype rows it read and wrote."""
        ms, r, w = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_select_last(self._ctx, C.byref(ms), C.byref(r), C.byref(w)), "twk_hip_select_last")
        return {"select_ms": ms.value, "bytes_read": int(r.value), "bytes_written": int(w.value)}

    # ---- variant subsets (twk_hip_select_variants: the base stays on the device, the context works on the kept variants) ----
    def select_variants(self, list=None, exclude=False, min_maf=0.0, max_maf=0.5, min_mac=0, max_missing=1.0, min_hwe=0.0) -> int:
        """Keep the variants of the base - the data as uploaded, or the working set of a sample selection - that pass the list (strictly
        ascending base indices; exclude: the list names the variants to drop) and every threshold.  -> n_kept.  Afterwards n_variants,
        download(), marginals(), meta() and every compute call are those of the kept variants, indexed 0 .. n_kept - 1; variant_map()
        gives their base indices.  A second call selects from the base again; select_variants(None) with every threshold off drops
        the selection."""
        off = (min_maf, max_maf, min_mac, max_missing, min_hwe) == (0.0, 0.5, 0, 1.0, 0.0)
        n = C.c_uint32(0)
        if list is None and off:
            self._check(self._lib.twk_hip_select_variants(self._ctx, None, None, 0, 0, C.byref(n)), "twk_hip_select_variants")
        else:
            if not 0 <= int(min_mac) <= 0xFFFFFFFF:
                raise HipError(E_INVALID, "twk_hip_select_variants", "min_mac outside 0 .. 2^32 - 1")
            f = _VariantFilter(float(min_maf), float(max_maf), int(min_mac), 0, float(max_missing), float(min_hwe))
            if list is None:
                ptr, count = None, 0
            else:
                k = np.asarray(list)
                if k.size and not np.issubdtype(k.dtype, np.integer):
                    raise TypeError("select_variants: variant indices must be integers")
                if k.size and (k.min() < 0 or k.max() > 0xFFFFFFFF):
                    raise HipError(E_INVALID, "twk_hip_select_variants", "a variant index outside 0 .. 2^32 - 1")
                k = np.ascontiguousarray(k.reshape(-1), dtype=np.uint32)
                buf = k if k.size else np.zeros(1, dtype=np.uint32)          # (an empty list is a list: not NULL, which means "no list test")
                ptr, count = buf.ctypes.data, k.size
            self._check(self._lib.twk_hip_select_variants(self._ctx, C.byref(f), ptr, count, int(bool(exclude)), C.byref(n)), "twk_hip_select_variants")
        self.n_variants = self.variant_selection()[1]
        return int(n.value)

    def variant_selection(self):
        """-> (variants of the base, variants of the working set); equal when no selection is active."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.twk_hip_variant_selection(self._ctx, C.byref(a), C.byref(b)), "twk_hip_variant_selection")
        return int(a.value), int(b.value)

    def variant_map(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """-> uint32[count]: the base index of every working variant (the identity while no selection is active)."""
        count = self.n_variants - first if count is None else count
        out = np.zeros(max(count, 0), dtype=np.uint32)
        if count == 0 and 0 <= first <= self.n_variants:
            return out                                                   # (an empty slice: the engine takes no zero count)
        self._check(self._lib.twk_hip_variant_map(self._ctx, first, count, out.ctypes.data), "twk_hip_variant_map")
        return out

    def select_variants_last(self) -> dict:
        """Of the last variant selection: the kernels' time and the bytes of genotype rows they read and wrote."""
        ms, r, w = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_select_variants_last(self._ctx, C.byref(ms), C.byref(r), C.byref(w)), "twk_hip_select_variants_last")
        return {"select_ms": ms.value, "bytes_read": int(r.value), "bytes_written": int(w.value)}

    # ---- compute ----
    @staticmethod
    def _tile(a0, nA, b0, nB, diag, window=0, l_window=0) -> _Tile:
        return _Tile(a0, nA, b0, nB, int(bool(diag)), int(window), l_window, 0)

    def count_tile(self, mode: int, a0: int, nA: int, b0: int, nB: int, diag: bool = False) -> np.ndarray:
        ncell = 4 if mode == MODE_PHASED else 9
        out = np.zeros((nA, nB, ncell), dtype=np.uint64)
        t = self._tile(a0, nA, b0, nB, diag)
        self._check(self._lib.twk_hip_count_tile(self._ctx, mode, C.byref(t), out.ctypes.data), "twk_hip_count_tile")
        return out

    def ld_tile(self, mode: int, a0: int, nA: int, b0: int, nB: int, diag: bool, filters: Filters,
                capacity: int | None = None, window: int = 0, l_window: int = 0):
        cap = capacity if capacity is not None else nA * nB
        out = np.zeros(max(cap, 1), dtype=RECORD_DTYPE)
        n, npairs = C.c_uint64(0), C.c_uint64(0)
        t = self._tile(a0, nA, b0, nB, diag, window, l_window)
        f = filters._c()
        rc = self._lib.twk_hip_ld_tile(self._ctx, mode, C.byref(t), C.byref(f), out.ctypes.data, cap,
                                       C.byref(n), C.byref(npairs))
        if rc == E_OVERFLOW:
            raise HipError(rc, "twk_hip_ld_tile", f"need capacity {n.value}")
        self._check(rc, "twk_hip_ld_tile")
        return out[: n.value].copy(), npairs.value

    def ld_all(self, mode: int, filters: Filters, part: int = 0, n_parts: int = 1, tile_variants: int = 0,
               window: int = 0, l_window: int = 0, collect: bool = True):
        """All-vs-all over shard `part` of `n_parts`. Returns (records, n_pairs, n_records).
        `window` carries the TWK_HIP_OPT_* bits unchanged (OPT_WINDOW = 1, OPT_KEEP_LOW_AC = 2)."""
        chunks = []

        def sink(_user, recs, n):
            if collect and n:
                buf = (C.c_char * (n * RECORD_DTYPE.itemsize)).from_address(recs)
                chunks.append(np.frombuffer(buf, dtype=RECORD_DTYPE).copy())
            return 0

        cb = _SINK(sink)
        npairs, nrec = C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        # (with the device sink on the records stay in HBM: the returned array is empty, see device_records_tensor)
        self._check(self._lib.twk_hip_ld_all(self._ctx, mode, C.byref(f), part, n_parts, tile_variants,
                                             int(window), l_window, cb, None, C.byref(npairs), C.byref(nrec)),
                    "twk_hip_ld_all")
        recs = np.concatenate(chunks) if chunks else np.zeros(0, dtype=RECORD_DTYPE)
        return recs, npairs.value, nrec.value

    def ld_region(self, mode: int, filters: Filters, a0: int, nA: int, b0: int, nB: int, triangle: bool,
                  part: int = 0, n_parts: int = 1, tile_variants: int = 0, window: int = 0, l_window: int = 0,
                  collect: bool = True):
        """LD over rows [a0,a0+nA) x cols [b0,b0+nB) (triangle: col > row, nB >= nA). Returns (records, n_pairs, n_records)."""
        chunks = []

        def sink(_user, recs, n):
            if collect and n:
                buf = (C.c_char * (n * RECORD_DTYPE.itemsize)).from_address(recs)
                chunks.append(np.frombuffer(buf, dtype=RECORD_DTYPE).copy())
            return 0

        cb = _SINK(sink)
        npairs, nrec = C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_region(self._ctx, mode, C.byref(f), a0, nA, b0, nB, int(bool(triangle)), part,
                                                n_parts, tile_variants, int(window), l_window, cb, None,
                                                C.byref(npairs), C.byref(nrec)), "twk_hip_ld_region")
        recs = np.concatenate(chunks) if chunks else np.zeros(0, dtype=RECORD_DTYPE)
        return recs, npairs.value, nrec.value

    def ld_score(self, mode: int, filters: Filters, a0: int = 0, nA: int | None = None, b0: int = 0, nB: int | None = None,
                 triangle: bool = True, part: int = 0, n_parts: int = 1, tile_variants: int = 0, window: int = 0, l_window: int = 0):
        """LD scores (twk_hip_ld_score): per variant the number of records ld_region would report with the variant at either end
        and the sum of their R2, reduced on the device - no record is formed.  filters.minP must be >= 1.  A shard returns
        partial arrays over all variants.  -> (n_partners uint64[M], sum_r2 float64[M], n_pairs)."""
        M = self.n_variants
        nA = M - a0 if nA is None else nA
        nB = M - b0 if nB is None else nB
        n = np.zeros(M, dtype=np.uint64)
        s = np.zeros(M, dtype=np.float64)
        npairs = C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_score(self._ctx, mode, C.byref(f), a0, nA, b0, nB, int(bool(triangle)), part, n_parts,
                                               tile_variants, int(window), l_window, n.ctypes.data, s.ctypes.data,
                                               C.byref(npairs)), "twk_hip_ld_score")
        return n, s, npairs.value

    def ld_score_annot(self, mode: int, filters: Filters, annot, a0: int = 0, nA: int | None = None, b0: int = 0, nB: int | None = None,
                       triangle: bool = True, part: int = 0, n_parts: int = 1, tile_variants: int = 0, window: int = 0,
                       l_window: int = 0):
        """Partitioned LD scores (twk_hip_ld_score_annot): for every variant v and annotation column c the sum over the records
        ld_region would report with v at either end of rint((R2 * annot[w][c]) * 2^32), w the variant at the other end - summed
        exactly in integers on the device, converted once and divided by 2^32: the same bits for any tiling, order or repeat.  The
        variant itself is no partner.  annot: (M, C) float64, one row per uploaded variant (1-D: one column); finite, |a| <= 65536,
        1 <= C <= 256.  filters.minP must be >= 1.  A shard returns partial arrays.
        -> (n_partners uint64[M], score float64[M, C], n_pairs)."""
        M = self.n_variants
        a = np.ascontiguousarray(annot, dtype=np.float64)
        if a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim != 2 or a.shape[0] != M:
            raise ValueError(f"annot must have one row per uploaded variant: {M}, not shape {a.shape}")
        ncat = a.shape[1]
        nA = M - a0 if nA is None else nA
        nB = M - b0 if nB is None else nB
        n = np.zeros(M, dtype=np.uint64)
        s = np.zeros((M, ncat), dtype=np.float64)
        npairs = C.c_uint64(0)
        f = filters._c()
        # (a column count the engine refuses is the engine's to refuse: it reads nothing before it has)
        self._check(self._lib.twk_hip_ld_score_annot(self._ctx, mode, C.byref(f), a0, nA, b0, nB, int(bool(triangle)), part, n_parts,
                                                     tile_variants, int(window), l_window, a.ctypes.data, ncat, max(ncat, 1),
                                                     n.ctypes.data, s.ctypes.data, C.byref(npairs)), "twk_hip_ld_score_annot")
        return n, s, npairs.value

    def ld_decay(self, mode: int, filters: Filters, range_bp: int = 10_000_000, n_bins: int = 1000, a0: int = 0, nA: int | None = None,
                 b0: int = 0, nB: int | None = None, triangle: bool = True, part: int = 0, n_parts: int = 1, tile_variants: int = 0,
                 window: int = 0, l_window: int = 0):
        """LD decay (twk_hip_ld_decay): r2 by distance.  A pair counts when ld_region would report a record for it, both variants
        lie on one contig and their positions differ; its bin is min(|posA - posB| // (range_bp // n_bins), n_bins - 1).  Per bin the
        number of counting pairs and the sum of their R2, each rounded once to a multiple of 2^-32 and summed exactly in integers on
        the device: the same bits for any tiling, order or repeat.  No record is formed.  filters.minP must be >= 1; n_bins <= 4096;
        range_bp >= n_bins.  A shard returns partial arrays.  -> (n uint64[n_bins], sum_r2 float64[n_bins], n_pairs)."""
        M = self.n_variants
        nA = M - a0 if nA is None else nA
        nB = M - b0 if nB is None else nB
        size = max(int(n_bins), 1) if 0 <= int(n_bins) <= 4096 else 1          # (a refused n_bins is the engine's to refuse)
        n = np.zeros(size, dtype=np.uint64)
        s = np.zeros(size, dtype=np.float64)
        npairs = C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_decay(self._ctx, mode, C.byref(f), a0, nA, b0, nB, int(bool(triangle)), part, n_parts,
                                               tile_variants, int(window), l_window, int(range_bp), int(n_bins), n.ctypes.data,
                                               s.ctypes.data, C.byref(npairs)), "twk_hip_ld_decay")
        return n, s, npairs.value

    def ld_aggregate(self, mode: int, filters: Filters, bin_x, bin_y, x_bins: int, y_bins: int, stat: int = STAT_R2, a0: int = 0,
                     nA: int | None = None, b0: int = 0, nB: int | None = None, triangle: bool = True, part: int = 0, n_parts: int = 1,
                     tile_variants: int = 0, window: int = 0, l_window: int = 0):
        """LD aggregate (twk_hip_ld_aggregate): the pairs' LD rasterised into x_bins x y_bins cells.  bin_x / bin_y: one uint16 per
        uploaded variant, its bin on that axis, 0xFFFF for off the landscape.  For every pair (A, B) ld_region would report a record
        for, v (stat: STAT_R signed, STAT_R2, STAT_D, STAT_DPRIME) is added to cell (bin_x[A], bin_y[B]) and to cell (bin_x[B],
        bin_y[A]), each if both bins are valid.  Per cell the contributions, the sums of rint(v * 2^32) / 2^32 and of
        rint((v * v) * 2^32) / 2^32, summed exactly in integers on the device, and the extremes of rint(v * 2^32) / 2^32 (0 in an
        empty cell): the same bits for any tiling, order or repeat.  No record is formed.  filters.minP must be >= 1; 1 <= x_bins,
        y_bins <= 4096.  A shard returns partial arrays.  -> (n uint64, sum, sum_sq, min, max float64, each (x_bins, y_bins), n_pairs)."""
        M = self.n_variants
        nA = M - a0 if nA is None else nA
        nB = M - b0 if nB is None else nB
        bx = np.ascontiguousarray(bin_x, dtype=np.uint16)
        by = np.ascontiguousarray(bin_y, dtype=np.uint16)
        if M and (bx.shape != (M,) or by.shape != (M,)):          # (before upload the engine refuses the call itself)
            raise ValueError(f"bin_x and bin_y hold one bin per uploaded variant ({M}): got {bx.shape} and {by.shape}")
        ok = 1 <= int(x_bins) <= 4096 and 1 <= int(y_bins) <= 4096          # (refused bin counts are the engine's to refuse)
        shape = (int(x_bins), int(y_bins)) if ok else (1, 1)
        n = np.zeros(shape, dtype=np.uint64)
        out = [np.zeros(shape, dtype=np.float64) for _ in range(4)]
        npairs = C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_aggregate(self._ctx, mode, C.byref(f), a0, nA, b0, nB, int(bool(triangle)), part, n_parts,
                                                   tile_variants, int(window), l_window, int(stat), bx.ctypes.data, by.ctypes.data,
                                                   int(x_bins), int(y_bins), n.ctypes.data, *(a.ctypes.data for a in out),
                                                   C.byref(npairs)), "twk_hip_ld_aggregate")
        return (n, *out, npairs.value)

    def ld_prune(self, mode: int, filters: Filters, a0: int = 0, n: int | None = None, tile_variants: int = 0, window: int = 0,
                 l_window: int = 0):
        """Greedy LD pruning in file order (twk_hip_ld_prune) of the triangle of variants [a0, a0 + n): a variant is kept if and
        only if no variant kept before it forms a record with it that ld_region would report; decided and walked on the device -
        no record is formed.  filters.minP must be >= 1.  -> (keep uint8[M], n_kept, n_edges, n_pairs)."""
        M = self.n_variants
        n = M - a0 if n is None else n
        keep = np.zeros(M, dtype=np.uint8)
        n_kept, n_edges, npairs = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_prune(self._ctx, mode, C.byref(f), a0, n, tile_variants, int(window), l_window,
                                               keep.ctypes.data, C.byref(n_kept), C.byref(n_edges), C.byref(npairs)), "twk_hip_ld_prune")
        return keep, n_kept.value, n_edges.value, npairs.value

    def prune_last(self) -> dict:
        """Of the last ld_prune call (twk_hip_prune_last): the walk kernel's device time and the adjacency bitmap's size."""
        ms, b = C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_prune_last(self._ctx, C.byref(ms), C.byref(b)), "twk_hip_prune_last")
        return {"walk_ms": ms.value, "bitmap_bytes": b.value}

    def ld_clump(self, mode: int, filters: Filters, p, p1: float = 1e-4, p2: float = 1e-2, a0: int = 0, n: int | None = None,
                 tile_variants: int = 0, window: int = 0, l_window: int = 0):
        """LD clumping (twk_hip_ld_clump) of the triangle of variants [a0, a0 + n): the variants are visited in ascending P (p: one
        float64 per variant, NaN for none) up to p1; a visited variant that belongs to no clump becomes an index variant and claims
        every free variant with P <= p2 that forms a record with it that ld_region would report; decided and walked on the device -
        no record is formed.  filters.minP must be >= 1.  -> (index_of uint32[M], n_clumps, n_members, n_edges, n_pairs);
        index_of is NO_CLUMP where a variant belongs to no clump."""
        M = self.n_variants
        n = M - a0 if n is None else n
        p = np.ascontiguousarray(p, dtype=np.float64)
        if p.shape != (M,):
            raise ValueError(f"p must hold one value per variant ({M}), not {p.shape}")
        index_of = np.full(M, NO_CLUMP, dtype=np.uint32)
        n_clumps, n_members, n_edges, npairs = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_clump(self._ctx, mode, C.byref(f), a0, n, tile_variants, int(window), l_window, p.ctypes.data,
                                               float(p1), float(p2), index_of.ctypes.data, C.byref(n_clumps), C.byref(n_members),
                                               C.byref(n_edges), C.byref(npairs)), "twk_hip_ld_clump")
        return index_of, n_clumps.value, n_members.value, n_edges.value, npairs.value

    def clump_last(self) -> dict:
        """Of the last ld_clump call (twk_hip_clump_last): the walk kernel's device time and the adjacency bitmap's size."""
        ms, b = C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_clump_last(self._ctx, C.byref(ms), C.byref(b)), "twk_hip_clump_last")
        return {"walk_ms": ms.value, "bitmap_bytes": b.value}

    def ld_matrix(self, mode: int, filters: Filters, stat: int = STAT_R, fill: float = 0.0, a0: int = 0, n: int | None = None,
                  tile_variants: int = 0, window: int = 0, l_window: int = 0):
        """The dense LD matrix (twk_hip_ld_matrix) of the triangle of variants [a0, a0 + n): entry (u, v) is the statistic - STAT_R
        (signed: copysign(R, D)), STAT_R2, STAT_D or STAT_DPRIME - of the record ld_region would report for the two variants, rounded
        once to float32, and `fill` (bit for bit) where it would report none; the diagonal is 1 (for STAT_D: fill).  Filled on the
        device - no record is formed.  filters.minP must be >= 1.  -> (float32 ndarray (n, n), n_records, n_pairs)."""
        M = self.n_variants
        n = M - a0 if n is None else n
        out = np.empty((max(n, 0), max(n, 0)), dtype=np.float32)
        nrec, npairs = C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        # (the fill travels as a C float: a NaN's payload is kept as far as the platform's float conversions keep it)
        self._check(self._lib.twk_hip_ld_matrix(self._ctx, mode, C.byref(f), a0, n, tile_variants, int(window), l_window, int(stat),
                                                C.c_float(fill), out.ctypes.data, n, C.byref(nrec), C.byref(npairs)), "twk_hip_ld_matrix")
        return out, nrec.value, npairs.value

    def matrix_last(self) -> dict:
        """Of the last ld_matrix call (twk_hip_matrix_last): the device-to-host copy's time and the matrix's size."""
        ms, b = C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_matrix_last(self._ctx, C.byref(ms), C.byref(b)), "twk_hip_matrix_last")
        return {"copy_ms": ms.value, "matrix_bytes": b.value}

    def bandmat_layout(self, l_window: int, a0: int = 0, n: int | None = None):
        """The banded LD matrix's layout (twk_hip_bandmat_layout) of the slice [a0, a0 + n) for a window of l_window base pairs, from
        the uploaded metadata, on the host: row u stores the columns [first[u], first[u] + indptr[u + 1] - indptr[u]) - the variants
        on u's contig within the window - from slot indptr[u] on; indptr[n] floats in all.
        -> (first uint32[n], indptr uint64[n + 1])."""
        n = self.n_variants - a0 if n is None else n
        first = np.zeros(max(n, 0), dtype=np.uint32)
        indptr = np.zeros(max(n, 0) + 1, dtype=np.uint64)
        self._check(self._lib.twk_hip_bandmat_layout(self._ctx, a0, n, l_window, first.ctypes.data, indptr.ctypes.data), "twk_hip_bandmat_layout")
        return first, indptr

    def ld_matrix_band(self, mode: int, filters: Filters, l_window: int, stat: int = STAT_R, fill: float = 0.0, a0: int = 0,
                       n: int | None = None, tile_variants: int = 0):
        """The banded LD matrix (twk_hip_ld_matrix_band): ld_matrix with window=OPT_WINDOW and this l_window, in band storage - for
        every in-band (u, v), values[indptr[u] + (v - first[u])] holds the bits of the dense matrix's entry (u, v); what the band does
        not store is the dense matrix's fill.  Both orientations are stored (band_to_csr, band_to_dense).  filters.minP must be >= 1.
        -> (values float32[indptr[n]], first uint32[n], indptr uint64[n + 1], n_records, n_pairs)."""
        n = self.n_variants - a0 if n is None else n
        _, layout_ptr = self.bandmat_layout(l_window, a0, n)          # (sizes `values`; refuses what the call would refuse about the slice)
        nnz = int(layout_ptr[-1])
        values = np.empty(nnz, dtype=np.float32)
        first = np.zeros(n, dtype=np.uint32)
        indptr = np.zeros(n + 1, dtype=np.uint64)
        nrec, npairs = C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_matrix_band(self._ctx, mode, C.byref(f), a0, n, tile_variants, int(OPT_WINDOW), l_window, int(stat),
                                                     C.c_float(fill), values.ctypes.data, nnz, first.ctypes.data, indptr.ctypes.data,
                                                     C.byref(nrec), C.byref(npairs)), "twk_hip_ld_matrix_band")
        return values, first, indptr, nrec.value, npairs.value

    def bandmat_last(self) -> dict:
        """Of the last ld_matrix_band call (twk_hip_bandmat_last): the device-to-host copy's time and the band's size."""
        ms, b = C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_bandmat_last(self._ctx, C.byref(ms), C.byref(b)), "twk_hip_bandmat_last")
        return {"copy_ms": ms.value, "band_bytes": b.value}

    def ld_dprime_ci_band(self, mode: int, filters: Filters, l_window: int, a0: int = 0, n: int | None = None, tile_variants: int = 0):
        """The confidence bounds of D' in band storage (twk_hip_ld_dprime_ci_band): for every in-band (u, v) of bandmat_layout's layout
        for l_window, lo / hi [indptr[u] + (v - first[u])] hold the bounds in percent (0 .. 100) of the pair's D' by a likelihood scan of
        the 2 x 2 table of the record ld_region would report, and 255 / 255 where it would report none, and on the diagonal.  Both
        orientations are stored.  filters.minP must be >= 1.
        -> (lo uint8[indptr[n]], hi uint8[indptr[n]], first uint32[n], indptr uint64[n + 1], n_records, n_pairs)."""
        n = self.n_variants - a0 if n is None else n
        _, layout_ptr = self.bandmat_layout(l_window, a0, n)          # (sizes the arrays; refuses what the call would refuse about the slice)
        nnz = int(layout_ptr[-1])
        lo, hi = np.empty(nnz, dtype=np.uint8), np.empty(nnz, dtype=np.uint8)
        first = np.zeros(n, dtype=np.uint32)
        indptr = np.zeros(n + 1, dtype=np.uint64)
        nrec, npairs = C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_dprime_ci_band(self._ctx, mode, C.byref(f), a0, n, tile_variants, l_window, lo.ctypes.data, hi.ctypes.data,
                                                        nnz, first.ctypes.data, indptr.ctypes.data, C.byref(nrec), C.byref(npairs)),
                    "twk_hip_ld_dprime_ci_band")
        return lo, hi, first, indptr, nrec.value, npairs.value

    def ld_blocks(self, mode: int, filters: Filters, l_window: int = 200000, params: BlockParams | None = None, a0: int = 0,
                  n: int | None = None, tile_variants: int = 0):
        """Haplotype blocks by the rule of Gabriel et al. (twk_hip_ld_blocks) over the variants [a0, a0 + n) in file order, from the
        bounds of ld_dprime_ci_band with the same arguments, selected on the device.  l_window is also the longest block in base pairs;
        params: a BlockParams (None: the defaults).  filters.minP must be >= 1.
        -> (block_of uint32[M], first uint32[B], last uint32[B], n_strong uint32[B], n_recomb uint32[B], n_candidates,
        n_informative, n_pairs); block_of is NO_BLOCK where a variant lies in no block, else its block's first variant."""
        M = self.n_variants
        n = M - a0 if n is None else n
        block_of = np.full(M, NO_BLOCK, dtype=np.uint32)
        per = [np.zeros(max(n // 2, 1), dtype=np.uint32) for _ in range(4)]
        nb, nc, ni, npairs = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        par = None if params is None else np.array(params.as_tuple(), dtype=np.uint32)
        self._check(self._lib.twk_hip_ld_blocks(self._ctx, mode, C.byref(f), a0, n, tile_variants, l_window, None if par is None else par.ctypes.data,
                                                block_of.ctypes.data, *(x.ctypes.data for x in per), C.byref(nb), C.byref(nc), C.byref(ni),
                                                C.byref(npairs)), "twk_hip_ld_blocks")
        return (block_of, *(x[:nb.value].copy() for x in per), nc.value, ni.value, npairs.value)

    def blocks_last(self) -> dict:
        """Of the last ld_blocks call (twk_hip_blocks_last, twk_hip_blocks_stages): the device time of the walk kernel and of the stages
        in front of it (prefix counts + candidate counts + scan, the emitting pass, the sort), and the size of the lo / hi band."""
        ms, b = C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_blocks_last(self._ctx, C.byref(ms), C.byref(b)), "twk_hip_blocks_last")
        counts, emit, sort = C.c_double(0), C.c_double(0), C.c_double(0)
        self._check(self._lib.twk_hip_blocks_stages(self._ctx, C.byref(counts), C.byref(emit), C.byref(sort)), "twk_hip_blocks_stages")
        return {"walk_ms": ms.value, "band_bytes": b.value, "counts_ms": counts.value, "emit_ms": emit.value, "sort_ms": sort.value}

    def ld_split(self, mode: int, filters: Filters, l_window: int, min_size: int, max_size: int, k_max: int, a0: int = 0,
                 n: int | None = None, tile_variants: int = 0, out=None):
        """LD splitting (twk_hip_ld_split): the slice [a0, a0 + n) - one contig - cut into K blocks of min_size .. max_size variants so
        that the r2 of ld_matrix_band(STAT_R2, fill 0) with the same arguments that crosses a cut is smallest, for every K up to k_max,
        solved on the device in integers of 2^-32.  filters.minP must be >= 1.  out: (total uint64[1], feasible uint8[k_max],
        cost uint64[k_max], cuts uint32[k_max * (k_max + 1)]) to be filled in place - a refused call and the rows of an infeasible K leave
        them as they are; None: fresh zeroed arrays.
        -> {"total": T, "feasible": uint8[k_max] (entry K - 1), "cost": uint64[k_max] (entry K - 1; 0 where infeasible),
        "cuts": [uint32[K + 1] for every feasible K, ascending], "K": the feasible K, "n_records", "n_pairs"}."""
        n = self.n_variants - a0 if n is None else n
        rows = int(k_max) if 1 <= int(k_max) <= 1024 else 0          # (outside 1 .. 1024 the call is refused and writes nothing)
        if out is None:
            out = (np.zeros(1, dtype=np.uint64), np.zeros(rows, dtype=np.uint8), np.zeros(rows, dtype=np.uint64),
                   np.zeros(rows * (rows + 1), dtype=np.uint32))
        total, feasible, cost, cuts = out
        assert total.dtype == np.uint64 and feasible.dtype == np.uint8 and cost.dtype == np.uint64 and cuts.dtype == np.uint32
        assert len(total) >= 1 and len(feasible) >= rows and len(cost) >= rows and len(cuts) >= rows * (rows + 1)
        nrec, npairs = C.c_uint64(0), C.c_uint64(0)
        f = filters._c()
        self._check(self._lib.twk_hip_ld_split(self._ctx, mode, C.byref(f), a0, n, tile_variants, l_window, min_size, max_size, k_max,
                                               total.ctypes.data, feasible.ctypes.data, cost.ctypes.data, cuts.ctypes.data,
                                               C.byref(nrec), C.byref(npairs)), "twk_hip_ld_split")
        ks = [K for K in range(1, rows + 1) if feasible[K - 1]]
        return {"total": int(total[0]), "feasible": feasible[:rows].copy(), "cost": cost[:rows].copy(),
                "cuts": [cuts[(K - 1) * (rows + 1):(K - 1) * (rows + 1) + K + 1].copy() for K in ks], "K": ks,
                "n_records": nrec.value, "n_pairs": npairs.value}

    def split_last(self) -> dict:
        """Of the last ld_split call (twk_hip_split_last): the device time of the band's launches, of row prefixes + block sums, of the
        layers and of the backtrack, and the device memory held."""
        band, sums, layers, back, b = C.c_double(0), C.c_double(0), C.c_double(0), C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_split_last(self._ctx, C.byref(band), C.byref(sums), C.byref(layers), C.byref(back), C.byref(b)), "twk_hip_split_last")
        return {"band_ms": band.value, "sums_ms": sums.value, "layers_ms": layers.value, "backtrack_ms": back.value, "bytes": b.value}

    def ld_topk(self, mode: int, filters: Filters, k: int, stat: int = STAT_R2, a0: int = 0, nA: int | None = None, b0: int = 0,
                nB: int | None = None, triangle: bool = True, part: int = 0, n_parts: int = 1, tile_variants: int = 0, window: int = 0,
                l_window: int = 0):
        """Top-k LD partners (twk_hip_ld_topk): for every variant the k partners with the largest |stat| among the records ld_region
        would report with the variant at either end - the value a float32 (the double rounded once: ld_matrix's bits), the order
        |value| descending, ties to the smaller partner index - selected on the device with integer atomic maxima: the same bytes for
        any tiling, order or repeat.  Slots not used hold (NO_PARTNER, +0.0).  1 <= k <= 32; filters.minP must be >= 1.  A shard
        returns the lists over its own pairs (topk_merge joins them).
        -> (idx uint32[M, k], val float32[M, k], n_pairs)."""
        M = self.n_variants
        nA = M - a0 if nA is None else nA
        nB = M - b0 if nB is None else nB
        kk = max(int(k), 0)
        idx = np.full((M, kk), NO_PARTNER, dtype=np.uint32)
        val = np.zeros((M, kk), dtype=np.float32)
        npairs = C.c_uint64(0)
        f = filters._c()
        # (a k the engine refuses is the engine's to refuse: it writes nothing before it has)
        self._check(self._lib.twk_hip_ld_topk(self._ctx, mode, C.byref(f), a0, nA, b0, nB, int(bool(triangle)), part, n_parts, tile_variants,
                                              int(window), l_window, int(stat), int(k), idx.ctypes.data, val.ctypes.data, C.byref(npairs)),
                    "twk_hip_ld_topk")
        return idx, val, npairs.value

    def topk_last(self) -> dict:
        """Of the last ld_topk call (twk_hip_topk_last): the time from the last launch's end to the unpacked lists, and the lists' size on the device."""
        ms, b = C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_topk_last(self._ctx, C.byref(ms), C.byref(b)), "twk_hip_topk_last")
        return {"unpack_ms": ms.value, "list_bytes": b.value}

    def relationship(self, stat: int = REL_KING, fill: float = float("nan"), variants=None, sA0: int = 0, nSA: int | None = None,
                     sB0: int = 0, nSB: int | None = None, want_counts: bool = False):
        """The sample relationship matrix (twk_hip_relationship) of the sample rows [sA0, sA0 + nSA) x columns [sB0, sB0 + nSB) over
        `variants` (indices as uploaded, strictly ascending; None: all): per pair, over the variants at which both samples are
        non-missing, the exact counts n, ibs0, ibs2, hethet, het_a, het_b and one statistic - REL_IBS (n + ibs2 - ibs0) / (2 n),
        REL_IBS0 ibs0 / n, REL_KING (hethet - 2 ibs0) / (het_a + het_b) - as one IEEE double division; `fill` (bit for bit) where
        the denominator is 0.  Transposed, contracted and divided on the device.
        -> float64 ndarray (nSA, nSB), or (that, REL_COUNTS_DTYPE ndarray (nSA, nSB)) with want_counts."""
        N = self.n_samples
        nSA = N - sA0 if nSA is None else nSA
        nSB = N - sB0 if nSB is None else nSB
        shape = (max(int(nSA), 0), max(int(nSB), 0))
        out = np.empty(shape, dtype=np.float64)
        cnt = np.zeros(shape, dtype=REL_COUNTS_DTYPE) if want_counts else None
        ids = None if variants is None else np.ascontiguousarray(variants, dtype=np.uint32)
        npairs = C.c_uint64(0)
        self._check(self._lib.twk_hip_relationship(self._ctx, None if ids is None else ids.ctypes.data, 0 if ids is None else len(ids),
                                                   sA0, nSA, sB0, nSB, int(stat), C.c_double(fill), out.ctypes.data, shape[1],
                                                   None if cnt is None else cnt.ctypes.data, shape[1], C.byref(npairs)), "twk_hip_relationship")
        return (out, cnt) if want_counts else out

    def relationship_last(self) -> dict:
        """Of the last relationship call (twk_hip_relationship_last): planes a sample (2: no variant in use had missing genotypes,
        3: one had), the transposition's device time and the plane set's size."""
        planes, ms, b = C.c_int32(0), C.c_double(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_relationship_last(self._ctx, C.byref(planes), C.byref(ms), C.byref(b)), "twk_hip_relationship_last")
        return {"planes_per_sample": planes.value, "transpose_ms": ms.value, "plane_bytes": b.value}

    def fisher_exact(self, tables: np.ndarray, ordered: bool = True):
        """Two-sided Fisher P of int32 tables [n, 4] = (n11, n12, n21, n22) through the engine's Fisher kernels
        (twk_hip_fisher_exact): as the engine runs them, the walks in the order of their length, or (ordered=False) in
        the order given - same P.  -> (P float64[n], kernel milliseconds)."""
        t = np.ascontiguousarray(tables, dtype=np.int32).reshape(-1, 4)
        out = np.zeros(len(t), dtype=np.float64)
        ms = C.c_float(0)
        self._check(self._lib.twk_hip_fisher_exact(self._ctx, t.ctypes.data, len(t), out.ctypes.data, 0 if ordered else 1,
                                                   C.byref(ms)), "twk_hip_fisher_exact")
        return out, float(ms.value)

    # ---- multi-GPU: survivors stay in HBM until the gather ----
    def set_device_sink(self, on: bool = True):
        """Region / all-vs-all calls keep their survivors on the device (twk_hip_set_device_sink); empties the buffer."""
        self._check(self._lib.twk_hip_set_device_sink(self._ctx, int(bool(on))), "twk_hip_set_device_sink")
        self._sink_on = bool(on)

    def device_records(self):
        """-> (device pointer, n records) of what the device sink holds (twk_hip_device_records)."""
        ptr, n = C.c_void_p(), C.c_uint64(0)
        self._check(self._lib.twk_hip_device_records(self._ctx, C.byref(ptr), C.byref(n)), "twk_hip_device_records")
        return (ptr.value or 0), n.value

    def drain_device_sink(self) -> np.ndarray:
        """The device sink's records on the host, in the order they lie in the sink; the sink is empty afterwards (twk_hip_drain_device_sink)."""
        chunks = []

        def sink(_user, recs, n):
            buf = (C.c_char * (n * RECORD_DTYPE.itemsize)).from_address(recs)
            chunks.append(np.frombuffer(buf, dtype=RECORD_DTYPE).copy())
            return 0

        cb = _SINK(sink)
        n = C.c_uint64(0)
        self._check(self._lib.twk_hip_drain_device_sink(self._ctx, cb, None, C.byref(n)), "twk_hip_drain_device_sink")
        out = np.concatenate(chunks) if chunks else np.zeros(0, dtype=RECORD_DTYPE)
        assert len(out) == n.value
        return out

    def device_records_tensor(self):
        """The device sink's records as a torch uint8 tensor [n * 104] that aliases the engine's HBM buffer (no copy):
        what tomahawk_amd.dist.gather_records sends over RCCL.  Valid until the next compute call."""
        import torch
        ptr, n = self.device_records()
        dev = torch.device("cuda", self.device)          # the context's own device, whatever torch's current one is
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device=dev)

        class _Span:          # the CUDA array interface is how torch wraps foreign device memory without owning it
            __cuda_array_interface__ = {"shape": (n * RECORD_DTYPE.itemsize,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        return torch.as_tensor(_Span(), device=dev)

    # ---- measurement ----
    def timing_reset(self):
        self._check(self._lib.twk_hip_timing_reset(self._ctx), "twk_hip_timing_reset")

    def launch_log(self, capacity: int = 4096):
        """The count launches since the last timing_reset, oldest first (twk_hip_launch_log) -> (list of dicts, launches seen)."""
        buf = (_LaunchStat * capacity)()
        n, total = C.c_uint32(0), C.c_uint64(0)
        self._check(self._lib.twk_hip_launch_log(self._ctx, buf, capacity, C.byref(n), C.byref(total)), "twk_hip_launch_log")
        return [{k: getattr(buf[i], k) for k, _ in _LaunchStat._fields_ if not k.startswith("_pad")} for i in range(n.value)], total.value

    def timing(self) -> dict:
        t = _Timing()
        self._check(self._lib.twk_hip_timing_get(self._ctx, C.byref(t)), "twk_hip_timing_get")
        return {k: getattr(t, k) for k, _ in _Timing._fields_}
