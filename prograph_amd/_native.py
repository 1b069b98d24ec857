"""
ctypes binding of libprograph_hip.so (include/prograph_hip.h) — the only way the package
reaches the GPU for the hot path.  torch tensors are used as device storage and for the
stream handle only.

There is NO CPU or eager fallback for the native entry points: if the shared library is
missing, was built for another ABI, or no HIP device is visible, every call raises
`NativeUnavailable` (a RuntimeError) with the reason.
"""
import ctypes
import os
import threading

import numpy as np
import torch   # must be imported before the library is loaded: see _load()

_HERE = os.path.dirname(os.path.abspath(__file__))
# PROGRAPH_HIP_LIB: load another build of the same ABI (kernel A/B comparisons, tools/ab.py)
LIB_PATH = os.environ.get("PROGRAPH_HIP_LIB") or os.path.join(_HERE, "libprograph_hip.so")
ABI_VERSION = 3

BITS_5, BITS_8 = 5, 8
CMP_LE, CMP_LT, CMP_EQ, CMP_GE, CMP_GT = 0, 1, 2, 3, 4
CMP_KEEP_ZERO = 0x10          # OR-ed into cmp of the fp16 / Minkowski / cosine / Euclidean eps entries: d = 0 (s = 1) is a hit
MAX_L, MAX_L_5BIT, MAX_K, MAX_K_ROUNDS, MAX_N_KNN, LEV_MAX_BAND = 128, 255, 63, 1023, 1 << 24, 8
SUB_MAX_L, SUB_MAX_A = 2048, 32   # pg_substitution_dense: positions per call, symbols of the cost table
ALN_MAX_L, ALN_MAX_GAP = 128, 255 # pg_alignment_dense: positions per operand, the largest gap penalty (tables as above)
ALN_MAX_OPEN = 255                # pg_alignment_affine_dense: the largest gap-open penalty
ALN_LOCAL_MIN, ALN_LOCAL_MAX = -128, 127    # pg_alignment_local_dense: the entries of a score table
ALN_LONG_MAX_L = 2048             # pg_alignment_long_dense / ..._local_long_dense / ..._semiglobal_long_dense: positions per operand
ALN_TRACE_GLOBAL, ALN_TRACE_LOCAL, ALN_TRACE_SEMIGLOBAL = 0, 1, 2     # pg_alignment_trace / pg_alignment_trace_long: the modes
ALN_TRACE_FIT = 3                 # pg_aln_trace.h's PG_TR_FIT: pg_alignment_fit_trace / _long, which take no mode
ALN_PROFILE_MODES = ("local", "semiglobal", "fit")      # pg_alignment_profile_dense / _long_dense: mode 0, 1, 2
ALN_TRACE_LONG_WORKSPACE = 2 << 30  # alignment_trace_long: the most workspace it takes unasked
LEV_LONG_MAX_L = 2048             # pg_levenshtein_long_dense: positions per operand
SPECTRUM_MAX_L, SPECTRUM_MAX_K, SPECTRUM_MAX_D = 2048, 6, 32768   # pg_spectrum_profile: positions per row, window length, profile width
ALN_LONG_CELL_MAX = 65535         # their cells are 16 bits wide (aln_long_fits / aln_local_long_fits / aln_semiglobal_long_fits)

# every symbol include/prograph_hip.h declares (tests check the library exports them all)
SYMBOLS = [
    "pg_version", "pg_last_error", "pg_device_info", "pg_npad", "pg_ngroups", "pg_nchunks", "pg_planes_bytes", "pg_workspace_bytes",
    "pg_pack_planes", "pg_pack_bytes",
    "pg_hamming_dense", "pg_eps_slots", "pg_scan_scratch_bytes", "pg_exclusive_scan",
    "pg_eps_compact", "pg_eps_fill_rows", "pg_eps_slots_sym", "pg_eps_compact_sym", "pg_knn_hamming", "pg_knn_sym_plan", "pg_knn_sym_plan_device", "pg_knn_hamming_round", "pg_index_flags", "pg_compact_flags",
    "pg_lev_profile", "pg_lev_candidates", "pg_lev_candidates_sym", "pg_lev_knn", "pg_csr_row_stats",
    "pg_levenshtein_dense", "pg_lev_eps_pairs", "pg_lev_eps_count", "pg_lev_eps_fill",
    "pg_lev_long_pack", "pg_levenshtein_long_dense",
    "pg_sub_pack", "pg_substitution_dense", "pg_alignment_dense", "pg_alignment_affine_dense",
    "pg_alignment_local_dense", "pg_alignment_long_workspace", "pg_alignment_long_dense", "pg_alignment_local_long_dense",
    "pg_alignment_semiglobal_dense", "pg_alignment_semiglobal_long_dense",
    "pg_alignment_fit_dense", "pg_alignment_fit_long_dense", "pg_alignment_fit_trace", "pg_alignment_fit_trace_long",
    "pg_alignment_profile_dense", "pg_alignment_profile_long_dense",
    "pg_alignment_trace_workspace", "pg_alignment_trace", "pg_alignment_trace_long_workspace", "pg_alignment_trace_long",
    "pg_alignment_stats", "pg_alignment_list_scores", "pg_alignment_list_long_scores",
    "pg_spectrum_dims", "pg_spectrum_profile",
    "pg_i32_knn", "pg_i32_knn_round", "pg_i32_eps_count", "pg_i32_eps_fill",
    "pg_comm_available", "pg_comm_unique_id", "pg_comm_init", "pg_comm_destroy", "pg_allgather_tokens",
    "pg_f16_nchunks", "pg_pack_f16", "pg_minkowski_dense", "pg_f16_knn", "pg_f16_knn_round", "pg_f16_eps_count",
    "pg_f16_eps_fill", "pg_minkowski_knn", "pg_minkowski_knn_round", "pg_minkowski_eps_slots", "pg_minkowski_eps_compact",
    "pg_minkowski_eps_fill_rows", "pg_cosine_prep", "pg_cosine_dense", "pg_cosine_knn", "pg_cosine_knn_round",
    "pg_cosine_eps_slots", "pg_cosine_eps_compact", "pg_cosine_eps_fill_rows",
    "pg_euclidean_dense", "pg_euclidean_knn", "pg_euclidean_knn_round", "pg_euclidean_eps_slots", "pg_euclidean_eps_fill_rows",
    "pg_query_workspace_bytes", "pg_query_knn_hamming",
    "pg_query_eps_segments", "pg_query_eps_count", "pg_query_eps_fill",
    "pg_csr_sort_workspace", "pg_csr_sort_rows_count", "pg_csr_sort_rows_fill", "pg_csr_histogram", "pg_csr_transpose_workspace",
    "pg_csr_transpose", "pg_csr_symmetrize_workspace", "pg_csr_symmetrize_count", "pg_csr_symmetrize_fill",
]


class NativeUnavailable(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()

_i64, _i32, _vp, _dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
_COS_METRICS = ("cosine", "euclidean")      # the metrics of pg_cos.hip: pg_<metric>_dense / _knn / _knn_round / _eps_*


def _load():
    """dlopen the library AFTER torch: hipcc stamps NEEDED libamdhip64.so.7 into it and torch
    ships a runtime with the same SONAME, so the loader binds us to the HIP runtime torch has
    already mapped.  One runtime per process is what makes torch-allocated pointers valid in
    our launches (SURVEY.md §7 hard part 1)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeUnavailable(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C prograph_amd/csrc` (hipcc, --offload-arch=gfx950)")
        try:
            lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:
            raise NativeUnavailable(f"cannot load {LIB_PATH}: {e}") from e
        missing = [s for s in SYMBOLS if not hasattr(lib, s)]
        if missing:
            raise NativeUnavailable(f"{LIB_PATH} does not export {missing}")
        lib.pg_version.restype = _i32
        if lib.pg_version() != ABI_VERSION:
            raise NativeUnavailable(f"ABI mismatch: library {lib.pg_version()}, binding {ABI_VERSION}")
        lib.pg_last_error.restype = ctypes.c_char_p
        lib.pg_npad.restype = _i64
        lib.pg_npad.argtypes = [_i64]
        lib.pg_ngroups.restype = _i32
        lib.pg_ngroups.argtypes = [_i32]
        lib.pg_nchunks.restype = _i32
        lib.pg_nchunks.argtypes = [_i32, _i32]
        lib.pg_planes_bytes.restype = _i64
        lib.pg_planes_bytes.argtypes = [_i64, _i32, _i32]
        lib.pg_scan_scratch_bytes.restype = _i64
        lib.pg_scan_scratch_bytes.argtypes = [_i64]
        lib.pg_workspace_bytes.restype = _i64
        lib.pg_workspace_bytes.argtypes = [_i64]
        lib.pg_device_info.argtypes = [ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.c_char_p, _i32]
        lib.pg_pack_planes.argtypes = [_vp, _i32, _i64, _i32, _i64, _vp, _i32, _vp, _i64, _vp, _vp]
        lib.pg_pack_bytes.argtypes = [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp]
        lib.pg_hamming_dense.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32, _i64, _i32, _vp]
        lib.pg_eps_slots.argtypes = [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i32,
                                     _vp, _vp, _vp, _vp, _vp]
        lib.pg_exclusive_scan.argtypes = [_vp, _i64, _vp, _vp, _vp]
        lib.pg_eps_slots_sym.argtypes = [_vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_eps_compact_sym.argtypes = [_vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _i32, _vp]
        lib.pg_eps_compact.argtypes = [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i32,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]
        lib.pg_eps_fill_rows.argtypes = [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _dbl,
                                         _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_knn_hamming.argtypes = [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp]
        lib.pg_knn_sym_plan.restype = _i64
        lib.pg_knn_sym_plan.argtypes = [_i64, _i64, _i32, _i32, _vp, _i64]
        lib.pg_knn_sym_plan_device.restype = _i64
        lib.pg_knn_sym_plan_device.argtypes = [_i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp]
        lib.pg_knn_hamming_round.argtypes = [_vp, _i64, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                             _vp, _vp, _vp]
        lib.pg_query_workspace_bytes.restype = _i64
        lib.pg_query_workspace_bytes.argtypes = [_i64, _i64, _i32]
        lib.pg_query_knn_hamming.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                             _i64, _vp]
        lib.pg_query_eps_segments.restype = _i64
        lib.pg_query_eps_segments.argtypes = [_i64, _i64]
        lib.pg_query_eps_count.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i64, _vp, _vp]
        lib.pg_query_eps_fill.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _dbl, _i64, _vp, _vp, _vp, _vp]
        lib.pg_index_flags.argtypes = [_vp, _i64, _i64, _i32, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_compact_flags.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp]
        lib.pg_csr_row_stats.argtypes = [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_csr_sort_workspace.restype = lib.pg_csr_transpose_workspace.restype = lib.pg_csr_symmetrize_workspace.restype = _i64
        lib.pg_csr_sort_workspace.argtypes = [_i64]
        lib.pg_csr_transpose_workspace.argtypes = lib.pg_csr_symmetrize_workspace.argtypes = [_i64, _i64]
        lib.pg_csr_sort_rows_count.argtypes = [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp]
        lib.pg_csr_sort_rows_fill.argtypes = [_vp, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
        lib.pg_csr_histogram.argtypes = [_vp, _i64, _i64, _vp, _vp]
        lib.pg_csr_transpose.argtypes = [_vp, _vp, _vp, _i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp]
        lib.pg_csr_symmetrize_count.argtypes = [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i64, _vp, _vp,
                                                _i64, _vp]
        lib.pg_csr_symmetrize_fill.argtypes = [_vp, _i64, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _i64, _vp]
        lib.pg_lev_profile.argtypes = [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _vp, _vp]
        lib.pg_lev_candidates.argtypes = [_vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp]
        lib.pg_lev_candidates_sym.argtypes = [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_lev_knn.argtypes = [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp]
        lib.pg_levenshtein_dense.argtypes = [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _i64, _vp]
        lib.pg_lev_eps_pairs.argtypes = [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_lev_eps_count.argtypes = [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]
        lib.pg_lev_eps_fill.argtypes = [_i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_lev_long_pack.argtypes = [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _vp, _vp]
        lib.pg_levenshtein_long_dense.argtypes = [_vp, _i64, _i64, _vp, _i32, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _i64, _vp]
        lib.pg_sub_pack.argtypes = [_vp, _i64, _i32, _i64, _i32, _vp, _i64, _vp, _vp]
        lib.pg_substitution_dense.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _vp]
        lib.pg_alignment_dense.argtypes = [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _i64, _i32, _vp]
        lib.pg_alignment_affine_dense.argtypes = [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _i32, _i32, _vp, _i64, _i32,
                                                  _vp]
        lib.pg_alignment_local_dense.argtypes = lib.pg_alignment_affine_dense.argtypes
        lib.pg_alignment_long_workspace.argtypes = [_i32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]
        lib.pg_alignment_long_dense.argtypes = [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _i32, _i32, _vp, _i64, _i32,
                                                _vp, _i64, _vp]
        lib.pg_alignment_local_long_dense.argtypes = lib.pg_alignment_long_dense.argtypes
        lib.pg_alignment_semiglobal_dense.argtypes = lib.pg_alignment_affine_dense.argtypes
        lib.pg_alignment_semiglobal_long_dense.argtypes = lib.pg_alignment_long_dense.argtypes
        lib.pg_alignment_fit_dense.argtypes = [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _i64,
                                               _i32, _vp]
        lib.pg_alignment_fit_long_dense.argtypes = [_vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _i32, _i32, _i32, _vp,
                                                    _i64, _i32, _vp, _i64, _vp]
        lib.pg_alignment_profile_dense.argtypes = [_i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32,
                                                   _i32, _vp, _i64, _i32, _vp]
        lib.pg_alignment_profile_long_dense.argtypes = lib.pg_alignment_profile_dense.argtypes[:-1] + [_vp, _i64, _vp]
        lib.pg_alignment_trace_workspace.argtypes = [_i32, _i32, ctypes.POINTER(_i64)]
        lib.pg_alignment_trace.argtypes = [_i32, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _i32, _i32,
                                           _vp, _vp, _i64, _vp, _i64, _vp]
        lib.pg_alignment_trace_long_workspace.argtypes = lib.pg_alignment_trace_workspace.argtypes
        lib.pg_alignment_trace_long.argtypes = lib.pg_alignment_trace.argtypes
        lib.pg_alignment_fit_trace.argtypes = lib.pg_alignment_trace.argtypes[1:]
        lib.pg_alignment_fit_trace_long.argtypes = lib.pg_alignment_trace.argtypes[1:]
        lib.pg_alignment_stats.argtypes = lib.pg_alignment_trace.argtypes[:16] + [_vp]
        lib.pg_alignment_list_scores.argtypes = [_i32, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp]
        lib.pg_alignment_list_long_scores.argtypes = [_i32, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _vp,
                                                      _vp, _i64, _vp]
        lib.pg_spectrum_dims.argtypes = [_i32, _i32, _i32]
        lib.pg_spectrum_profile.argtypes = [_vp, _i64, _i32, _i64, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _vp]
        lib.pg_i32_knn.argtypes = [_vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp]
        lib.pg_i32_knn_round.argtypes = [_vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp]
        lib.pg_i32_eps_count.argtypes = [_vp, _i64, _i64, _i64, _i32, _i64, _vp, _vp]
        lib.pg_i32_eps_fill.argtypes = [_vp, _i64, _i64, _i64, _i32, _i64, _vp, _vp, _vp, _vp]
        lib.pg_f16_nchunks.argtypes = [_i32]
        lib.pg_pack_f16.argtypes = [_vp, _i64, _i32, _i64, _vp, _vp, _i64, _vp]
        lib.pg_minkowski_dense.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _vp]
        lib.pg_f16_knn.argtypes = [_vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp]
        lib.pg_f16_knn_round.argtypes = [_vp, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp]
        lib.pg_f16_eps_count.argtypes = [_vp, _i64, _i64, _i64, _i32, ctypes.c_float, _i32, _vp, _vp]
        lib.pg_f16_eps_fill.argtypes = [_vp, _i64, _i64, _i64, _i32, ctypes.c_float, _i32, _vp, _vp, _vp, _vp]
        lib.pg_minkowski_knn.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp]
        lib.pg_minkowski_knn_round.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp,
                                               _i64, _vp]
        lib.pg_minkowski_eps_slots.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, ctypes.c_float, _i32,
                                               _vp, _vp, _vp, _vp]
        lib.pg_minkowski_eps_compact.argtypes = [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.pg_minkowski_eps_fill_rows.argtypes = [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, ctypes.c_float, _vp,
                                                   _i64, _vp, _vp, _vp, _vp]
        _ops = [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32]     # x, y operands of pg_cosine_* / pg_euclidean_*
        lib.pg_cosine_prep.argtypes = [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]
        lib.pg_cosine_eps_compact.argtypes = [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        for metric in _COS_METRICS:
            getattr(lib, f"pg_{metric}_dense").argtypes = _ops + [_vp, _i64, _vp]
            getattr(lib, f"pg_{metric}_knn").argtypes = _ops + [_i32, _i32, _vp, _vp, _vp]
            getattr(lib, f"pg_{metric}_knn_round").argtypes = _ops + [_i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp]
            getattr(lib, f"pg_{metric}_eps_slots").argtypes = _ops + [_i32, ctypes.c_float, _i32, _vp, _vp, _vp, _vp]
            getattr(lib, f"pg_{metric}_eps_fill_rows").argtypes = _ops + [_i32, ctypes.c_float, _vp, _i64, _vp, _vp, _vp, _vp]
        lib.pg_comm_unique_id.argtypes = [_vp]
        lib.pg_comm_init.argtypes = [ctypes.POINTER(_vp), _i32, _i32, _vp]
        lib.pg_comm_destroy.argtypes = [_vp]
        lib.pg_allgather_tokens.argtypes = [_vp, _vp, _i64, _i32, _vp, _vp]
        for name in SYMBOLS:
            fn = getattr(lib, name)
            if fn.restype is ctypes.c_int and name not in ("pg_version",):
                fn.restype = _i32
        _lib = lib
        return lib


def lib():
    return _load()


def device():
    """The device the hot path runs on: the current CUDA(HIP) device of this process."""
    if not torch.cuda.is_available():
        raise NativeUnavailable("no HIP device visible to torch; the Hamming/graph path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _check(rc, what):
    if rc != 0:
        msg = lib().pg_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr())


def workspace(nrows, dev):
    """Launch-private device state of one all-pairs call (pg_workspace_bytes): a fresh block per launch - torch's
    caching allocator hands a freed block out again only to later work on the same stream, which is exactly the
    reuse the ABI allows."""
    return torch.empty(int(lib().pg_workspace_bytes(int(nrows))), dtype=torch.uint8, device=dev)


def npad(n):
    return ((max(int(n), 1) + 255) // 256) * 256


def ngroups(l):
    return (max(int(l), 1) + 31) // 32


def nchunks(l, bits):
    return (ngroups(l) * int(bits) + 3) // 4


def planes_bytes(n, l, bits):
    """Chunk arrays + 64 bytes per sequence: signature section (MFMA column operand) + fold section."""
    return (nchunks(l, bits) * 16 + 64) * npad(n)


class Planes:
    """Device-resident token matrix as bit-sliced records (see include/prograph_hip.h).
    `flags`: the device word pg_pack_planes sets when a token does not fit the bit planes; `pack(check=False)`
    leaves reading it (one host sync) to the caller, `ensure_valid()` does it."""
    __slots__ = ("buf", "n", "l", "npad", "g", "q", "bits", "flags")

    def __init__(self, buf, n, l, bits, flags=None):
        self.buf, self.n, self.l, self.bits, self.flags = buf, int(n), int(l), int(bits), flags
        self.npad, self.g, self.q = npad(n), ngroups(l), nchunks(l, bits)

    def ensure_valid(self):
        if self.flags is not None and int(self.flags.item()):
            raise ValueError(f"tokens outside 0..{(1 << self.bits) - 1} cannot be packed with {self.bits} bit planes")
        self.flags = None

    @property
    def nbytes(self):
        return self.buf.numel()


def pack(tokens, rows=None, bits=None, width=None, check=True):
    """
    (N, L) integer tokens (torch tensor on the GPU, or anything np.asarray takes) -> Planes.
    `rows`: optional index list (the reference's `idxs`, prograph/prograph.py:726).
    `bits`: 5 or 8 bit planes per token; None picks 5 when every token is <= 31, else 8.
    `width`: pack as if the rows were zero right-padded to this length (clean_input's padding).
    Raises ValueError when a token does not fit a byte: such data is not "tokenized" and the
    caller must take the generic torch path.  `check=False` skips the host sync that reads the
    device-side validity word (callers in a pipeline read `Planes.flags` together with something
    else they wait for anyway, or call `ensure_valid()` later).
    """
    L = lib()
    dev = device()
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dim() != 2:
        raise ValueError("token matrix must be 2-D")
    if tokens.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise TypeError(f"integer tokens expected, got {tokens.dtype}")
    if tokens.dtype == torch.int8:
        tokens = tokens.to(torch.int16)
    tokens = tokens.to(dev).contiguous()
    n_src, l = tokens.shape
    lw = l if width is None else int(width)
    if lw < l:
        raise ValueError("width smaller than the token matrix")
    if lw > MAX_L_5BIT:
        raise ValueError(f"L={lw} exceeds the native limit of {MAX_L_5BIT}")
    ridx = None
    n = n_src
    if rows is not None:
        ridx = torch.as_tensor(np.asarray(rows), dtype=torch.int64).reshape(-1)
        if ridx.numel() and (int(ridx.min()) < -n_src or int(ridx.max()) >= n_src):
            raise IndexError("row index out of range")
        ridx = torch.where(ridx < 0, ridx + n_src, ridx).to(dev)
        n = int(ridx.numel())
    if n == 0 or l == 0:
        raise ValueError("empty token matrix")
    if bits is None:
        lo, hi = int(tokens.min()), int(tokens.max())
        if lo < 0 or hi > 255:
            raise ValueError("tokens outside 0..255 cannot use the byte-token Hamming path")
        bits = BITS_5 if hi <= 31 else BITS_8
    if lw > (MAX_L_5BIT if bits == BITS_5 else MAX_L):
        raise ValueError(f"L={lw} exceeds the native limit for {bits} bit planes")
    np_ = npad(n)
    if lw != l:
        wide = torch.zeros((n_src, lw), dtype=tokens.dtype, device=dev)   # clean_input's zero right-padding
        wide[:, :l] = tokens
        tokens = wide
    buf = torch.empty(planes_bytes(n, lw, bits), dtype=torch.uint8, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)      # (pg_pack_planes zeroes it on the stream)
    _check(L.pg_pack_planes(_ptr(tokens), tokens.element_size(), n, lw, tokens.stride(0), _ptr(ridx), int(bits),
                            _ptr(buf), np_, _ptr(flags), _stream()), "pg_pack_planes")
    planes = Planes(buf, n, lw, bits, flags)
    if check:
        planes.ensure_valid()
    return planes


def pack_bytes(raw, lut, bits=BITS_5, want_tokens=True, check=True):
    """
    Tokenise and pack on the device (pg_pack_bytes): `raw` = the fixed-width byte view of the sequence strings,
    (N, width) uint8 (host array or device tensor), `lut` = 256 table entries (letter -> token, else 0).
    Returns (Planes, tokens) with tokens = the (N, width) uint8 token matrix on the device, or None.
    """
    L = lib()
    dev = device()
    if not isinstance(raw, torch.Tensor):
        raw = torch.from_numpy(np.ascontiguousarray(np.asarray(raw, dtype=np.uint8)))
    if raw.dim() != 2 or raw.dtype != torch.uint8:
        raise TypeError("pack_bytes expects a 2-D uint8 byte matrix")
    raw = raw.to(dev).contiguous()
    n, width = raw.shape
    if n == 0 or width == 0:
        raise ValueError("empty byte matrix")
    if width > (MAX_L_5BIT if bits == BITS_5 else MAX_L):
        raise ValueError(f"L={width} exceeds the native limit for {bits} bit planes")
    lut_t = torch.as_tensor(np.asarray(lut, dtype=np.uint8).reshape(256)).to(dev)
    np_ = npad(n)
    buf = torch.empty(planes_bytes(n, width, bits), dtype=torch.uint8, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)      # (pg_pack_bytes zeroes it on the stream)
    tokens = torch.empty((n, width), dtype=torch.uint8, device=dev) if want_tokens else None
    _check(L.pg_pack_bytes(_ptr(raw), n, width, raw.stride(0), None, _ptr(lut_t), int(bits), _ptr(buf), np_, _ptr(tokens),
                           _ptr(flags), _stream()), "pg_pack_bytes")
    planes = Planes(buf, n, width, bits, flags)
    if check:
        planes.ensure_valid()
    return planes, tokens


_TORCH_OUT = {1: torch.uint8, 2: torch.float16, 4: torch.int32, 8: torch.int64}


def hamming_dense(xp, yp, out_bytes=8, out=None):
    """(M, N) distance matrix of every row of `yp` against every row of `xp` (hamming.py:34).
    With `out` given the distances are ADDED to it (segment-wise sums for long sequences)."""
    if xp.g != yp.g or xp.bits != yp.bits:
        raise ValueError("operands must be packed with the same width and bit planes")
    accumulate = out is not None
    if out is None:
        out = torch.empty((yp.n, xp.n), dtype=_TORCH_OUT[out_bytes], device=xp.buf.device)
    out_bytes = out.element_size()
    _check(lib().pg_hamming_dense(_ptr(xp.buf), xp.n, xp.npad, _ptr(yp.buf), yp.n, yp.npad, xp.g * 32, xp.bits,
                                  _ptr(out), out_bytes, out.stride(0), 1 if accumulate else 0, _stream()),
           "pg_hamming_dense")
    return out


def _bits2(rp, cp):
    if rp.bits != cp.bits or rp.g != cp.g:
        raise ValueError("row and column operands must be packed with the same width and bit planes")
    return rp.bits


def _csr_alloc(counts, wdtype, extra=None):
    """Per-row (or per-segment) int32 device counts -> (indptr int64 [m+1], indices int32 [nnz], weights wdtype [nnz]):
    the exclusive scan, ONE host sync that reads nnz, and the two allocations.  `extra`: a device scalar read in the
    same sync; then its value is returned fourth."""
    L = lib()
    m, dev = counts.numel(), counts.device
    indptr = torch.empty(m + 1, dtype=torch.int64, device=dev)
    scratch = torch.empty(int(L.pg_scan_scratch_bytes(m)), dtype=torch.uint8, device=dev)
    _check(L.pg_exclusive_scan(_ptr(counts), m, _ptr(indptr), _ptr(scratch), _stream()), "pg_exclusive_scan")
    if extra is None:
        nnz, also = int(indptr[-1].item()), ()
    else:
        nnz, *also = (int(v) for v in torch.stack([indptr[-1], extra]).cpu())
    indices = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
    weights = torch.empty(max(nnz, 1), dtype=wdtype, device=dev)[:nnz]
    return (indptr, indices, weights, *also)


def cat_csr(parts):
    """Row blocks of one CSR, each (indptr, indices, weights) counting from 0 -> the whole (pure torch).  A single
    part comes back as it is."""
    if len(parts) == 1:
        return parts[0]
    base, ptrs = 0, [torch.zeros(1, dtype=torch.int64, device=parts[0][0].device)]
    for indptr, _, _ in parts:
        ptrs.append(indptr[1:] + base)
        base += int(indptr[-1].item())
    return torch.cat(ptrs), torch.cat([p_[1] for p_ in parts]), torch.cat([p_[2] for p_ in parts])


def eps_graph(rp, cp, cmp, eps, row0=0, nrows=None, cap=256):
    """
    Epsilon-neighbourhood CSR of rows [row0, row0+nrows) of `rp` against all of `cp`.
    Returns device tensors (indptr int64 [nrows+1], indices int32 [nnz], weights uint8 [nnz]).
    ONE host sync (nnz and the number of rows that outgrew their slot) sits between the N^2 pass and
    the compaction: the output size is data dependent.  Rows with more matches than `cap` stay exact:
    a handful is recomputed inside the compaction kernel; more than that (dense graphs - most rows of
    a mutant library at eps >= 2) are listed on the device and the engine runs once more over just those
    rows, writing straight into the CSR (`pg_eps_fill_rows`).
    """
    L = lib()
    nrows = rp.n - row0 if nrows is None else int(nrows)
    dev = rp.buf.device
    bits = _bits2(rp, cp)
    cap = int(cap)
    symenv = os.environ.get("PG_EPS_SYM", "auto")            # 0 = never, 1 = whenever possible, auto = from 32k rows
    sym = (rp is cp and row0 == 0 and nrows == rp.n and rp.n < (1 << 27) and cap >= 2 and symenv != "0"
           and (symenv == "1" or rp.n >= 32768))          # whole square graph: every unordered pair once
    counts = torch.empty(nrows, dtype=torch.int32, device=dev)
    counts_lo = torch.empty(nrows, dtype=torch.int32, device=dev) if sym else None
    slot_idx = torch.empty(nrows * cap, dtype=torch.int32, device=dev)
    slot_w = torch.empty(nrows * cap, dtype=torch.uint8, device=dev)
    if sym:
        args = (_ptr(rp.buf), rp.npad, rp.n, rp.g * 32, bits, cmp, float(eps), cap, _ptr(slot_idx), _ptr(slot_w),
                _ptr(counts), _ptr(counts_lo))
        _check(L.pg_eps_slots_sym(*args, _ptr(workspace(nrows, dev)), _stream()), "pg_eps_slots_sym")
        total = counts + counts_lo
        over = (total > cap) | (counts_lo > 512)              # more than PG_SORT_MAX entries from below: not rank-sorted in LDS
    else:
        args = (_ptr(rp.buf), rp.npad, row0, nrows, _ptr(cp.buf), cp.npad, cp.n, cp.g * 32, bits, cmp, float(eps),
                cap, _ptr(slot_idx), _ptr(slot_w), _ptr(counts))
        _check(L.pg_eps_slots(*args, _ptr(workspace(nrows, dev)), _stream()), "pg_eps_slots")
        total = counts
        over = total > cap
    indptr, indices, weights, n_over = _csr_alloc(total, torch.uint8, extra=over.sum())     # the one sync
    if indices.numel():
        fill = n_over > int(os.environ.get("PG_FILL_MIN_ROWS", "8"))
        if sym:
            _check(L.pg_eps_compact_sym(*args, _ptr(indptr), _ptr(indices), _ptr(weights), 1 if fill else 0, _stream()),
                   "pg_eps_compact_sym")
        else:
            _check(L.pg_eps_compact(*args, _ptr(indptr), _ptr(indices), _ptr(weights), 1 if fill else 0, _stream()),
                   "pg_eps_compact")
        if fill:
            rows = compact_flags(over.to(torch.uint8), count=n_over)
            again = torch.empty(n_over, dtype=torch.int32, device=dev)
            _check(L.pg_eps_fill_rows(_ptr(rp.buf), rp.npad, row0, _ptr(rows), n_over, _ptr(cp.buf), cp.npad, cp.n,
                                      cp.g * 32, bits, cmp, float(eps), _ptr(indptr), _ptr(indices), _ptr(weights),
                                      _ptr(again), _ptr(workspace(n_over, dev)), _stream()), "pg_eps_fill_rows")
    return indptr, indices, weights


def eps_slots_only(rp, cp, cmp, eps, row0, nrows, cap, slot_idx, slot_w, counts):
    """Just the N^2 launch on preallocated buffers (bench.py times this)."""
    args = (_ptr(rp.buf), rp.npad, row0, nrows, _ptr(cp.buf), cp.npad, cp.n, cp.g * 32, _bits2(rp, cp), cmp,
            float(eps), int(cap))
    _check(lib().pg_eps_slots(*args, _ptr(slot_idx), _ptr(slot_w), _ptr(counts), _ptr(workspace(nrows, counts.device)), _stream()),
           "pg_eps_slots")


def knn_graph_rounds(rp, cp, k, row0=0, nrows=None):
    """k > 63: the canonical order is produced 63 + 64 + 64 ... ranks per all-pairs round, every
    round continuing after the previous round's last (distance, column) key."""
    L = lib()
    nrows = rp.n - row0 if nrows is None else int(nrows)
    dev = rp.buf.device
    bits = _bits2(rp, cp)
    idx = torch.empty((nrows, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nrows, k), dtype=torch.uint8, device=dev)
    keys_a = torch.empty(nrows, dtype=torch.int32, device=dev)
    keys_b = torch.empty(nrows, dtype=torch.int32, device=dev)
    done, first = 0, True
    while done < k:
        kk = min(63 if first else 64, k - done)
        ri = torch.empty((nrows, kk), dtype=torch.int32, device=dev)
        rd = torch.empty((nrows, kk), dtype=torch.uint8, device=dev)
        _check(L.pg_knn_hamming_round(_ptr(rp.buf), rp.npad, row0, nrows, _ptr(cp.buf), cp.npad, cp.n, cp.g * 32, bits,
                                      kk, 1 if first else 0, _ptr(keys_a), _ptr(keys_b), _ptr(ri), _ptr(rd),
                                      _ptr(workspace(nrows, dev)), _stream()),
               "pg_knn_hamming_round")
        idx[:, done:done + kk] = ri
        dist[:, done:done + kk] = rd
        keys_a, keys_b = keys_b, keys_a
        done += kk
        first = False
    return idx, dist


def knn_graph(rp, cp, k, row0=0, nrows=None, out=None):
    """(nrows, k) int32 indices and uint8 distances, ranks 1..k of the canonical order."""
    if k > MAX_K and out is None:
        return knn_graph_rounds(rp, cp, k, row0=row0, nrows=nrows)
    nrows = rp.n - row0 if nrows is None else int(nrows)
    dev = rp.buf.device
    if out is None:
        idx = torch.empty((nrows, k), dtype=torch.int32, device=dev)
        dist = torch.empty((nrows, k), dtype=torch.uint8, device=dev)
    else:
        idx, dist = out
    _check(lib().pg_knn_hamming(_ptr(rp.buf), rp.npad, row0, nrows, _ptr(cp.buf), cp.npad, cp.n, cp.g * 32,
                                _bits2(rp, cp), int(k), _ptr(idx), _ptr(dist), _ptr(workspace(nrows, dev)), _stream()),
           "pg_knn_hamming")
    return idx, dist


def query_knn(qp, dp, k):
    """Ranks 0..k-1 of every query row of `qp` against the database `dp` (pg_query_knn_hamming): (nq, k) int32 indices
    and uint8 distances in the canonical (distance, column) order, rank 0 kept.  k <= MAX_K_ROUNDS: rounds of 64
    ranks, each continuing after the previous round's last key.  Ranks that do not exist: -1 / 255."""
    if not 1 <= int(k) <= MAX_K_ROUNDS:
        raise ValueError(f"k must be in 1..{MAX_K_ROUNDS}")
    L = lib()
    bits = _bits2(qp, dp)
    dev = dp.buf.device
    k = int(k)
    idx = torch.empty((qp.n, k), dtype=torch.int32, device=dev)
    dist = torch.empty((qp.n, k), dtype=torch.uint8, device=dev)
    keys = [torch.empty(qp.n, dtype=torch.int32, device=dev) for _ in range(2)] if k > 64 else [None, None]
    done = 0
    while done < k:
        kk = min(64, k - done)
        ws_bytes = int(L.pg_query_workspace_bytes(qp.n, dp.n, kk))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        ri, rd = (idx, dist) if kk == k else (torch.empty((qp.n, kk), dtype=torch.int32, device=dev),
                                                torch.empty((qp.n, kk), dtype=torch.uint8, device=dev))
        _check(L.pg_query_knn_hamming(_ptr(qp.buf), qp.n, qp.npad, _ptr(dp.buf), dp.n, dp.npad, dp.g * 32, bits, kk,
                                      _ptr(keys[0]) if done else None, _ptr(keys[1]), _ptr(ri), _ptr(rd), _ptr(ws),
                                      ws_bytes, _stream()), "pg_query_knn_hamming")
        if kk != k:
            idx[:, done:done + kk] = ri
            dist[:, done:done + kk] = rd
        keys = keys[::-1]
        done += kk
    return idx, dist


def query_eps(qp, dp, cmp, eps, pieces=None):
    """The eps rows of every query row of `qp` against the database `dp` (pg_query_eps_count / _fill): the columns j with
    comp(d(q, j), eps) in ascending j, d = 0 kept.  Returns device tensors (indptr int64 [Q+1], indices int32 [nnz],
    weights uint8 [nnz]).  Two sweeps with a scan of the per-segment counts between them; ONE host sync (nnz) after the
    scan.  `pieces`: column pieces per query instead of the planned number (the same result; tests and measurements)."""
    L = lib()
    bits = _bits2(qp, dp)
    dev = dp.buf.device
    nseg = int(L.pg_query_eps_segments(qp.n, dp.n)) if pieces is None else 4 * int(pieces)
    ops = (_ptr(qp.buf), qp.n, qp.npad, _ptr(dp.buf), dp.n, dp.npad, dp.g * 32, bits, int(cmp), float(eps), nseg)
    m = qp.n * nseg
    counts = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    _check(L.pg_query_eps_count(*ops, _ptr(counts), _stream()), "pg_query_eps_count")
    seg_indptr, indices, weights = _csr_alloc(counts[:m], torch.uint8)          # the one sync
    if indices.numel():
        _check(L.pg_query_eps_fill(*ops, _ptr(seg_indptr), _ptr(indices), _ptr(weights), _stream()), "pg_query_eps_fill")
    return seg_indptr[::nseg].contiguous(), indices, weights


def index_flags(planes, ref, want=None, pos_mode=0, pos_mask=None, not_mask=None, want_dist_out=True,
                want_hist=True, want_flags=True):
    """Fused 1xN pass of Prograph.indexing; returns (dist uint8[n] | None, hist int64[256] | None, flags | None).
    `pos_mask` / `not_mask` are iterables of positions (selected / must-not-differ)."""
    dev = planes.buf.device
    n = planes.n
    dist = torch.empty(n, dtype=torch.uint8, device=dev) if want_dist_out else None
    hist = torch.zeros(256, dtype=torch.int64, device=dev) if want_hist else None
    flags = torch.empty(n, dtype=torch.uint8, device=dev) if want_flags else None
    wt = None
    if want is not None:
        bits = np.zeros(8, dtype=np.uint32)
        for d in want:
            d = int(d)
            if 0 <= d < 256:
                bits[d >> 5] |= np.uint32(1 << (d & 31))
        wt = torch.from_numpy(bits.view(np.int32)).to(dev)
    pm = nm = None
    if pos_mode:
        pm = torch.from_numpy(position_bitmask(pos_mask, planes.g).view(np.int32)).to(dev)
        nm = torch.from_numpy(position_bitmask(not_mask, planes.g).view(np.int32)).to(dev)
    _check(lib().pg_index_flags(_ptr(planes.buf), n, planes.npad, planes.l, planes.bits, int(ref), _ptr(wt),
                                int(pos_mode), _ptr(pm), _ptr(nm), _ptr(dist), _ptr(hist), _ptr(flags), _stream()),
           "pg_index_flags")
    return dist, hist, flags


def position_bitmask(positions, g):
    """uint32[g] with bit j of word w set for every position 32w+j in `positions`."""
    out = np.zeros(g, dtype=np.uint32)
    for p in positions:
        p = int(p)
        if not 0 <= p < 32 * g:
            raise IndexError(f"position {p} outside the packed width {32 * g}")
        out[p >> 5] |= np.uint32(1 << (p & 31))
    return out


def compact_flags(flags, count=None):
    """Ascending int64 indices of the non-zero entries of a uint8 device vector.  `count`: the number
    of non-zero entries when the caller already knows it (saves the host sync that reads it)."""
    L = lib()
    n = flags.numel()
    dev = flags.device
    out = torch.empty(n, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(int(L.pg_scan_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    _check(L.pg_compact_flags(_ptr(flags), n, _ptr(out), _ptr(cnt), _ptr(scratch), _stream()), "pg_compact_flags")
    return out[: int(cnt.item()) if count is None else int(count)]


def levenshtein_knn(tokens, k, band=8, row0=0, nrows=None, cap=512, return_stats=False):
    """
    Banded (capped) Levenshtein kNN — build defined, BASELINE.json configs[4] (no reference
    counterpart).  `tokens`: (N, L<=128) uint8, tokens 1..31, zero right-padded.
    Returns (idx int32 (nrows,k), dist uint8 (nrows,k)): ranks 1..k of the (d, column) order with
    d = min(edit distance, band+1).
    Invalid input (a token above 31, an interior zero) raises ValueError - after the candidate pass: the validity
    word of the profile kernel is read together with the largest candidate count (the step's ONE host sync), so a
    bad matrix costs one filter sweep before it is rejected (the kernels mask symbols, nothing goes out of bounds).
    """
    L = lib()
    dev = device()
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dtype != torch.uint8 or tokens.dim() != 2:
        raise TypeError("levenshtein_knn expects a 2-D uint8 token matrix")
    tokens = tokens.to(dev).contiguous()
    n, l = tokens.shape
    nrows = n - row0 if nrows is None else int(nrows)
    np_ = npad(n)
    prof = torch.empty(3 * np_ * 16, dtype=torch.uint8, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(L.pg_lev_profile(_ptr(tokens), n, l, tokens.stride(0), _ptr(prof), np_, _ptr(lens), _ptr(flags), _stream()),
           "pg_lev_profile")
    if l > 128:
        raise ValueError("levenshtein_knn: at most 128 tokens per sequence")
    planes = pack(tokens, bits=BITS_5, width=128, check=False)   # chunk p of a record = bit plane p (128 bits)
    counts = torch.empty(nrows, dtype=torch.int32, device=dev)
    symenv = os.environ.get("PG_EPS_SYM", "auto")            # the filter is symmetric like the eps graph
    sym = row0 == 0 and nrows == n and n < (1 << 24) and symenv != "0" and (symenv == "1" or n >= 32768)
    counts_lo = torch.empty(nrows, dtype=torch.int32, device=dev) if sym else None
    passes = 0
    while True:
        passes += 1
        slot_idx = torch.empty(nrows * cap, dtype=torch.int32, device=dev)
        slot_w = torch.empty(nrows * cap, dtype=torch.uint8, device=dev)
        slot_aux = torch.empty(nrows * cap, dtype=torch.int32, device=dev) if sym else None
        if sym:
            _check(L.pg_lev_candidates_sym(_ptr(prof), np_, n, int(band), int(cap), _ptr(slot_idx), _ptr(slot_w),
                                           _ptr(slot_aux), _ptr(counts), _ptr(counts_lo), _stream()), "pg_lev_candidates_sym")
            tot = counts + counts_lo
        else:
            _check(L.pg_lev_candidates(_ptr(prof), np_, n, row0, nrows, int(band), int(cap), _ptr(slot_idx),
                                       _ptr(slot_w), _ptr(counts), _stream()), "pg_lev_candidates")
            tot = counts
        # the ONE host sync of a step: the token check of the profile pass and the largest candidate count
        bad, mx = (int(v) for v in torch.stack([(flags[0] | planes.flags[0]).to(torch.int64), tot.max().to(torch.int64)]).cpu())
        if bad:
            raise ValueError("levenshtein_knn: tokens must be 1..31 with zeros only as right padding")
        if mx <= cap:
            break
        cap = ((mx + 63) // 64) * 64          # some row has more candidates than slots: redo with room
    idx = torch.empty((nrows, k), dtype=torch.int32, device=dev)
    dist = torch.empty((nrows, k), dtype=torch.uint8, device=dev)
    _check(L.pg_lev_knn(_ptr(tokens), n, l, tokens.stride(0), _ptr(planes.buf), planes.npad, _ptr(lens), row0, nrows,
                        int(band), int(k), int(cap),
                        _ptr(slot_idx), _ptr(slot_w), _ptr(slot_aux), _ptr(counts), _ptr(counts_lo), _ptr(idx), _ptr(dist),
                        _stream()), "pg_lev_knn")
    if return_stats:
        ncand = int(counts.to(torch.int64).sum().item()) + (int(counts_lo.to(torch.int64).sum().item()) if sym else 0)
        return idx, dist, {"candidates": ncand, "cap": cap, "filter_passes": passes, "symmetric": bool(sym)}
    return idx, dist


class LevOperand:
    """A token matrix staged for the exact Levenshtein kernels: `tokens` (n, l <= 128) uint8 on the device, `planes` (5 bit
    planes at width 128), `lens` int32 [n], `prof` (pg_lev_profile's bag profiles) and the two validity words."""
    __slots__ = ("tokens", "planes", "lens", "prof", "flags", "n", "l")

    def __init__(self, tokens, planes, lens, prof, flags):
        self.tokens, self.planes, self.lens, self.prof, self.flags = tokens, planes, lens, prof, flags
        self.n, self.l = int(tokens.shape[0]), int(tokens.shape[1])

    def bad_word(self):
        """Device int64 scalar, non-zero when a token is above 31 or a zero is not trailing padding."""
        return (self.flags[0] | self.planes.flags[0]).to(torch.int64)

    def valid(self):
        """One host sync: do the kernels' preconditions hold?"""
        return int(self.bad_word().item()) == 0


def lev_operand(tokens):
    """(N, L <= 128) uint8 tokens -> LevOperand (pg_lev_profile + pg_pack_planes at width 128).  No host sync: ask
    `valid()` before trusting a result computed from it (the kernels mask symbols and clamp lengths, so an invalid
    operand gives wrong numbers, never an out-of-bounds access)."""
    L = lib()
    dev = device()
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dtype != torch.uint8 or tokens.dim() != 2 or tokens.shape[0] == 0 or tokens.shape[1] == 0:
        raise TypeError("lev_operand expects a non-empty 2-D uint8 token matrix")
    if tokens.shape[1] > 128:
        raise ValueError("lev_operand: at most 128 tokens per sequence")
    tokens = tokens.to(dev).contiguous()
    n, l = tokens.shape
    np_ = npad(n)
    prof = torch.empty(3 * np_ * 16, dtype=torch.uint8, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(L.pg_lev_profile(_ptr(tokens), n, l, tokens.stride(0), _ptr(prof), np_, _ptr(lens), _ptr(flags), _stream()),
           "pg_lev_profile")
    planes = pack(tokens, bits=BITS_5, width=128, check=False)   # chunk p of a record = bit plane p (128 bits)
    return LevOperand(tokens, planes, lens, prof, flags)


def levenshtein_dense(xo, yo, out_bytes=8, rows=None):
    """(M, N) exact edit distances of the rows of LevOperand `yo` (rows = (r0, r1): only those) against every row of `xo`
    (pg_levenshtein_dense): int64 (out_bytes 8) or the fp16 block f16_knn / f16_eps select from (2)."""
    r0, r1 = (0, yo.n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= yo.n:
        raise ValueError("row range outside the operand")
    out = torch.empty((r1 - r0, xo.n), dtype=_TORCH_OUT[out_bytes], device=xo.tokens.device)
    _check(lib().pg_levenshtein_dense(_ptr(xo.planes.buf), xo.n, xo.planes.npad, _ptr(xo.lens),
                                      ctypes.c_void_p(yo.planes.buf.data_ptr() + 16 * r0), r1 - r0, yo.planes.npad,
                                      ctypes.c_void_p(yo.lens.data_ptr() + 4 * r0), max(xo.l, yo.l), _ptr(out), out_bytes,
                                      out.stride(0), _stream()), "pg_levenshtein_dense")
    return out


class LevLongOperand:
    """A token matrix staged for pg_levenshtein_long_dense (pg_lev_long_pack): `tokens` (n, l <= 2048) uint8 on the device,
    `buf` = ceil(l / 128) blocks x 5 bit planes x npad uint4 (block b is a 128-position operand), `lens` int32 [n] and
    the validity word."""
    __slots__ = ("tokens", "buf", "lens", "flags", "n", "l", "npad")

    def __init__(self, tokens, buf, lens, flags):
        self.tokens, self.buf, self.lens, self.flags = tokens, buf, lens, flags
        self.n, self.l = int(tokens.shape[0]), int(tokens.shape[1])
        self.npad = npad(self.n)

    def bad_word(self):
        """Device int64 scalar, non-zero when a token is above 31 or a zero is not trailing padding."""
        return self.flags[0].to(torch.int64)

    def valid(self):
        """One host sync: do the kernel's preconditions hold?"""
        return int(self.bad_word().item()) == 0


def lev_long_ready():
    """Can the Levenshtein kernel beyond 128 positions run (`levenshtein_long_dense`)?  True only with a HIP device; the
    routes of prograph.py and the operator ask before they leave the 128-position kernels / the torch expression."""
    try:
        return device().type == "cuda"
    except NativeUnavailable:
        return False


def lev_long_operand(tokens):
    """(N, L <= 2048) uint8 tokens -> LevLongOperand (pg_lev_long_pack).  No host sync: ask `valid()` before trusting a
    result computed from it (the kernel masks symbols and clamps lengths, so an invalid operand gives wrong numbers,
    never an out-of-bounds access)."""
    L = lib()
    dev = device()
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dtype != torch.uint8 or tokens.dim() != 2 or tokens.shape[0] == 0 or tokens.shape[1] == 0:
        raise TypeError("lev_long_operand expects a non-empty 2-D uint8 token matrix")
    if tokens.shape[1] > LEV_LONG_MAX_L:
        raise ValueError(f"lev_long_operand: at most {LEV_LONG_MAX_L} tokens per sequence")
    tokens = tokens.to(dev).contiguous()
    n, l = tokens.shape
    np_ = npad(n)
    buf = torch.empty(((l + 127) // 128) * 5 * np_ * 16, dtype=torch.uint8, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)       # (pg_lev_long_pack zeroes it on the stream)
    _check(L.pg_lev_long_pack(_ptr(tokens), n, l, tokens.stride(0), _ptr(buf), np_, _ptr(lens), _ptr(flags), _stream()),
           "pg_lev_long_pack")
    return LevLongOperand(tokens, buf, lens, flags)


def levenshtein_long_dense(xo, yo, out_bytes=8, rows=None):
    """(M, N) exact edit distances of the rows of LevLongOperand `yo` (rows = (r0, r1): only those) against every row of
    `xo` (pg_levenshtein_long_dense), each operand at its own width of up to 2048 positions: int64 (out_bytes 8) or the
    fp16 block f16_knn / f16_eps select from (2; a distance is at most 2048: exact)."""
    if out_bytes not in (2, 8):
        raise ValueError("levenshtein_long_dense: out_bytes 8 (int64) or 2 (fp16)")
    r0, r1 = (0, yo.n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= yo.n:
        raise ValueError("row range outside the operand")
    out = torch.empty((r1 - r0, xo.n), dtype=_TORCH_OUT[out_bytes], device=xo.tokens.device)
    _check(lib().pg_levenshtein_long_dense(_ptr(xo.buf), xo.n, xo.npad, _ptr(xo.lens), xo.l,
                                           ctypes.c_void_p(yo.buf.data_ptr() + 16 * r0), r1 - r0, yo.npad,
                                           ctypes.c_void_p(yo.lens.data_ptr() + 4 * r0), yo.l, _ptr(out), out_bytes,
                                           out.stride(0), _stream()), "pg_levenshtein_long_dense")
    return out


def levenshtein_eps(op, cmp, thr, cap=512, keep_zero=False):
    """Epsilon graph of all rows of a LevOperand under the exact edit distance: the entries with comp(d, thr) and d > 0
    (d >= 0 with keep_zero), comp = CMP_LE / CMP_LT / CMP_EQ, integer thr in 0..LEV_MAX_BAND.  The bag filter with
    band = thr over every unordered pair, the banded distance of every candidate pair once (exact where it is within the
    band), then count / scan / fill.  Two host syncs: the filter's largest candidate count with the token check (a row
    with more candidates than `cap` reruns the filter with room), and the CSR size.
    Returns (indptr int64 [n+1], indices int32 ascending within a row, weights uint8).  ValueError for invalid tokens."""
    L = lib()
    if cmp not in (CMP_LE, CMP_LT, CMP_EQ) or int(thr) != thr or not 0 <= thr <= LEV_MAX_BAND:
        raise ValueError("levenshtein_eps: comp le / lt / eq with an integer threshold in 0..8")
    n, thr, cap = op.n, int(thr), int(cap)
    if n >= (1 << 27):
        raise ValueError("levenshtein_eps: n must be below 2^27")
    dev = op.tokens.device
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    counts_lo = torch.empty(n, dtype=torch.int32, device=dev)
    while True:
        slot_idx = torch.empty(n * cap, dtype=torch.int32, device=dev)
        slot_w = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        slot_aux = torch.empty(n * cap, dtype=torch.int32, device=dev)
        _check(L.pg_lev_candidates_sym(_ptr(op.prof), op.planes.npad, n, thr, cap, _ptr(slot_idx), _ptr(slot_w), _ptr(slot_aux),
                                       _ptr(counts), _ptr(counts_lo), _stream()), "pg_lev_candidates_sym")
        bad, mx = (int(v) for v in torch.stack([op.bad_word(), (counts + counts_lo).max().to(torch.int64)]).cpu())
        if bad:
            raise ValueError("levenshtein_eps: tokens must be 1..31 with zeros only as right padding")
        if mx <= cap:
            break
        cap = ((mx + 63) // 64) * 64          # some row has more candidates than slots: redo with room
    _check(L.pg_lev_eps_pairs(_ptr(op.tokens), n, op.l, op.tokens.stride(0), _ptr(op.planes.buf), op.planes.npad, _ptr(op.lens),
                              thr, cap, _ptr(slot_idx), _ptr(slot_w), _ptr(slot_aux), _ptr(counts), _ptr(counts_lo), _stream()),
           "pg_lev_eps_pairs")
    code = int(cmp) | (CMP_KEEP_ZERO if keep_zero else 0)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    _check(L.pg_lev_eps_count(n, cap, code, thr, _ptr(slot_w), _ptr(counts), _ptr(counts_lo), _ptr(kept), _stream()),
           "pg_lev_eps_count")
    indptr, indices, weights = _csr_alloc(kept, torch.uint8)
    if indices.numel():
        _check(L.pg_lev_eps_fill(n, cap, code, thr, _ptr(slot_idx), _ptr(slot_w), _ptr(counts), _ptr(counts_lo), _ptr(indptr),
                                 _ptr(indices), _ptr(weights), _stream()), "pg_lev_eps_fill")
    return indptr, indices, weights


class SubOperand:
    """A token matrix staged for pg_substitution_dense (pg_sub_pack): `buf` int32 [ceil(l / 4) * npad], dword g of sequence
    c at g * npad + c, and the validity word (non-zero: a token is outside the cost table)."""
    __slots__ = ("buf", "n", "l", "npad", "flags")

    def __init__(self, buf, n, l, flags):
        self.buf, self.n, self.l, self.npad, self.flags = buf, int(n), int(l), npad(n), flags

    def valid(self):
        """One host sync: is every token an index of the table it was packed for?"""
        return int(self.flags.item()) == 0


def sub_cost(table):
    """(A, A) integer cost table, A <= 32, entries 0..255 -> the 32 x 32 uint8 device table of pg_substitution_dense."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[0] != t.shape[1] or not 1 <= t.shape[0] <= SUB_MAX_A or t.min() < 0 or t.max() > 255:
        raise ValueError("cost table: square, at most 32 symbols, entries 0..255")
    full = np.zeros((SUB_MAX_A, SUB_MAX_A), dtype=np.uint8)
    full[:t.shape[0], :t.shape[0]] = t
    return torch.from_numpy(full).to(device())


def sub_operand(tokens, a):
    """(N, L <= 2048) uint8 tokens -> SubOperand for a table of `a` symbols.  No host sync: ask `valid()` before trusting a
    result computed from it (the kernel masks tokens, so an invalid operand gives wrong numbers, nothing else)."""
    dev = device()
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dtype != torch.uint8 or tokens.dim() != 2 or tokens.shape[0] == 0 or tokens.shape[1] == 0:
        raise TypeError("sub_operand expects a non-empty 2-D uint8 token matrix")
    if tokens.shape[1] > SUB_MAX_L:
        raise ValueError(f"sub_operand: at most {SUB_MAX_L} tokens per sequence")
    tokens = tokens.to(dev).contiguous()
    n, l = tokens.shape
    np_ = npad(n)
    buf = torch.empty(((l + 3) // 4) * np_, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(lib().pg_sub_pack(_ptr(tokens), n, l, tokens.stride(0), int(a), _ptr(buf), np_, _ptr(flags), _stream()), "pg_sub_pack")
    return SubOperand(buf, n, l, flags)


def substitution_dense(xo, yo, cost, out_bytes=8, rows=None, out=None, cols=None):
    """(M, N) substitution distances of the rows of SubOperand `yo` (rows = (r0, r1): only those) against every row of
    `xo` (pg_substitution_dense); `cost` from sub_cost.  int64 (out_bytes 8), int32 (4) or the fp16 block f16_knn /
    f16_eps select from (2: exact while the distances stay within 2048).  With `out` given the distances are ADDED to
    it; cols = (p0, p1), p0 a multiple of 4: only those positions (a distance is the sum over column segments)."""
    if xo.l != yo.l:
        raise ValueError("operands must be packed at the same width")
    r0, r1 = (0, yo.n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= yo.n:
        raise ValueError("row range outside the operand")
    p0, p1 = (0, xo.l) if cols is None else (int(cols[0]), int(cols[1]))
    if not 0 <= p0 < p1 <= xo.l or p0 % 4:
        raise ValueError("column segment outside the operand, or not from a multiple of 4 on")
    accumulate = out is not None
    if out is None:
        out = torch.empty((r1 - r0, xo.n), dtype=_TORCH_OUT[out_bytes], device=xo.buf.device)
    elif out.shape != (r1 - r0, xo.n) or out.stride(1) != 1:
        raise ValueError("out must be a (rows, N) matrix with contiguous rows")
    _check(lib().pg_substitution_dense(ctypes.c_void_p(xo.buf.data_ptr() + 4 * (p0 // 4) * xo.npad), xo.n, xo.npad,
                                       ctypes.c_void_p(yo.buf.data_ptr() + 4 * ((p0 // 4) * yo.npad + r0)), r1 - r0,
                                       yo.npad, p1 - p0, _ptr(cost), _ptr(out), out.stride(0), out.element_size(),
                                       1 if accumulate else 0, _stream()), "pg_substitution_dense")
    return out


class AlnOperand(SubOperand):
    """A token matrix staged for pg_alignment_dense: the transposed dwords and validity word of a SubOperand, at most
    ALN_MAX_L positions.  The kernel finds the sequence lengths (last non-zero + 1) in these dwords itself."""
    __slots__ = ()


def aln_operand(tokens, a):
    """(N, L <= 128) uint8 tokens -> AlnOperand for a table of `a` symbols (pg_sub_pack).  No host sync: ask `valid()`
    before trusting a result computed from it (the kernel masks tokens, so an invalid operand gives wrong numbers, nothing
    else)."""
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dim() == 2 and tokens.shape[1] > ALN_MAX_L:
        raise ValueError(f"aln_operand: at most {ALN_MAX_L} tokens per sequence")
    so = sub_operand(tokens, a)
    return AlnOperand(so.buf, so.n, so.l, so.flags)


def _aln_dense(entry, name, xo, yo, table, penalties, out_bytes, rows, long=False):
    """One dense alignment entry: the rows (r0, r1) of `yo` against every row of `xo`; `penalties` are the entry's integers
    between the table and `out` (gap[, gap_open[, bias]]).  `long`: int32 | int64 out and the call's workspace (the entries
    beyond 128 positions), else fp16 | int64."""
    small = 4 if long else 2
    if out_bytes not in (small, 8):
        raise ValueError(f"{name}: out_bytes 8 (int64) or {small} ({'int32' if long else 'fp16'})")
    r0, r1 = (0, yo.n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= yo.n:
        raise ValueError("row range outside the operand")
    out = torch.empty((r1 - r0, xo.n), dtype=_TORCH_OUT[out_bytes], device=xo.buf.device)
    tail = ()
    if long:
        ws = aln_long_workspace(xo, r1 - r0)
        tail = (_ptr(ws), ws.numel())
    _check(getattr(lib(), entry)(_ptr(xo.buf), xo.n, xo.npad, xo.l, ctypes.c_void_p(yo.buf.data_ptr() + 4 * r0), r1 - r0,
                                 yo.npad, yo.l, _ptr(table), *(int(v) for v in penalties), _ptr(out), out.stride(0), out_bytes,
                                 *tail, _stream()), entry)
    return out


def alignment_dense(xo, yo, cost, gap, out_bytes=8, rows=None):
    """(M, N) gapped alignment distances of the rows of AlnOperand `yo` (rows = (r0, r1): only those) against every row
    of `xo` (pg_alignment_dense); `cost` from sub_cost, `gap` 1..255; the operands' widths need not agree.  int64
    (out_bytes 8) or the fp16 block f16_knn / f16_eps select from (2: exact while the distances stay within 2048)."""
    return _aln_dense("pg_alignment_dense", "alignment_dense", xo, yo, cost, (gap,), out_bytes, rows)


def alignment_affine_dense(xo, yo, cost, gap, gap_open, out_bytes=8, rows=None):
    """`alignment_dense` with affine gap penalties (pg_alignment_affine_dense): a run of g unaligned symbols costs
    gap_open + g * gap, `gap` 1..255, `gap_open` 0..255 (0: the distances of `alignment_dense`).  Same AlnOperands, row
    range and outputs; fp16 is exact while width * max(max C, gap) + gap_open stays within 2048."""
    return _aln_dense("pg_alignment_affine_dense", "alignment_affine_dense", xo, yo, cost, (gap, gap_open), out_bytes, rows)


def aln_local_score(table):
    """(A, A) integer score table, A <= 32, entries -128..127 -> the 32 x 32 int8 device table of pg_alignment_local_dense."""
    t = np.asarray(table)
    if (t.ndim != 2 or t.shape[0] != t.shape[1] or not 1 <= t.shape[0] <= SUB_MAX_A or t.min() < ALN_LOCAL_MIN
            or t.max() > ALN_LOCAL_MAX):
        raise ValueError("score table: square, at most 32 symbols, entries -128..127")
    full = np.zeros((SUB_MAX_A, SUB_MAX_A), dtype=np.int8)
    full[:t.shape[0], :t.shape[0]] = t
    return torch.from_numpy(full).to(device())


def alignment_local_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    """(M, N) local alignment SCORES (larger is nearer) of the rows of AlnOperand `yo` (rows = (r0, r1): only those)
    against every row of `xo` (pg_alignment_local_dense); `score` from aln_local_score, `gap` 1..255, `gap_open` 0..255;
    the operands' widths need not agree.  int64 (out_bytes 8) or the fp16 block f16_knn / f16_eps select from (2: exact
    while width * max(S) stays within 2048)."""
    return _aln_dense("pg_alignment_local_dense", "alignment_local_dense", xo, yo, score, (gap, gap_open), out_bytes, rows)


def alignment_semiglobal_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    """(M, N) semi-global alignment SCORES (both sequences end to end, free end gaps; larger is nearer) of the rows of
    AlnOperand `yo` (rows = (r0, r1): only those) against every row of `xo` (pg_alignment_semiglobal_dense); arguments and
    outputs as `alignment_local_dense`, `score` from aln_local_score."""
    return _aln_dense("pg_alignment_semiglobal_dense", "alignment_semiglobal_dense", xo, yo, score, (gap, gap_open), out_bytes, rows)


def aln_long_ready():
    """Can the kernels beyond 128 positions run (`alignment_long_dense`, `i32_knn`, ...)?  True only with a HIP device;
    the routes of prograph.py and the operators ask before they leave the 128-position kernels / the torch expression."""
    try:
        return device().type == "cuda"
    except NativeUnavailable:
        return False


def aln_long_fits(width, max_cost, gap, gap_open):
    """Do `alignment` distances of operands up to `width` positions fit the 16-bit cells of pg_alignment_long_dense?  A
    cell is at most width * max_cost + gap_open (max_cost = max(max C, gap)), E and F one gap_open + gap above it, and
    the sums formed before a min add gap once more."""
    return width <= ALN_LONG_MAX_L and width * max_cost + 2 * gap_open + 2 * gap <= ALN_LONG_CELL_MAX


def aln_local_long_fits(width_x, width_y, max_score):
    """The same for `local_alignment` scores: a cell is at most min(width) * max(S), the diagonal term adds a profile
    byte (at most 255) before the bias comes off."""
    return max(width_x, width_y) <= ALN_LONG_MAX_L and min(width_x, width_y) * max_score + 255 <= ALN_LONG_CELL_MAX


def aln_semiglobal_long_fits(width_x, width_y, max_score):
    """The same for `semiglobal_alignment` scores: a cell holds score + Z, Z = min(width) * max(S), a score is at most Z,
    and the diagonal term adds a profile byte (at most 255) before the bias comes off."""
    return (max(width_x, width_y) <= ALN_LONG_MAX_L
            and 2 * min(width_x, width_y) * max(int(max_score), 0) + 255 <= ALN_LONG_CELL_MAX)


def aln_fit_fits(width_x, width_y, max_score, gap, gap_open):
    """Do `fit_alignment` scores fit the 16-bit cells of pg_alignment_fit_dense AND pg_alignment_fit_long_dense?  A cell holds
    score + Z, Z = gap_open + width_y * (gap + max(0, max S)) (the Y operand is the whole one), a score is at most
    width_y * max(S), and the diagonal term adds a profile byte (at most 255) before the bias comes off.  Unlike the other
    modes the short kernel needs it too: 128 positions at 255 / 255 / 127 give 65 662."""
    top = max(int(max_score), 0)
    return (max(width_x, width_y) <= ALN_LONG_MAX_L
            and int(gap_open) + int(width_y) * (int(gap) + 2 * top) + 255 <= ALN_LONG_CELL_MAX)


def alignment_fit_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None, bias=0):
    """(M, N) fit alignment SCORES (all of the Y row within any substring of the X row; larger is nearer, NEGATIVE values
    occur) of the rows of AlnOperand `yo` (rows = (r0, r1): only those) against every row of `xo`, plus `bias` >= 0
    (pg_alignment_fit_dense); arguments and outputs as `alignment_semiglobal_dense`.  Exact while
    `aln_fit_fits(xo.l, yo.l, max(S), gap, gap_open)` holds, and in fp16 while every score + bias lies in 0..2048; the
    caller checks both."""
    return _aln_dense("pg_alignment_fit_dense", "alignment_fit_dense", xo, yo, score, (gap, gap_open, bias), out_bytes, rows)


def alignment_fit_long_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None, bias=0):
    """`alignment_fit_dense` for operands of up to ALN_LONG_MAX_L positions (pg_alignment_fit_long_dense): int64 (out_bytes
    8) or the int32 block i32_knn / i32_eps select from (4).  Exact while `aln_fit_fits` holds, which the caller checks.
    Allocates the call's workspace."""
    return _aln_dense("pg_alignment_fit_long_dense", "alignment_fit_long_dense", xo, yo, score, (gap, gap_open, bias), out_bytes,
                      rows, long=True)


class ProfileOperand:
    """Profiles staged for pg_alignment_profile_dense / _long_dense: `buf` uint8 (Q, 32, lpad), byte P[j][a] + bias at
    [q][a][j], zeros past a profile's length and for symbols it does not have; `lengths` int32 (Q,) on the device; `l` the
    longest length, `lpad` it rounded up to 128; `bias` = -min(0, min P) and `top` = max(0, max P) over all Q profiles."""
    __slots__ = ("buf", "lengths", "n", "l", "lpad", "bias", "top")

    def __init__(self, buf, lengths, l, bias, top):
        self.buf, self.lengths, self.n, self.l, self.lpad = buf, lengths, int(buf.shape[0]), int(l), int(buf.shape[2])
        self.bias, self.top = int(bias), int(top)


def profile_pack(profiles):
    """A list of (L_q, A) integer arrays (1 <= L_q <= 2048, 2 <= A <= 32, entries -128..127) -> the host arrays of a
    ProfileOperand: (buf uint8 (Q, 32, lpad), lengths int32 (Q,), longest length, bias, top).  Host numpy: it is not hot."""
    lengths = np.array([p.shape[0] for p in profiles], dtype=np.int32)
    l = int(lengths.max())
    if l > ALN_LONG_MAX_L or lengths.min() < 1 or any(p.ndim != 2 or not 2 <= p.shape[1] <= SUB_MAX_A for p in profiles):
        raise ValueError(f"profile_pack: (L, A) profiles of 1..{ALN_LONG_MAX_L} positions and 2..{SUB_MAX_A} symbols")
    lo, hi = min(int(p.min()) for p in profiles), max(int(p.max()) for p in profiles)
    if lo < ALN_LOCAL_MIN or hi > ALN_LOCAL_MAX:
        raise ValueError("profile_pack: entries in -128..127")
    bias, top = -min(0, lo), max(0, hi)
    buf = np.zeros((len(profiles), SUB_MAX_A, ((l + 127) // 128) * 128), dtype=np.uint8)
    for q, p in enumerate(profiles):
        buf[q, :p.shape[1], :p.shape[0]] = (np.asarray(p, dtype=np.int64) + bias).T
    return buf, lengths, l, bias, top


def profile_operand(profiles):
    """`profile_pack` on the current HIP device."""
    buf, lengths, l, bias, top = profile_pack(profiles)
    dev = device()
    return ProfileOperand(torch.from_numpy(buf).to(dev), torch.from_numpy(lengths).to(dev), l, bias, top)


def _profile_dense(entry, name, mode, xo, po, gap, gap_open, out_bytes, rows, bias, long=False):
    """One profile entry: the profiles (r0, r1) of `po` against every row of `xo`, as `_aln_dense`."""
    small = 4 if long else 2
    if out_bytes not in (small, 8):
        raise ValueError(f"{name}: out_bytes 8 (int64) or {small} ({'int32' if long else 'fp16'})")
    r0, r1 = (0, po.n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= r0 < r1 <= po.n:
        raise ValueError("row range outside the operand")
    out = torch.empty((r1 - r0, xo.n), dtype=_TORCH_OUT[out_bytes], device=xo.buf.device)
    tail = ()
    if long:
        ws = aln_long_workspace(xo, r1 - r0)
        tail = (_ptr(ws), ws.numel())
    _check(getattr(lib(), entry)(ALN_PROFILE_MODES.index(mode), _ptr(xo.buf), xo.n, xo.npad, xo.l,
                                 ctypes.c_void_p(po.buf.data_ptr() + r0 * SUB_MAX_A * po.lpad),
                                 ctypes.c_void_p(po.lengths.data_ptr() + 4 * r0), r1 - r0, po.lpad, po.l, po.bias, po.top, int(gap),
                                 int(gap_open), int(bias), _ptr(out), out.stride(0), out_bytes, *tail, _stream()), entry)
    return out


def alignment_profile_dense(mode, xo, po, gap, gap_open, out_bytes=8, rows=None, bias=0):
    """(Q, N) profile alignment SCORES of the profiles of ProfileOperand `po` (rows = (r0, r1): only those) against every row
    of AlnOperand `xo` (pg_alignment_profile_dense; both at most 128 positions); `mode` one of ALN_PROFILE_MODES, `gap`
    1..255, `gap_open` 0..255, `bias` >= 0 the shift of `alignment_fit_dense` (fit alone).  int64 (out_bytes 8) or the fp16
    block f16_knn / f16_eps select from (2: exact while every value lies in 0..2048).  The caller checks the mode's cell
    bound (`aln_local_long_fits`, `aln_semiglobal_long_fits`, `aln_fit_fits` with po.top for max S)."""
    return _profile_dense("pg_alignment_profile_dense", "alignment_profile_dense", mode, xo, po, gap, gap_open, out_bytes, rows, bias)


def alignment_profile_long_dense(mode, xo, po, gap, gap_open, out_bytes=8, rows=None, bias=0):
    """`alignment_profile_dense` up to ALN_LONG_MAX_L positions on either side (pg_alignment_profile_long_dense): int64 (8) or
    the int32 block i32_knn / i32_eps select from (4).  Allocates the call's workspace."""
    return _profile_dense("pg_alignment_profile_long_dense", "alignment_profile_long_dense", mode, xo, po, gap, gap_open, out_bytes,
                          rows, bias, long=True)


def aln_long_operand(tokens, a):
    """(N, L <= 2048) uint8 tokens -> AlnOperand for a table of `a` symbols, for the kernels beyond 128 positions
    (pg_sub_pack at the operand's own width).  No host sync, as `aln_operand`."""
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dim() == 2 and tokens.shape[1] > ALN_LONG_MAX_L:
        raise ValueError(f"aln_long_operand: at most {ALN_LONG_MAX_L} tokens per sequence")
    so = sub_operand(tokens, a)
    return AlnOperand(so.buf, so.n, so.l, so.flags)


def aln_long_workspace(xo, nrows):
    """The boundary-column workspace of one call (pg_alignment_long_workspace): a share per workgroup in flight on the
    whole device, or per (256 columns, 8 rows) tile of the call when those are fewer."""
    one, full = _i64(0), _i64(0)
    _check(lib().pg_alignment_long_workspace(xo.l, ctypes.byref(one), ctypes.byref(full)), "pg_alignment_long_workspace")
    tiles = ((xo.n + 255) // 256) * ((int(nrows) + 7) // 8)
    return torch.empty(min(full.value, tiles * one.value), dtype=torch.uint8, device=xo.buf.device)


def alignment_long_dense(xo, yo, cost, gap, gap_open, out_bytes=8, rows=None):
    """`alignment_affine_dense` for operands of up to ALN_LONG_MAX_L positions (pg_alignment_long_dense; gap_open = 0: the
    linear penalty): int64 (out_bytes 8) or the int32 block i32_knn / i32_eps select from (4).  Exact while
    `aln_long_fits(max(xo.l, yo.l), ...)` holds, which the caller checks.  Allocates the call's workspace."""
    return _aln_dense("pg_alignment_long_dense", "alignment_long_dense", xo, yo, cost, (gap, gap_open), out_bytes, rows, long=True)


def alignment_local_long_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    """`alignment_local_dense` for operands of up to ALN_LONG_MAX_L positions (pg_alignment_local_long_dense), outputs as
    `alignment_long_dense`.  Exact while `aln_local_long_fits(xo.l, yo.l, max(S))` holds, which the caller checks."""
    return _aln_dense("pg_alignment_local_long_dense", "alignment_local_long_dense", xo, yo, score, (gap, gap_open), out_bytes, rows, long=True)


def alignment_semiglobal_long_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    """`alignment_semiglobal_dense` for operands of up to ALN_LONG_MAX_L positions (pg_alignment_semiglobal_long_dense),
    outputs as `alignment_long_dense`.  Exact while `aln_semiglobal_long_fits(xo.l, yo.l, max(S))` holds, which the caller
    checks."""
    return _aln_dense("pg_alignment_semiglobal_long_dense", "alignment_semiglobal_long_dense", xo, yo, score, (gap, gap_open),
                      out_bytes, rows, long=True)


TRACE_ENTRIES = ("pg_alignment_trace", "pg_alignment_fit_trace")                    # the moded entry and its fit entry
TRACE_LONG_ENTRIES = ("pg_alignment_trace_long", "pg_alignment_fit_trace_long")


def _wave_bytes(entry, xl, yl):
    """One wave's share of a traceback's workspace, from the workspace entry `entry`."""
    one = _i64(0)
    _check(getattr(lib(), entry)(int(xl), int(yl), ctypes.byref(one)), entry)
    return one.value


def aln_trace_wave_bytes(xl, yl):
    """The direction bits of the 64 pairs of one wave of pg_alignment_trace (pg_alignment_trace_workspace)."""
    return _wave_bytes("pg_alignment_trace_workspace", xl, yl)


def _trace_launch(xo, yo, xi, yi, p0, p1, mode, table, gap, gap_open, head, ops, ws, entries=TRACE_ENTRIES):
    """One call of `entries` (the moded entry and its fit entry): pairs p0..p1-1 of the lists into rows p0..p1-1 of head and
    ops.  ALN_TRACE_FIT goes to the fit entry, an entry of its own without `mode`."""
    ldo = ops.stride(0)
    fit = int(mode) == ALN_TRACE_FIT
    entry = entries[fit]
    _check(getattr(lib(), entry)(*(() if fit else (int(mode),)), _ptr(xo.buf), xo.n, xo.npad, xo.l, _ptr(yo.buf), yo.n, yo.npad,
                                 yo.l, ctypes.c_void_p(xi.data_ptr() + 4 * p0), ctypes.c_void_p(yi.data_ptr() + 4 * p0), p1 - p0,
                                 _ptr(table), int(gap), int(gap_open), ctypes.c_void_p(head.data_ptr() + 32 * p0),
                                 ctypes.c_void_p(ops.data_ptr() + ldo * p0), ldo, _ptr(ws), ws.numel(), _stream()), entry)


def _trace_long_launch(*args):
    """`_trace_launch` on pg_alignment_trace_long and its fit entry; a name of its own, which the test stand-ins replace."""
    _trace_launch(*args, entries=TRACE_LONG_ENTRIES)


def _pair_lists(name, xo, yo, xi, yi):
    """The pair lists of `alignment_trace`, `alignment_trace_long` and `alignment_stats` as int32 device tensors, their
    index ranges checked on the host: ONE SYNC, IndexError for a row number outside its operand."""
    dev = xo.buf.device
    xi = torch.as_tensor(xi).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    yi = torch.as_tensor(yi).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if xi.numel() != yi.numel() or xi.numel() == 0:
        raise ValueError(f"{name}: xi and yi must be two non-empty lists of one length")
    lo_hi = torch.stack([xi.min(), xi.max(), yi.min(), yi.max()]).tolist()                # the one host sync
    if lo_hi[0] < 0 or lo_hi[1] >= xo.n or lo_hi[2] < 0 or lo_hi[3] >= yo.n:
        raise IndexError(f"{name}: a pair's row number is outside its operand")
    return xi, yi


def _trace_list(name, wave_bytes, launch, xo, yo, xi, yi, mode, table, gap, gap_open, workspace_bytes):
    """`alignment_trace` / `alignment_trace_long`: the index check, the workspace, the split into launches."""
    dev = xo.buf.device
    xi, yi = _pair_lists(name, xo, yo, xi, yi)
    one = wave_bytes(xo.l, yo.l)
    p, ldo = xi.numel(), xo.l + yo.l
    if workspace_bytes is None:                                             # what the list needs; a share is 129 MiB at most
        workspace_bytes = min(((p + 63) // 64) * one, ALN_TRACE_LONG_WORKSPACE)
    if int(workspace_bytes) < one:
        raise ValueError(f"{name}: workspace_bytes must hold one wave's share ({one} bytes)")
    waves = min(int(workspace_bytes) // one, (p + 63) // 64)
    ws = torch.empty(waves * one, dtype=torch.uint8, device=dev)
    head = torch.empty((p, 8), dtype=torch.int32, device=dev)
    ops = torch.empty((p, ldo), dtype=torch.uint8, device=dev)
    for p0 in range(0, p, waves * 64):
        launch(xo, yo, xi, yi, p0, min(p, p0 + waves * 64), mode, table, gap, gap_open, head, ops, ws)
    return head, ops


def alignment_trace(xo, yo, xi, yi, mode, table, gap, gap_open, workspace_bytes=256 << 20):
    """The canonical alignments (pg_alignment_trace) of the pairs (row xi[p] of AlnOperand `xo`, row yi[p]
    of `yo`), P >= 1 of them, repeats allowed: `mode` ALN_TRACE_GLOBAL (`table` from sub_cost), ALN_TRACE_LOCAL,
    ALN_TRACE_SEMIGLOBAL or ALN_TRACE_FIT (`table` from aln_local_score; FIT runs pg_alignment_fit_trace: y whole within x); `gap` 1..255, `gap_open` 0..255.  Returns (head int32 (P, 8): score,
    x_begin, x_end, y_begin, y_end, n_ops, identities, status; ops uint8 (P, xo.l + yo.l): 1 pair, 2 x unaligned, 3 y
    unaligned, 0 from n_ops on) on the device.  The index ranges are checked on the host - ONE SYNC - and an index outside
    its operand raises IndexError.  The list is split into launches whose waves all fit `workspace_bytes` of direction
    bits (at least one wave's share, ValueError below it); the workspace is allocated here, once."""
    return _trace_list("alignment_trace", aln_trace_wave_bytes, _trace_launch, xo, yo, xi, yi, mode, table, gap,
                       gap_open, workspace_bytes)


def aln_trace_long_ready():
    """Can `alignment_trace_long` run?  True only with a HIP device.  The routes of alignments.py and `Prograph.align` ask
    this, not `aln_long_ready`, before they leave `host_trace` for operands beyond 128 positions."""
    try:
        return device().type == "cuda"
    except NativeUnavailable:
        return False


def aln_trace_long_wave_bytes(xl, yl):
    """One wave's share of pg_alignment_trace_long's workspace (pg_alignment_trace_long_workspace): the direction bits of
    its 64 pairs and their boundary column between strips."""
    return _wave_bytes("pg_alignment_trace_long_workspace", xl, yl)


def alignment_trace_long(xo, yo, xi, yi, mode, table, gap, gap_open, workspace_bytes=None):
    """`alignment_trace` for operands of up to ALN_LONG_MAX_L positions (pg_alignment_trace_long; `xo`,
    `yo` from aln_long_operand): the same lists, index check (ONE SYNC), errors and (head, ops).  Cells are int32: every
    table and penalty is exact, there is no "fits" condition.  `workspace_bytes` None: what the list needs, at most
    ALN_TRACE_LONG_WORKSPACE (2 GiB: about 400 waves in flight at 400 positions) and at least one wave's share."""
    return _trace_list("alignment_trace_long", aln_trace_long_wave_bytes, _trace_long_launch, xo, yo, xi, yi,
                       mode, table, gap, gap_open, workspace_bytes)


ALN_STATS_OPS_BYTES = 256 << 20     # alignment_trace_long_heads: the most `ops` alive at a time


def alignment_trace_long_heads(xo, yo, xi, yi, mode, table, gap, gap_open, ops_bytes=ALN_STATS_OPS_BYTES):
    """The heads of `alignment_trace_long` without its `ops`, for lists whose ops would not fit: the pair list runs through
    pg_alignment_trace_long in slices of `ops_bytes // (xo.l + yo.l)` pairs (at least one) that share ONE ops buffer of at
    most `ops_bytes` and one workspace (a slice's need, at most ALN_TRACE_LONG_WORKSPACE), and only head (P, 8) is kept.
    The same index check (ONE SYNC) and errors.  DESIGN.md §4.25: the route of `ops=False` beyond 128 positions."""
    xi, yi = _pair_lists("alignment_trace_long_heads", xo, yo, xi, yi)
    dev = xo.buf.device
    one = aln_trace_long_wave_bytes(xo.l, yo.l)
    p, ldo = xi.numel(), xo.l + yo.l
    per = min(p, max(1, int(ops_bytes) // ldo))
    waves = max(1, min(ALN_TRACE_LONG_WORKSPACE // one, (per + 63) // 64))
    ws = torch.empty(waves * one, dtype=torch.uint8, device=dev)
    head = torch.empty((p, 8), dtype=torch.int32, device=dev)
    ops = torch.empty((per, ldo), dtype=torch.uint8, device=dev)
    for s0 in range(0, p, per):
        s1 = min(p, s0 + per)
        for p0 in range(0, s1 - s0, waves * 64):
            _trace_long_launch(xo, yo, xi[s0:s1], yi[s0:s1], p0, min(s1 - s0, p0 + waves * 64), mode, table, gap, gap_open,
                               head[s0:s1], ops[:s1 - s0], ws)
    return head


def _stats_launch(xo, yo, xi, yi, mode, table, gap, gap_open, head):
    """One pg_alignment_stats call: every pair of the lists into the rows of head."""
    _check(lib().pg_alignment_stats(int(mode), _ptr(xo.buf), xo.n, xo.npad, xo.l, _ptr(yo.buf), yo.n, yo.npad, yo.l, _ptr(xi),
                                    _ptr(yi), xi.numel(), _ptr(table), int(gap), int(gap_open), _ptr(head), _stream()),
           "pg_alignment_stats")


def alignment_stats(xo, yo, xi, yi, mode, table, gap, gap_open):
    """The head of `alignment_trace` without the alignments' columns (pg_alignment_stats): int32 (P, 8) =
    score, x_begin, x_end, y_begin, y_end, n_ops, identities, status of the canonical alignment of every pair, field for
    field what `alignment_trace` returns, from a forward pass that carries the path's counts - no ops, no workspace, one
    launch.  `mode` ALN_TRACE_GLOBAL (`table` from sub_cost), ALN_TRACE_LOCAL, ALN_TRACE_SEMIGLOBAL or ALN_TRACE_FIT (`table`
    from aln_local_score); operands from aln_operand (at most 128 positions); `gap` 1..255, `gap_open` 0..255.  The index
    check is `alignment_trace`'s: ONE SYNC, IndexError for a row number outside its operand."""
    xi, yi = _pair_lists("alignment_stats", xo, yo, xi, yi)
    head = torch.empty((xi.numel(), 8), dtype=torch.int32, device=xo.buf.device)
    _stats_launch(xo, yo, xi, yi, mode, table, gap, gap_open, head)
    return head


def aln_list_ready():
    """Can `alignment_list_scores` run?  True only with a HIP device.  `Prograph.rescore` asks this before it leaves the
    scores of `align(..., ops=False)` for the list kernel."""
    try:
        return device().type == "cuda"
    except NativeUnavailable:
        return False


INT32_MIN = -(1 << 31)              # alignment_list_scores: the value of an entry that names no column


def alignment_list_scores(xo, yo, indptr, indices, mode, table, gap, gap_open):
    """The alignment value of every edge of a CSR list (pg_alignment_list_scores): int32 [nnz] on the
    device, entry e of row r = the value of Y row r against X column indices[e] - what `alignment_affine_dense`,
    `alignment_local_dense`, `alignment_semiglobal_dense` or `alignment_fit_dense` (bias 0) holds at [r, indices[e]].
    `indptr` int64 [yo.n + 1] from 0, non-decreasing, `indices` int32 (cast and moved to the device when they are not);
    `mode` ALN_TRACE_GLOBAL (`table` from sub_cost), ALN_TRACE_LOCAL, ALN_TRACE_SEMIGLOBAL or ALN_TRACE_FIT (`table` from
    aln_local_score; exact while `aln_fit_fits` holds, which the caller checks); operands from aln_operand; `gap` 1..255,
    `gap_open` 0..255.  An entry outside 0..xo.n-1 (the -1 of an unfilled kNN slot) gets INT32_MIN.  No host sync, no
    workspace: `indptr` is the caller's word for the length of `indices`."""
    dev = xo.buf.device
    indptr = torch.as_tensor(indptr).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    indices = torch.as_tensor(indices).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if indptr.numel() != yo.n + 1:
        raise ValueError("alignment_list_scores: indptr must have one entry per row of yo, and one more")
    scores = torch.empty(indices.numel(), dtype=torch.int32, device=dev)
    if indices.numel():
        _check(lib().pg_alignment_list_scores(int(mode), _ptr(xo.buf), xo.n, xo.npad, xo.l, _ptr(yo.buf), yo.n, yo.npad, yo.l,
                                              _ptr(indptr), _ptr(indices), _ptr(table), int(gap), int(gap_open), _ptr(scores),
                                              _stream()), "pg_alignment_list_scores")
    return scores


def aln_list_long_ready():
    """Can `alignment_list_long_scores` run?  True only with a HIP device.  `Prograph.rescore` asks this, not `aln_list_ready`
    or `aln_long_ready`, before it leaves the scores of `align(..., ops=False)` for the long list kernel at 129..2048
    positions."""
    try:
        return device().type == "cuda"
    except NativeUnavailable:
        return False


def alignment_list_long_scores(xo, yo, indptr, indices, mode, table, gap, gap_open, workspace_bytes=None):
    """`alignment_list_scores` for operands of up to ALN_LONG_MAX_L positions (pg_alignment_list_long_scores, DESIGN.md
    §4.29; `xo`, `yo` from aln_long_operand): int32 [nnz], entry e of row r = what `alignment_long_dense`,
    `alignment_local_long_dense`, `alignment_semiglobal_long_dense` or `alignment_fit_long_dense` (bias 0) holds at
    [r, indices[e]], INT32_MIN for an entry outside 0..xo.n-1.  Exact while the mode's 16-bit bound holds (`aln_long_fits`,
    `aln_local_long_fits`, `aln_semiglobal_long_fits`, `aln_fit_fits`), which the caller checks.  The boundary-column
    workspace - min(the whole device's, a share per row) bytes, or `workspace_bytes` of it, at least one share - is
    allocated here, once per call.  No host sync."""
    dev = xo.buf.device
    indptr = torch.as_tensor(indptr).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    indices = torch.as_tensor(indices).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if indptr.numel() != yo.n + 1:
        raise ValueError("alignment_list_long_scores: indptr must have one entry per row of yo, and one more")
    scores = torch.empty(indices.numel(), dtype=torch.int32, device=dev)
    if indices.numel():
        one, full = _i64(0), _i64(0)
        _check(lib().pg_alignment_long_workspace(xo.l, ctypes.byref(one), ctypes.byref(full)), "pg_alignment_long_workspace")
        nbytes = min(full.value, yo.n * one.value) if workspace_bytes is None else int(workspace_bytes)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _check(lib().pg_alignment_list_long_scores(int(mode), _ptr(xo.buf), xo.n, xo.npad, xo.l, _ptr(yo.buf), yo.n, yo.npad, yo.l,
                                                   _ptr(indptr), _ptr(indices), _ptr(table), int(gap), int(gap_open), _ptr(scores),
                                                   _ptr(ws), ws.numel(), _stream()), "pg_alignment_list_long_scores")
    return scores


def spectrum_profile(tokens, k, symbols, dims=None, rows=None):
    """The k-mer count profiles of a (N, L <= 2048) uint8 token matrix (pg_spectrum_profile): tokens
    1..symbols, 0 padding or unknown anywhere; `dims` None / 0 for the exact width symbols^k, else the hashed width.
    `rows`: row numbers of `tokens` to profile, in that order (host values are checked here; a device tensor costs one
    sync for the same check).  Returns ((len(rows) or N, D) fp16 device tensor, int32[1] flag tensor - non-zero when a
    token above `symbols` was read); no host sync: read the flag before trusting the profiles."""
    L = lib()
    dev = device()
    if not isinstance(tokens, torch.Tensor):
        tokens = torch.from_numpy(np.ascontiguousarray(np.asarray(tokens)))
    if tokens.dtype != torch.uint8 or tokens.dim() != 2 or tokens.shape[0] == 0 or tokens.shape[1] == 0:
        raise TypeError("spectrum_profile expects a non-empty 2-D uint8 token matrix")
    if tokens.shape[1] > SPECTRUM_MAX_L:
        raise ValueError(f"spectrum_profile: at most {SPECTRUM_MAX_L} tokens per sequence")
    D = int(L.pg_spectrum_dims(int(k), int(symbols), int(dims or 0)))
    if D < 0:
        raise ValueError(L.pg_last_error().decode("utf-8", "replace"))
    tokens = tokens.to(dev)
    if tokens.stride(1) != 1 or tokens.stride(0) < tokens.shape[1]:
        tokens = tokens.contiguous()
    n = tokens.shape[0]
    if rows is not None:
        rows = torch.as_tensor(rows).reshape(-1).to(torch.int64)
        if rows.numel() == 0:
            raise ValueError("spectrum_profile: an empty row list")
        if bool(((rows < 0) | (rows >= n)).any()):
            raise ValueError("spectrum_profile: a row number outside the token matrix")
        rows = rows.to(dev).contiguous()
        n = rows.numel()
    out = torch.empty((n, D), dtype=torch.float16, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)        # (pg_spectrum_profile zeroes it on the stream)
    _check(L.pg_spectrum_profile(_ptr(tokens), n, tokens.shape[1], tokens.stride(0), _ptr(rows), int(k), int(symbols), int(dims or 0),
                                 _ptr(out), out.stride(0), _ptr(flags), _stream()), "pg_spectrum_profile")
    return out, flags


def i32_knn_round(block, k, floor_idx, floor_w, idx_out, w_out, descending=False):
    """One round of pg_i32_knn_round: the next k <= 64 ranks of every row of an int32 block after its floor (views as for
    f16_knn_round)."""
    m, n = block.shape
    _check(lib().pg_i32_knn_round(_ptr(block), m, n, block.stride(0), int(k), 1 if descending else 0, _ptr(floor_idx),
                                  _ptr(floor_w), floor_idx.stride(0), _ptr(idx_out), _ptr(w_out), idx_out.stride(0),
                                  _stream()), "pg_i32_knn_round")


def i32_knn(block, k, first=1, descending=False):
    """Ranks first..first+k-1 of every row of a block of non-negative int32 values in the stable (value, column) order
    (descending: largest first) -> (idx int32, w int32).  first + k > 64 (k <= MAX_K_ROUNDS): in rounds of 64 ranks over
    the same block (knn_rounds)."""
    if first + k > 64:
        return knn_rounds(block.shape[0], int(k), int(first), torch.int32, block.device,
                          lambda kk: i32_knn(block, kk, first, descending),
                          lambda kk, fi, fw, oi, ow: i32_knn_round(block, kk, fi, fw, oi, ow, descending))
    m, n = block.shape
    idx = torch.empty((m, k), dtype=torch.int32, device=block.device)
    w = torch.empty((m, k), dtype=torch.int32, device=block.device)
    _check(lib().pg_i32_knn(_ptr(block), m, n, block.stride(0), int(k), int(first), 1 if descending else 0, _ptr(idx), _ptr(w),
                            _stream()), "pg_i32_knn")
    return idx, w


def i32_eps(block, cmp, thr, keep_zero=False):
    """CSR of the entries of an int32 block with comp(v, thr) & (v > 0), thr an integer; keep_zero: v = 0 is a hit too
    (rows of queries).  Returns (indptr int64 [m+1], indices int32 ascending within a row, weights int32)."""
    L = lib()
    m, n = block.shape
    thr = min(max(int(thr), -1), 1 << 31)                                     # the same test on every value in 0..2^31-1
    cmp = int(cmp) | (CMP_KEEP_ZERO if keep_zero else 0)
    counts = torch.empty(m, dtype=torch.int32, device=block.device)
    _check(L.pg_i32_eps_count(_ptr(block), m, n, block.stride(0), cmp, thr, _ptr(counts), _stream()), "pg_i32_eps_count")
    indptr, indices, weights = _csr_alloc(counts, torch.int32)
    if indices.numel():
        _check(L.pg_i32_eps_fill(_ptr(block), m, n, block.stride(0), cmp, thr, _ptr(indptr), _ptr(indices), _ptr(weights),
                                 _stream()), "pg_i32_eps_fill")
    return indptr, indices, weights


def csr_row_stats(indptr, indices, weights, f=None, want=("deg",), row0=0, ncols=None):
    """Per-row reductions over a device CSR (see pg_csr_row_stats).  `weights`: uint8 or float32
    device tensor or None (boolean).  `want` from deg / sum_f / sum_wf / self_w (per row) and col_sum
    (per column, needs `ncols`).  Returns a dict of float64 device tensors."""
    nrows = indptr.numel() - 1
    dev = indptr.device
    out = {k: torch.empty(nrows, dtype=torch.float64, device=dev) for k in want if k != "col_sum"}
    if "col_sum" in want:
        out["col_sum"] = torch.zeros(int(ncols), dtype=torch.float64, device=dev)
    w8 = weights if (weights is not None and weights.dtype == torch.uint8) else None
    wf = weights if (weights is not None and weights.dtype == torch.float32) else None
    if weights is not None and w8 is None and wf is None:
        raise TypeError("weights must be uint8 or float32")
    fd = None if f is None else f.to(device=dev, dtype=torch.float64).contiguous()
    _check(lib().pg_csr_row_stats(_ptr(indptr), _ptr(indices), _ptr(w8), _ptr(wf), nrows, int(row0), _ptr(fd),
                                  _ptr(out.get("deg")), _ptr(out.get("sum_f")), _ptr(out.get("sum_wf")),
                                  _ptr(out.get("self_w")), _ptr(out.get("col_sum")), _stream()), "pg_csr_row_stats")
    return out


# ----------------------------------------------------------------------------------------------
# Undirected graphs from a device CSR (pg_graph.hip; definitions in include/prograph_hip.h and DESIGN.md §4.30)
# ----------------------------------------------------------------------------------------------
W_KINDS = {torch.uint8: (1, 0), torch.int16: (2, 1), torch.int32: (4, 1), torch.float16: (2, 2), torch.float32: (4, 2)}
SYM_MODES, SYM_COMBINES = {"union": 0, "mutual": 1}, {"min": 0, "max": 1}


def _w_kind(weights):
    """(elem_bytes, kind) of the weight dtypes the graph containers carry."""
    if weights.dtype not in W_KINDS:
        raise TypeError(f"weights must be one of {sorted(str(d) for d in W_KINDS)}, not {weights.dtype}")
    return W_KINDS[weights.dtype]


def _csr_operands(indptr, indices, weights):
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or weights.numel() != indices.numel() or indptr.numel() < 1:
        raise TypeError("a CSR is indptr int64 [n + 1], indices int32 [nnz], weights [nnz]")
    if not (indptr.is_cuda and indices.is_cuda and weights.is_cuda):
        raise NativeUnavailable("the graph operations run on device tensors; there is no CPU path")
    return indptr.contiguous(), indices.contiguous(), weights.contiguous()


def _bytes(n, dev):
    return torch.empty(max(int(n), 8), dtype=torch.uint8, device=dev)


def _scan(counts):
    """uint32 counts (an int32 tensor) -> indptr int64 [m + 1] on the device; m = 0: [0]."""
    m, dev = counts.numel(), counts.device
    indptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    if m:
        scratch = _bytes(lib().pg_scan_scratch_bytes(m), dev)
        _check(lib().pg_exclusive_scan(_ptr(counts), m, _ptr(indptr), _ptr(scratch), _stream()), "pg_exclusive_scan")
    return indptr


def _csr_out(indptr, nnz_max, like, trim):
    """The arrays of a result of at most nnz_max entries; trim: ONE host read of its nnz, else the arrays keep nnz_max entries
    of which the first indptr[-1] are the result (a stage of `csr_symmetrize`, which reads once at its end)."""
    nnz = int(indptr[-1].item()) if trim else int(nnz_max)
    dev = indptr.device
    return torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz], torch.empty(max(nnz, 1), dtype=like.dtype, device=dev)[:nnz]


def csr_sort_rows(indptr, indices, weights, ncols, trim=True):
    """sorted(): every row's edges ascending by column, equal columns in storage order, entries whose column is outside
    0..ncols-1 dropped.  Device tensors in, (indptr, indices, weights) out."""
    indptr, indices, weights = _csr_operands(indptr, indices, weights)
    eb, _ = _w_kind(weights)
    L, dev = lib(), indptr.device
    nrows, nnz = indptr.numel() - 1, indices.numel()
    if not nnz:
        return torch.zeros(nrows + 1, dtype=torch.int64, device=dev), indices, weights
    counts = torch.zeros(nrows, dtype=torch.int32, device=dev)
    nbytes = int(L.pg_csr_sort_workspace(nnz))
    ws = _bytes(nbytes, dev)
    _check(L.pg_csr_sort_rows_count(_ptr(indptr), _ptr(indices), nrows, nnz, int(ncols), _ptr(counts), _ptr(ws), nbytes, _stream()),
           "pg_csr_sort_rows_count")
    out_indptr = _scan(counts)
    out_idx, out_w = _csr_out(out_indptr, nnz, weights, trim)
    _check(L.pg_csr_sort_rows_fill(_ptr(indptr), _ptr(weights), eb, nrows, nnz, _ptr(counts), _ptr(out_indptr), _ptr(out_idx),
                                   _ptr(out_w), _ptr(ws), nbytes, _stream()), "pg_csr_sort_rows_fill")
    return out_indptr, out_idx, out_w


def csr_transpose(indptr, indices, weights, ncols, row0=0, trim=True):
    """transpose(): (indptr [ncols + 1], indices, weights) of T, whose row c lists (row0 + r, w) for every edge (r, c, w) in
    storage order; the same bits every run."""
    indptr, indices, weights = _csr_operands(indptr, indices, weights)
    eb, _ = _w_kind(weights)
    L, dev = lib(), indptr.device
    nrows, nnz, ncols = indptr.numel() - 1, indices.numel(), int(ncols)
    if not nnz or not ncols:
        return torch.zeros(ncols + 1, dtype=torch.int64, device=dev), indices[:0], weights[:0]
    counts = torch.zeros(ncols, dtype=torch.int32, device=dev)
    _check(L.pg_csr_histogram(_ptr(indices), nnz, ncols, _ptr(counts), _stream()), "pg_csr_histogram")
    t_indptr = _scan(counts)
    t_idx, t_w = _csr_out(t_indptr, nnz, weights, trim)
    nbytes = int(L.pg_csr_transpose_workspace(nnz, ncols))
    ws = _bytes(nbytes, dev)
    _check(L.pg_csr_transpose(_ptr(indptr), _ptr(indices), _ptr(weights), eb, nrows, nnz, ncols, int(row0), _ptr(t_indptr),
                              _ptr(t_idx), _ptr(t_w), _ptr(ws), nbytes, _stream()), "pg_csr_transpose")
    return t_indptr, t_idx, t_w


def csr_symmetrize(indptr, indices, weights, mode="union", combine="min"):
    """symmetrize() of a square graph over n = nrows = ncols nodes (row0 = 0): rows ascending by column, each column once;
    union | mutual, the weight min | max over every occurrence of (r, c) and (c, r).  One host read, of the result's nnz."""
    if mode not in SYM_MODES or combine not in SYM_COMBINES:
        raise ValueError("mode is 'union' or 'mutual', combine is 'min' or 'max'")
    indptr, indices, weights = _csr_operands(indptr, indices, weights)
    eb, kind = _w_kind(weights)
    L, dev = lib(), indptr.device
    n, nnz = indptr.numel() - 1, indices.numel()
    if not nnz:
        return torch.zeros(n + 1, dtype=torch.int64, device=dev), indices, weights
    a = csr_sort_rows(indptr, indices, weights, n, trim=False)
    t = csr_transpose(indptr, indices, weights, n, trim=False)
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    nbytes = int(L.pg_csr_symmetrize_workspace(nnz, nnz))
    ws = _bytes(nbytes, dev)
    _check(L.pg_csr_symmetrize_count(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), nnz, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), nnz, eb, kind,
                                     SYM_MODES[mode], SYM_COMBINES[combine], n, _ptr(counts), _ptr(ws), nbytes, _stream()),
           "pg_csr_symmetrize_count")
    out_indptr = _scan(counts)
    out_idx, out_w = _csr_out(out_indptr, 0, weights, True)
    _check(L.pg_csr_symmetrize_fill(_ptr(a[0]), nnz, _ptr(t[0]), nnz, eb, n, _ptr(out_indptr), _ptr(out_idx), _ptr(out_w), _ptr(ws),
                                    nbytes, _stream()), "pg_csr_symmetrize_fill")
    return out_indptr, out_idx, out_w


class PackedF16:
    """Device-resident fp16 vectors in chunk-major order (pg_pack_f16)."""
    __slots__ = ("buf", "n", "d", "npad")

    def __init__(self, buf, n, d):
        self.buf, self.n, self.d, self.npad = buf, int(n), int(d), npad(n)


def pack_f16(x):
    """(N, D) fp16 device tensor -> PackedF16."""
    if x.dtype != torch.float16 or x.dim() != 2 or not x.is_cuda or x.shape[0] == 0 or x.shape[1] == 0:
        raise TypeError("pack_f16 expects a non-empty 2-D fp16 device tensor")
    x = x.contiguous()
    n, d = x.shape
    np_ = npad(n)
    buf = torch.empty(((d + 7) // 8) * np_ * 16, dtype=torch.uint8, device=x.device)
    _check(lib().pg_pack_f16(_ptr(x), n, d, x.stride(0), None, _ptr(buf), np_, _stream()), "pg_pack_f16")
    return PackedF16(buf, n, d)


def minkowski_dense(xp, yp, similarity=False):
    """(M, N) fp16 block: Minkowski p=2 distance (or 1/(1+d)) of every Y vector against every X vector,
    rounded step by step like the reference's fp16 tensor expression (minkowski.py:36-40)."""
    if xp.d != yp.d:
        raise ValueError("operands must have the same dimension")
    out = torch.empty((yp.n, xp.n), dtype=torch.float16, device=xp.buf.device)
    _check(lib().pg_minkowski_dense(_ptr(xp.buf), xp.n, xp.npad, _ptr(yp.buf), yp.n, yp.npad, xp.d, 1 if similarity else 0,
                                    _ptr(out), out.stride(0), _stream()), "pg_minkowski_dense")
    return out


def knn_rounds(m, k, first, wdtype, dev, head, step):
    """Ranks first..first+k-1 (first + k > 64, k <= MAX_K_ROUNDS) of the pg_*_knn_round scheme -> (idx int32 (m, k),
    w (m, k) of wdtype).  head(kk) is the floor-free call for ranks first..63 (kk = 64 - first); then
    step(kk, floor_idx, floor_w, idx_out, w_out) writes the next kk <= 64 ranks after each row's floor - the
    previous round's last column - straight into the column slice idx_out / w_out of the result."""
    if not 64 - first < k <= MAX_K_ROUNDS:
        raise ValueError(f"the rounds produce {65 - first}..{MAX_K_ROUNDS} ranks per row, not {k}")
    idx = torch.empty((m, k), dtype=torch.int32, device=dev)
    w = torch.empty((m, k), dtype=wdtype, device=dev)
    done = 64 - first
    idx[:, :done], w[:, :done] = head(done)
    while done < k:
        kk = min(64, k - done)
        step(kk, idx[:, done - 1], w[:, done - 1], idx[:, done:done + kk], w[:, done:done + kk])
        done += kk
    return idx, w


def f16_knn_round(block, k, floor_idx, floor_w, idx_out, w_out, descending=False):
    """One round of pg_f16_knn_round: the next k <= 64 ranks of every row of an fp16 block after its floor
    (floor_idx / floor_w: (m,) views of the previous round's last column) into the (m, k) views idx_out / w_out."""
    m, n = block.shape
    _check(lib().pg_f16_knn_round(_ptr(block), m, n, block.stride(0), int(k), 1 if descending else 0, _ptr(floor_idx),
                                  _ptr(floor_w), floor_idx.stride(0), _ptr(idx_out), _ptr(w_out), idx_out.stride(0),
                                  _stream()), "pg_f16_knn_round")


def f16_knn(block, k, first=1, descending=False):
    """Ranks first..first+k-1 of every row of an fp16 block in (value, column) order -> (idx int32, w fp16).
    first + k > 64 (k <= MAX_K_ROUNDS): in rounds of 64 ranks over the same block (knn_rounds)."""
    if first + k > 64:
        return knn_rounds(block.shape[0], int(k), int(first), torch.float16, block.device,
                          lambda kk: f16_knn(block, kk, first, descending),
                          lambda kk, fi, fw, oi, ow: f16_knn_round(block, kk, fi, fw, oi, ow, descending))
    m, n = block.shape
    idx = torch.empty((m, k), dtype=torch.int32, device=block.device)
    w = torch.empty((m, k), dtype=torch.float16, device=block.device)
    _check(lib().pg_f16_knn(_ptr(block), m, n, block.stride(0), int(k), int(first), 1 if descending else 0, _ptr(idx), _ptr(w),
                            _stream()), "pg_f16_knn")
    return idx, w


def f16_eps(block, cmp, eps, similarity=False, keep_zero=False):
    """CSR of the entries of an fp16 block that satisfy comp(d, eps) & (d > 0)  [comp(eps, s) & (s < 1)].
    `eps` is rounded to fp16 first, as torch does when an fp16 tensor meets a Python number.
    keep_zero: without the second test (rows of queries: d = 0 is a hit)."""
    L = lib()
    m, n = block.shape
    dev = block.device
    e16 = float(np.float16(eps))
    cmp = int(cmp) | (CMP_KEEP_ZERO if keep_zero else 0)
    counts = torch.empty(m, dtype=torch.int32, device=dev)
    _check(L.pg_f16_eps_count(_ptr(block), m, n, block.stride(0), int(cmp), e16, 1 if similarity else 0, _ptr(counts), _stream()),
           "pg_f16_eps_count")
    indptr, indices, weights = _csr_alloc(counts, torch.float16)
    if indices.numel():
        _check(L.pg_f16_eps_fill(_ptr(block), m, n, block.stride(0), int(cmp), e16, 1 if similarity else 0, _ptr(indptr),
                                 _ptr(indices), _ptr(weights), _stream()), "pg_f16_eps_fill")
    return indptr, indices, weights


def _f16_rows(yp, r0, r1):
    """Pointer to vector r0 of a PackedF16 with its npad: chunk q of vector r0 + i sits at (q*npad + r0 + i)*16, so rows
    [r0, r1) are an operand of their own without a copy."""
    return ctypes.c_void_p(yp.buf.data_ptr() + 16 * r0), r1 - r0


def minkowski_knn_round(xp, yp, k, floor_idx, floor_w, idx_out, w_out, similarity=False):
    """One round of pg_minkowski_knn_round: the next k <= 64 ranks of every Y row after its floor, one fused sweep
    (views as for f16_knn_round)."""
    _check(lib().pg_minkowski_knn_round(_ptr(xp.buf), xp.n, xp.npad, _ptr(yp.buf), yp.n, yp.npad, xp.d, 1 if similarity else 0,
                                        int(k), _ptr(floor_idx), _ptr(floor_w), floor_idx.stride(0), _ptr(idx_out), _ptr(w_out),
                                        idx_out.stride(0), _stream()), "pg_minkowski_knn_round")


def minkowski_knn(xp, yp, k, first=1, similarity=False):
    """f16_knn(minkowski_dense(xp, yp, similarity), k, first, descending=similarity) in one fused sweep (pg_minkowski_knn):
    the distances are selected in LDS and never written out.  Returns (idx int32 (m, k), w fp16 (m, k)).
    first + k > 64 (k <= MAX_K_ROUNDS): one more sweep per 64 ranks (knn_rounds)."""
    if xp.d != yp.d:
        raise ValueError("operands must have the same dimension")
    if first + k > 64:
        return knn_rounds(yp.n, int(k), int(first), torch.float16, xp.buf.device,
                          lambda kk: minkowski_knn(xp, yp, kk, first, similarity),
                          lambda kk, fi, fw, oi, ow: minkowski_knn_round(xp, yp, kk, fi, fw, oi, ow, similarity))
    dev = xp.buf.device
    idx = torch.empty((yp.n, int(k)), dtype=torch.int32, device=dev)
    w = torch.empty((yp.n, int(k)), dtype=torch.float16, device=dev)
    _check(lib().pg_minkowski_knn(_ptr(xp.buf), xp.n, xp.npad, _ptr(yp.buf), yp.n, yp.npad, xp.d, 1 if similarity else 0,
                                  int(k), int(first), _ptr(idx), _ptr(w), _stream()), "pg_minkowski_knn")
    return idx, w


def _slots_eps(m_all, rows, slots, compact, fill_rows, wdtype, cap, rows_per_block, dev):
    """The slots -> CSR host loop of minkowski_eps / cosine_eps over blocks of rows_per_block Y rows (None: blocks that
    keep the slots within 256 MB).  Per block: ops = rows(r0, r1) stages the block's operands; slots(ops, slot_idx,
    slot_w, counts) is the one distance sweep (exact counts, up to `cap` entries per row); scan and the block's ONE
    host sync (nnz and the number of rows beyond `cap`); compact(<the C entry's arguments>) moves the rows within `cap`
    into the CSR and fill_rows(ops, row list, its length, indptr, indices, weights) sweeps the others once more,
    straight into it.  ops[-1] is the block's row count."""
    if rows_per_block is None:
        rows_per_block = max(64, (256 << 20) // (cap * (4 + torch.finfo(wdtype).bits // 8)))     # int32 + weight per slot
    parts = []
    for r0 in range(0, m_all, rows_per_block):
        ops = rows(r0, min(m_all, r0 + rows_per_block))
        m = ops[-1]
        counts = torch.empty(m, dtype=torch.int32, device=dev)
        slot_idx = torch.empty(m * cap, dtype=torch.int32, device=dev)
        slot_w = torch.empty(m * cap, dtype=wdtype, device=dev)
        slots(ops, slot_idx, slot_w, counts)
        over = counts > cap
        indptr, indices, weights, n_over = _csr_alloc(counts, wdtype, extra=over.sum())     # the one sync
        if indices.numel():
            compact(m, cap, _ptr(slot_idx), _ptr(slot_w), _ptr(counts), _ptr(indptr), _ptr(indices), _ptr(weights), _stream())
        if n_over:
            fill_rows(ops, compact_flags(over.to(torch.uint8), count=n_over), n_over, indptr, indices, weights)
        del slot_idx, slot_w
        parts.append((indptr, indices, weights))
    return cat_csr(parts)


def minkowski_eps(xp, yp, cmp, eps, similarity=False, cap=256, keep_zero=False, rows_per_block=None):
    """f16_eps(minkowski_dense(xp, yp, similarity), cmp, eps, similarity) with ONE distance sweep per row block: exact
    counts plus up to `cap` entries per row in slots (pg_minkowski_eps_slots), scan, compaction, and a second sweep over
    just the rows with more than `cap` matches, written straight into the CSR (pg_minkowski_eps_fill_rows).  One host
    sync per block (nnz and the number of such rows); blocks keep the slots within 256 MB (_slots_eps).  keep_zero as in
    f16_eps.  Returns (indptr int64 [m+1], indices int32 [nnz], weights fp16 [nnz])."""
    if xp.d != yp.d:
        raise ValueError("operands must have the same dimension")
    L = lib()
    cap = max(1, int(cap))
    sel = (1 if similarity else 0, int(cmp) | (CMP_KEEP_ZERO if keep_zero else 0), float(np.float16(eps)))

    def call(fn, name, ops, *args):
        _check(fn(_ptr(xp.buf), xp.n, xp.npad, ops[0], ops[1], yp.npad, xp.d, *sel, *args, _stream()), name)

    return _slots_eps(
        yp.n, lambda r0, r1: _f16_rows(yp, r0, r1),
        lambda ops, si, sw, cnt: call(L.pg_minkowski_eps_slots, "pg_minkowski_eps_slots", ops, cap, _ptr(si), _ptr(sw), _ptr(cnt)),
        lambda *a: _check(L.pg_minkowski_eps_compact(*a), "pg_minkowski_eps_compact"),
        lambda ops, rows, n_over, ip, ix, w: call(L.pg_minkowski_eps_fill_rows, "pg_minkowski_eps_fill_rows", ops, _ptr(rows),
                                                  n_over, _ptr(ip), _ptr(ix), _ptr(w)),
        torch.float16, cap, rows_per_block, xp.buf.device)


class CosineOperand:
    """A PackedF16 with its pg_cosine_prep results: norms / rnorms fp32 [npad] (n and 1/sqrt(n) per vector) and
    `nonfinite` (a uint32[1] device flag, 1 when some element is inf or nan)."""
    __slots__ = ("packed", "norms", "rnorms", "flag")

    def __init__(self, packed, norms, rnorms, flag):
        self.packed, self.norms, self.rnorms, self.flag = packed, norms, rnorms, flag

    @property
    def n(self):
        return self.packed.n

    @property
    def d(self):
        return self.packed.d

    def nonfinite(self):
        """Does some element hold an inf or nan?  (reads the flag: a host sync)"""
        return bool(int(self.flag.item()))

    def rows(self, r0, r1):
        """(packed ptr, norms ptr, rnorms ptr, m) of vectors [r0, r1): the _f16_rows offset on all three arrays."""
        y, m = _f16_rows(self.packed, r0, r1)
        return y, ctypes.c_void_p(self.norms.data_ptr() + 4 * r0), ctypes.c_void_p(self.rnorms.data_ptr() + 4 * r0), m


def cosine_prep(x):
    """(N, D) fp16 device tensor (or a PackedF16) -> CosineOperand: the packed vectors, their fp32 norms and
    reciprocal roots from the cosine tile routine (pg_cosine_prep), and the non-finite flag."""
    xp = x if isinstance(x, PackedF16) else pack_f16(x)
    dev = xp.buf.device
    norms = torch.empty(xp.npad, dtype=torch.float32, device=dev)
    rnorms = torch.empty(xp.npad, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    _check(lib().pg_cosine_prep(_ptr(xp.buf), xp.n, xp.npad, xp.d, _ptr(norms), _ptr(rnorms), _ptr(flag), _stream()),
           "pg_cosine_prep")
    return CosineOperand(xp, norms, rnorms, flag)


def _cos_ops(xc, y, yn, yr, m, ynpad):
    if xc is None:
        raise TypeError("cosine operands come from cosine_prep")
    xp = xc.packed
    return [_ptr(xp.buf), _ptr(xc.norms), _ptr(xc.rnorms), xp.n, xp.npad, y, yn, yr, m, ynpad, xp.d]


def _cos_same_d(xc, yc):
    if xc.d != yc.d:
        raise ValueError("operands must have the same dimension")


def _cos_dense(metric, xc, yc, similarity):
    _cos_same_d(xc, yc)
    entry = f"pg_{metric}_dense"
    fn = getattr(lib(), entry)
    dev = xc.packed.buf.device
    out = torch.empty((yc.n, xc.n), dtype=torch.float32, device=dev)
    for r0 in range(0, yc.n, 65535 * 32):                            # grid.y limit of one launch
        y, yn, yr, m = yc.rows(r0, min(yc.n, r0 + 65535 * 32))
        _check(fn(*_cos_ops(xc, y, yn, yr, m, yc.packed.npad), 1 if similarity else 0, _ptr(out[r0:]), out.stride(0), _stream()),
               entry)
    return out


_COS_ROWS = 1 << 20          # Y rows per launch of the fused cosine / Euclidean kernels


def _cos_knn_round(metric, xc, yc, k, floor_idx, floor_w, idx_out, w_out, similarity, rows_per_block):
    entry = f"pg_{metric}_knn_round"
    fn = getattr(lib(), entry)
    fld, ldo = floor_idx.stride(0), idx_out.stride(0)
    for r0 in range(0, yc.n, rows_per_block):
        y, yn, yr, m = yc.rows(r0, min(yc.n, r0 + rows_per_block))
        _check(fn(*_cos_ops(xc, y, yn, yr, m, yc.packed.npad), 1 if similarity else 0, int(k), _ptr(floor_idx[r0:]),
                  _ptr(floor_w[r0:]), fld, _ptr(idx_out[r0:]), _ptr(w_out[r0:]), ldo, _stream()), entry)


def _cos_knn(metric, xc, yc, k, first, similarity, rows_per_block):
    _cos_same_d(xc, yc)
    if first + k > 64:
        head, more = globals()[metric + "_knn"], globals()[metric + "_knn_round"]      # the public wrappers, as they are now
        return knn_rounds(yc.n, int(k), int(first), torch.float32, xc.packed.buf.device,
                          lambda kk: head(xc, yc, kk, first, similarity, rows_per_block),
                          lambda kk, fi, fw, oi, ow: more(xc, yc, kk, fi, fw, oi, ow, similarity, rows_per_block))
    entry = f"pg_{metric}_knn"
    fn = getattr(lib(), entry)
    dev = xc.packed.buf.device
    idx = torch.empty((yc.n, int(k)), dtype=torch.int32, device=dev)
    w = torch.empty((yc.n, int(k)), dtype=torch.float32, device=dev)
    for r0 in range(0, yc.n, rows_per_block):
        y, yn, yr, m = yc.rows(r0, min(yc.n, r0 + rows_per_block))
        _check(fn(*_cos_ops(xc, y, yn, yr, m, yc.packed.npad), 1 if similarity else 0, int(k), int(first), _ptr(idx[r0:]),
                  _ptr(w[r0:]), _stream()), entry)
    return idx, w


def _cos_eps(metric, xc, yc, cmp, eps, similarity, cap, keep_zero, rows_per_block):
    _cos_same_d(xc, yc)
    L = lib()
    cap = max(1, int(cap))
    sel = (1 if similarity else 0, int(cmp) | (CMP_KEEP_ZERO if keep_zero else 0), float(np.float32(eps)))
    slots, fill = f"pg_{metric}_eps_slots", f"pg_{metric}_eps_fill_rows"

    def call(name, ops, *args):
        _check(getattr(L, name)(*_cos_ops(xc, *ops, yc.packed.npad), *sel, *args, _stream()), name)

    return _slots_eps(
        yc.n, yc.rows,
        lambda ops, si, sw, cnt: call(slots, ops, cap, _ptr(si), _ptr(sw), _ptr(cnt)),
        lambda *a: _check(L.pg_cosine_eps_compact(*a), "pg_cosine_eps_compact"),     # metric-free
        lambda ops, rows, n_over, ip, ix, w: call(fill, ops, _ptr(rows), n_over, _ptr(ip), _ptr(ix), _ptr(w)),
        torch.float32, cap, rows_per_block, xc.packed.buf.device)


def cosine_dense(xc, yc, similarity=False):
    """(M, N) fp32 block: cosine distance (or 1/(1+d)) of every Y vector against every X vector (pg_cosine_dense).
    Operands from cosine_prep; the caller checks their non-finite flags."""
    return _cos_dense("cosine", xc, yc, similarity)


def cosine_knn_round(xc, yc, k, floor_idx, floor_w, idx_out, w_out, similarity=False, rows_per_block=_COS_ROWS):
    """One round of pg_cosine_knn_round: the next k <= 64 ranks of every Y row after its floor, one fused sweep per
    block of Y rows (views as for f16_knn_round)."""
    _cos_knn_round("cosine", xc, yc, k, floor_idx, floor_w, idx_out, w_out, similarity, rows_per_block)


def cosine_knn(xc, yc, k, first=1, similarity=False, rows_per_block=_COS_ROWS):
    """Ranks first..first+k-1 of every row of cosine_dense(xc, yc, similarity) in (value, column) order - descending
    for similarities, ties by column - in one fused sweep (pg_cosine_knn), Y rows in blocks.
    Returns (idx int32 (m, k), w fp32 (m, k)); missing ranks idx -1, weight 0.
    first + k > 64 (k <= MAX_K_ROUNDS): one more sweep per 64 ranks (knn_rounds), in the same row blocks."""
    return _cos_knn("cosine", xc, yc, k, first, similarity, rows_per_block)


def cosine_eps(xc, yc, cmp, eps, similarity=False, cap=256, keep_zero=False, rows_per_block=None):
    """CSR of the entries of cosine_dense(xc, yc, similarity) with comp(d, eps) & (d > 0)  [comp(eps, s) & (s < 1)],
    `eps` rounded to fp32 first (as torch does when an fp32 tensor meets a Python number).  The minkowski_eps
    structure (_slots_eps): one sweep into per-row slots with exact counts, scan, compaction, and a second sweep over
    the rows with more than `cap` matches; one host sync per block of rows.  keep_zero: without the d > 0 (s < 1) test.
    Returns (indptr int64 [m+1], indices int32 [nnz], weights fp32 [nnz])."""
    return _cos_eps("cosine", xc, yc, cmp, eps, similarity, cap, keep_zero, rows_per_block)


def euclidean_dense(xc, yc, similarity=False):
    """cosine_dense with the Euclidean epilogue (pg_euclidean_dense): d = sqrt(max((nx + ny) - 2p, 0)) in fp32 steps, 0
    for identical vectors.  Operands from cosine_prep (their reciprocal roots are not read)."""
    return _cos_dense("euclidean", xc, yc, similarity)


def euclidean_knn_round(xc, yc, k, floor_idx, floor_w, idx_out, w_out, similarity=False, rows_per_block=_COS_ROWS):
    """cosine_knn_round over the Euclidean values (pg_euclidean_knn_round)."""
    _cos_knn_round("euclidean", xc, yc, k, floor_idx, floor_w, idx_out, w_out, similarity, rows_per_block)


def euclidean_knn(xc, yc, k, first=1, similarity=False, rows_per_block=_COS_ROWS):
    """cosine_knn over euclidean_dense(xc, yc, similarity) (pg_euclidean_knn; first + k > 64 in rounds up to MAX_K_ROUNDS)."""
    return _cos_knn("euclidean", xc, yc, k, first, similarity, rows_per_block)


def euclidean_eps(xc, yc, cmp, eps, similarity=False, cap=256, keep_zero=False, rows_per_block=None):
    """cosine_eps over euclidean_dense(xc, yc, similarity) (pg_euclidean_eps_slots / pg_euclidean_eps_fill_rows; the
    compaction is the metric-free pg_cosine_eps_compact)."""
    return _cos_eps("euclidean", xc, yc, cmp, eps, similarity, cap, keep_zero, rows_per_block)


COMM_ID_BYTES = 128


def comm_available():
    """Can this process bind RCCL (local check, not a collective)?"""
    try:
        return bool(lib().pg_comm_available())
    except NativeUnavailable:
        return False


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it, the host carries it to the other ranks)."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(lib().pg_comm_unique_id(buf), "pg_comm_unique_id")
    return buf.raw


def comm_init(nranks, rank, id_bytes):
    """RCCL communicator of this rank on the current HIP device; returns an opaque handle."""
    device()
    h = _vp(0)
    _check(lib().pg_comm_init(ctypes.byref(h), int(nranks), int(rank), ctypes.c_char_p(bytes(id_bytes))), "pg_comm_init")
    return h


def comm_destroy(comm):
    _check(lib().pg_comm_destroy(comm), "pg_comm_destroy")


def allgather_tokens(comm, shard, nranks):
    """(rows_per_rank, L) uint8 device shard of every rank -> (nranks*rows_per_rank, L) on every rank."""
    if shard.dtype != torch.uint8 or shard.dim() != 2 or not shard.is_cuda:
        raise TypeError("allgather_tokens expects a 2-D uint8 device tensor")
    shard = shard.contiguous()
    full = torch.empty((shard.shape[0] * int(nranks), shard.shape[1]), dtype=torch.uint8, device=shard.device)
    _check(lib().pg_allgather_tokens(comm, _ptr(shard), shard.shape[0], shard.shape[1], _ptr(full), _stream()), "pg_allgather_tokens")
    return full


def device_info():
    L = lib()
    device()
    cus, wave = _i32(0), _i32(0)
    arch = ctypes.create_string_buffer(64)
    _check(L.pg_device_info(ctypes.byref(cus), ctypes.byref(wave), arch, 64), "pg_device_info")
    return {"cus": cus.value, "wave": wave.value, "arch": arch.value.decode()}
