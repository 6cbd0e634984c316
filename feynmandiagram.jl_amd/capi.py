"""ctypes binding of the C ABI declared in include/fdg.h (libfdg.so).

This is the reference-side binding a maintainer would add, written for the
Python host (the Julia ``ccall`` twin is julia/hip_compiler.jl).  It is a thin
1:1 wrapper: no arithmetic happens on this side, and there is no fallback --
when the shared library (the HIP extension) is missing, importing any
evaluation entry point raises ``FdgLibraryMissing``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .nodetable import NodeTable

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FDG_LIBRARY") or os.path.join(_HERE, "lib", "libfdg.so")      # (FDG_LIBRARY: the dev tools point at lib/libfdg_dev.so, `make -C csrc dev`)
KERNEL_CACHE = os.path.join(_HERE, "kernel_cache")

FDG_OK = 0
FDG_E_INVALID, FDG_E_UNSUPPORTED, FDG_E_NO_DEVICE, FDG_E_NOMEM, FDG_E_JIT, FDG_E_INTERNAL = -1, -2, -3, -4, -5, -6
FDG_SPEC_DEFAULT, FDG_SPEC_KEEP_SOURCE, FDG_SPEC_FAST_MATH, FDG_SPEC_ISA, FDG_SPEC_AUTOTUNE = 0, 1, 2, 4, 8
# element types of leafVal / root (include/fdg.h FDG_DT_*); names as the reference's julia_to_C_typestr takes them (static.jl:135-153)
FDG_DT_F64, FDG_DT_F32, FDG_DT_C64, FDG_DT_C32 = 0, 1, 2, 3
DTYPES = {"Float64": FDG_DT_F64, "Float32": FDG_DT_F32, "ComplexF64": FDG_DT_C64, "ComplexF32": FDG_DT_C32}
FDG_SPEC_ROW_MAJOR_COMPANION = 16
FDG_ASSOC_STATIC, FDG_ASSOC_INTERP = 0, 1     # fdg_graph_set_association: static.jl's generated code / eval.jl's interpreter
FDG_TILE_SAMPLES = 64

EXPORTS = [
    "fdg_last_error", "fdg_version", "fdg_graph_create", "fdg_graph_destroy", "fdg_graph_query",
    "fdg_graph_emit_source", "fdg_free", "fdg_graph_specialize", "fdg_eval_device", "fdg_eval",
    "fdg_accumulate_device", "fdg_fill_uniform_device", "fdg_copy_device", "fdg_read_device", "fdg_clock_probe_device", "fdg_graph_specialize_typed", "fdg_eval_device_typed", "fdg_accumulate_device_typed", "fdg_graph_create_complex_view", "fdg_isa_check_hazards", "fdg_graph_release_device", "fdg_powi",
    "fdg_eval_strided", "fdg_graph_coop_program", "fdg_graph_set_opt_params", "fdg_graph_opt_program", "fdg_graph_set_schedule_groups", "fdg_leaf_eval_device", "fdg_leaf_eval_device_tiled",
    "fdg_comm_unique_id", "fdg_comm_create", "fdg_comm_destroy", "fdg_reduce_device",
    "fdg_graph_specialize_fused", "fdg_mc_eval_device", "fdg_mc_accumulate_device", "fdg_graph_mc_program",
    "fdg_graph_kernel_info",
    "fdg_eval_device_tiled", "fdg_accumulate_device_tiled", "fdg_fill_uniform_device_tiled", "fdg_graph_set_association",
    "fdg_batch_alloc", "fdg_batch_free", "fdg_graph_pool_program", "fdg_batch_alloc_pair", "fdg_graph_set_option", "fdg_graph_get_option", "fdg_set_default_option", "fdg_get_default_option", "fdg_selftest_pair_search",
    "fdg_repack_tile_major", "fdg_unpack_tile_major",
    "fdg_accumulate_device_binned", "fdg_mc_accumulate_device_binned",
    "fdg_accumulate_device_moments", "fdg_mc_accumulate_device_moments",
    "fdg_vegas_sample_device", "fdg_accumulate_device_vegas", "fdg_mc_accumulate_device_vegas", "fdg_vegas_refine",
    "fdg_vegas_sample_device_discrete", "fdg_accumulate_device_vegas_binned", "fdg_mc_accumulate_device_vegas_binned",
    "fdg_vegas_refine_discrete",
    "fdg_vegas_sample_device_polar", "fdg_sincos",
    "fdg_matsubara_phase", "fdg_accumulate_device_matsubara", "fdg_mc_accumulate_device_matsubara",
    "fdg_vegas_sample_device_grouped", "fdg_accumulate_device_grouped", "fdg_mc_accumulate_device_grouped",
    "fdg_accumulate_device_observables", "fdg_mc_accumulate_device_observables",
    "fdg_accumulate_device_freq_observables", "fdg_mc_accumulate_device_freq_observables",
    "fdg_vegas_sample_device_strat", "fdg_accumulate_device_strat", "fdg_mc_accumulate_device_strat", "fdg_strat_allocate",
    "fdg_vegas_sample_device_strat_grouped", "fdg_accumulate_device_strat_grouped", "fdg_mc_accumulate_device_strat_grouped",
    "fdg_strat_allocate_cols",
    "fdg_chain_propose_device", "fdg_chain_step_device", "fdg_mc_chain_step_device", "fdg_chain_reduce_device",
    "fdg_chain_step_device_matsubara", "fdg_mc_chain_step_device_matsubara",
    "fdg_chain_step_device_grouped", "fdg_mc_chain_step_device_grouped",
    "fdg_chain_propose_device_discrete", "fdg_chain_step_device_binned", "fdg_mc_chain_step_device_binned",
    "fdg_chain_propose_device_polar", "fdg_chain_propose_device_local",
    "fdg_chain_reduce_observables_work_bytes", "fdg_chain_reduce_device_observables",
]
FDG_BIN_MAX = 16384     # fdg_accumulate_device_binned: largest n_bin
FDG_VEGAS_DIM_MAX, FDG_VEGAS_GRID_MAX = 64, 1024     # the VEGAS map: most variables, most cells per variable
FDG_VEGAS_EXT_MAX = 16  # the discrete variable's table: most columns per value
FDG_VEGAS_POLAR_MAX = 21  # fdg_vegas_sample_device_polar: most groups of polar variables
FDG_MATSUBARA_FREQ_MAX = 64  # fdg_[mc_]accumulate_device_matsubara: most frequencies per call
FDG_WEIGHT_GROUP_MAX = 8  # fdg_weight_groups: most groups of roots with their own integration variables
FDG_OBS_MAX = 16  # fdg_observables: most linear combinations of the roots per call
FDG_FREQ_OBS_MAX = 8  # fdg_freq_observables: most linear combinations of the projected roots per call
FDG_STRAT_CUBE_MAX = 1 << 20  # the stratified calls: most hypercubes
FDG_CHAIN_INIT, FDG_CHAIN_MEASURE = 1, 2  # flags of fdg_[mc_]chain_step_device
FDG_CHAIN_BIN_MAX = 64  # fdg_[mc_]chain_step_device_binned: most values of the chain's discrete variable
# fdg_chain_reduce_device_observables: most rows per call, most columns of the window, the workgroups of the first stage
FDG_CHAIN_OBS_MAX, FDG_CHAIN_OBS_COL_MAX, FDG_CHAIN_OBS_GROUPS = 16, 1024, 1024
COMM_ID_BYTES = 128


class FdgLibraryMissing(ImportError):
    pass


class FdgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fdg error {code}: {msg}")
        self.code = code


class GraphDesc(C.Structure):
    _fields_ = [("n_leaf", C.c_uint32), ("n_node", C.c_uint32), ("n_root", C.c_uint32), ("n_edge", C.c_uint32),
                ("op", C.POINTER(C.c_uint8)), ("power", C.POINTER(C.c_int32)),
                ("child_off", C.POINTER(C.c_uint32)), ("child_idx", C.POINTER(C.c_uint32)),
                ("child_fac", C.POINTER(C.c_double)), ("root_slot", C.POINTER(C.c_uint32))]


class GraphInfo(C.Structure):
    _fields_ = [("n_leaf", C.c_uint32), ("n_node", C.c_uint32), ("n_root", C.c_uint32), ("n_edge", C.c_uint32),
                ("n_live_node", C.c_uint32), ("n_live_leaf", C.c_uint32),
                ("flops_alg", C.c_uint64), ("bytes_alg", C.c_uint64),
                ("max_live", C.c_uint32), ("n_slot_lds", C.c_uint32), ("n_slot_mem", C.c_uint32),
                ("n_ops", C.c_uint32), ("specialized", C.c_int32),
                ("spec_vgpr", C.c_uint32), ("spec_lds_bytes", C.c_uint32), ("spec_scratch_bytes", C.c_uint32)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class KernelInfo(C.Structure):
    _fields_ = [("last_kernel", C.c_char * 48), ("n_valu", C.c_uint64 * 3), ("n_ld_leaf", C.c_uint32 * 3),
                ("n_panel", C.c_uint32 * 3), ("n_lds", C.c_uint32 * 3), ("waves_per_cu", C.c_uint32 * 3),
                ("has_acc", C.c_uint32), ("has_rm", C.c_uint32), ("has_coop", C.c_uint32), ("rm_bufs", C.c_uint32),
                ("has_pool", C.c_uint32), ("pool_fetch", C.c_uint32), ("pool_valu", C.c_uint64),
                ("has_rl", C.c_uint32), ("last_launch", C.c_uint32), ("rl_valu", C.c_uint64)]


class LeafTables(C.Structure):
    _fields_ = [("n_leaf", C.c_uint32), ("n_basis", C.c_uint32), ("n_loop", C.c_uint32), ("dim", C.c_uint32),
                ("n_tau", C.c_uint32), ("leaf_type", C.c_void_p), ("leaf_order", C.c_void_p), ("tau_in", C.c_void_p),
                ("tau_out", C.c_void_p), ("loop_index", C.c_void_p), ("basis", C.c_void_p),
                ("kF", C.c_double), ("beta", C.c_double), ("lambda_", C.c_double)]


class Matsubara(C.Structure):
    """fdg_matsubara (include/fdg.h)"""
    _fields_ = [("n_freq", C.c_uint32), ("fermionic", C.c_int32), ("freq", C.c_void_p), ("root_tau_in", C.c_void_p),
                ("root_tau_out", C.c_void_p), ("beta", C.c_double), ("d_T", C.c_void_p), ("t_sample_stride", C.c_int64),
                ("t_comp_stride", C.c_int64), ("n_tau", C.c_uint32), ("d_acc_re", C.c_void_p), ("d_acc_im", C.c_void_p),
                ("d_acc2_re", C.c_void_p), ("d_acc2_im", C.c_void_p)]


class ChainMatsubara(C.Structure):
    """fdg_chain_matsubara (include/fdg.h)"""
    _fields_ = [("n_freq", C.c_uint32), ("fermionic", C.c_int32), ("freq", C.c_void_p), ("weight_freq", C.c_uint32),
                ("root_col_in", C.c_void_p), ("root_col_out", C.c_void_p), ("beta", C.c_double)]


class ChainGroups(C.Structure):
    """fdg_chain_groups (include/fdg.h)"""
    _fields_ = [("n_group", C.c_uint32), ("root_group", C.c_void_p), ("var_mask", C.c_void_p), ("reweight", C.c_void_p)]


class WeightGroups(C.Structure):
    """fdg_weight_groups (include/fdg.h)"""
    _fields_ = [("n_group", C.c_uint32), ("root_group", C.c_void_p), ("var_mask", C.c_void_p), ("weight_group_stride", C.c_int64)]


class Observables(C.Structure):
    """fdg_observables (include/fdg.h)"""
    _fields_ = [("n_obs", C.c_uint32), ("coef", C.c_void_p), ("d_obs", C.c_void_p), ("d_cov", C.c_void_p)]


class FreqObservables(C.Structure):
    """fdg_freq_observables (include/fdg.h)"""
    _fields_ = [("n_obs", C.c_uint32), ("coef", C.c_void_p), ("d_fobs", C.c_void_p), ("d_fcov", C.c_void_p)]


class OptParams(C.Structure):
    _fields_ = [("n_reg", C.c_uint32), ("n_lds", C.c_uint32), ("lookahead_lds", C.c_uint32),
                ("lookahead_mem", C.c_uint32), ("lookahead_leaf", C.c_uint32), ("n_acc", C.c_uint32),
                ("vn_window", C.c_uint32), ("fma", C.c_uint32), ("remat_window", C.c_uint32), ("remat_cost", C.c_uint32)]


class MOp(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("nega", C.c_uint8), ("negb", C.c_uint8), ("negc", C.c_uint8),
                ("d", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("imm", C.c_double),
                ("c", C.c_uint32), ("param", C.c_uint32)]


MOP_DTYPE = np.dtype([("kind", "u1"), ("nega", "u1"), ("negb", "u1"), ("negc", "u1"),
                      ("d", "<u4"), ("a", "<u4"), ("b", "<u4"), ("imm", "<f8"), ("c", "<u4"), ("param", "<u4")])

_lib = None


class BatchPairInfo(C.Structure):
    """fdg_batch_pair_info (include/fdg.h)"""
    _fields_ = [("leaf_bytes", C.c_uint64), ("root_bytes", C.c_uint64), ("chunk_tiles", C.c_uint64), ("n_chunk", C.c_uint32),
                ("n_candidate", C.c_uint32), ("n_filler", C.c_uint32), ("n_probe", C.c_uint32), ("n_matched", C.c_uint32),
                ("calibrated", C.c_uint32), ("gbs_fast", C.c_double), ("gbs_slow", C.c_double), ("gbs_before_mean", C.c_double),
                ("gbs_before_min", C.c_double), ("gbs_after_mean", C.c_double), ("gbs_after_min", C.c_double), ("seconds", C.c_double),
                ("seconds_settling", C.c_double), ("level_reached", C.c_uint32), ("span_gb", C.c_uint32)]


def lib():
    """Load libfdg.so once; fail loudly when the HIP extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FdgLibraryMissing(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C feynmandiagram.jl_amd/csrc). "
            "There is no CPU fallback for the evaluator.")
    # PyTorch wheels bundle their own libamdhip64/libhsa-runtime64.  One process
    # must use ONE HIP runtime, or device pointers and streams cannot be shared:
    # when torch is installed, load it first so libfdg.so binds to the runtime
    # torch already mapped (same SONAME) instead of a second copy from /opt/rocm.
    if not os.environ.get("FDG_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    # the code objects and tuned parameters shipped with the package: a read-only secondary lookup (fdg_runtime.hip: read_cached)
    L = C.CDLL(LIB_PATH)
    vp, i64, u64, u32, dp = C.c_void_p, C.c_int64, C.c_uint64, C.c_uint32, C.c_void_p
    L.fdg_last_error.restype = C.c_char_p
    L.fdg_version.restype = C.c_int
    L.fdg_graph_create.argtypes = [C.POINTER(GraphDesc), C.POINTER(vp)]
    L.fdg_graph_destroy.argtypes = [vp]
    L.fdg_graph_query.argtypes = [vp, C.POINTER(GraphInfo)]
    L.fdg_graph_kernel_info.argtypes = [vp, C.POINTER(KernelInfo)]
    L.fdg_graph_emit_source.argtypes = [vp, C.c_uint, C.POINTER(C.c_char_p)]
    L.fdg_free.argtypes = [vp]
    L.fdg_free.restype = None
    L.fdg_graph_specialize.argtypes = [vp, C.c_char_p, C.c_uint]
    L.fdg_eval_device.argtypes = [vp, dp, i64, i64, dp, i64, i64, i64, vp]
    L.fdg_eval.argtypes = [vp, dp, dp, i64]
    L.fdg_graph_set_association.argtypes = [vp, C.c_int]
    L.fdg_batch_alloc.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.fdg_batch_free.argtypes = [vp]
    L.fdg_graph_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.fdg_graph_get_option.argtypes = [vp, C.c_char_p]
    L.fdg_graph_get_option.restype = C.c_char_p
    L.fdg_set_default_option.argtypes = [C.c_char_p, C.c_char_p]
    L.fdg_get_default_option.argtypes = [C.c_char_p]
    L.fdg_get_default_option.restype = C.c_char_p
    L.fdg_selftest_pair_search.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.fdg_batch_alloc_pair.argtypes = [vp, C.c_int64, C.c_size_t, C.c_uint, C.POINTER(vp), C.POINTER(vp), C.POINTER(BatchPairInfo)]
    L.fdg_eval_device_tiled.argtypes = [vp, dp, i64, i64, i64, dp, i64, i64, i64, i64, vp]
    L.fdg_accumulate_device_tiled.argtypes = [vp, dp, i64, i64, i64, dp, dp, i64, vp]
    L.fdg_fill_uniform_device_tiled.argtypes = [dp, i64, u32, i64, i64, i64, u64, u64, vp]
    L.fdg_eval_strided.argtypes = [vp, dp, i64, i64, dp, i64, i64, i64]
    L.fdg_accumulate_device.argtypes = [vp, dp, i64, i64, dp, dp, i64, vp]
    L.fdg_fill_uniform_device.argtypes = [dp, i64, u32, i64, i64, u64, u64, vp]
    L.fdg_copy_device.argtypes = [dp, dp, i64, vp]
    L.fdg_read_device.argtypes = [dp, i64, dp, vp]
    L.fdg_repack_tile_major.argtypes = [dp, i64, i64, dp, i64, C.c_uint32, vp]
    L.fdg_unpack_tile_major.argtypes = [dp, dp, i64, i64, i64, C.c_uint32, vp]
    L.fdg_clock_probe_device.argtypes = [C.c_double, vp, vp]
    L.fdg_graph_specialize_typed.argtypes = [vp, C.c_int, C.c_char_p, C.c_uint]
    L.fdg_eval_device_typed.argtypes = [vp, C.c_int, vp, i64, i64, vp, i64, i64, i64, vp]
    L.fdg_accumulate_device_typed.argtypes = [vp, C.c_int, vp, i64, i64, vp, vp, vp, i64, vp]
    L.fdg_graph_create_complex_view.argtypes = [vp, C.POINTER(vp)]
    L.fdg_isa_check_hazards.argtypes = [C.c_char_p, C.POINTER(C.c_char_p)]
    L.fdg_graph_release_device.argtypes = [vp]
    L.fdg_leaf_eval_device.argtypes = [C.POINTER(LeafTables), dp, i64, i64, dp, i64, i64, dp, i64, i64, i64, vp]
    L.fdg_leaf_eval_device_tiled.argtypes = [C.POINTER(LeafTables), dp, i64, i64, dp, i64, i64, dp, i64, i64, i64, i64, vp]
    L.fdg_graph_set_schedule_groups.argtypes = [vp, C.c_void_p, u32]
    L.fdg_graph_set_opt_params.argtypes = [vp, C.POINTER(OptParams)]
    L.fdg_graph_opt_program.argtypes = [vp, C.POINTER(OptParams), C.POINTER(C.POINTER(MOp)), C.POINTER(C.c_uint64),
                                        C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.fdg_graph_mc_program.argtypes = [vp, C.POINTER(LeafTables), C.POINTER(OptParams), C.POINTER(C.POINTER(MOp)), C.POINTER(C.c_uint64),
                                       C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.fdg_graph_coop_program.argtypes = [vp, C.POINTER(OptParams), u32, C.POINTER(C.POINTER(MOp)), C.POINTER(C.c_uint64), C.POINTER(u32)]
    L.fdg_graph_pool_program.argtypes = [vp, C.POINTER(OptParams), u32, C.POINTER(C.POINTER(MOp)), C.POINTER(C.c_uint64), C.POINTER(u32)]
    L.fdg_graph_specialize_fused.argtypes = [vp, C.POINTER(LeafTables), C.c_char_p, C.c_uint]
    L.fdg_mc_eval_device.argtypes = [vp, dp, i64, i64, dp, i64, i64, C.c_double, C.c_double, C.c_double, dp, i64, i64, i64, vp]
    L.fdg_mc_accumulate_device.argtypes = [vp, dp, i64, i64, dp, i64, i64, C.c_double, C.c_double, C.c_double, dp, dp, i64, vp]
    L.fdg_vegas_sample_device.argtypes = [dp, u32, u32, C.c_void_p, u64, u64, dp, i64, i64, dp, dp, i64, vp]
    L.fdg_vegas_refine.argtypes = [C.c_void_p, C.c_void_p, u32, u32, C.c_double]
    L.fdg_vegas_sample_device_discrete.argtypes = [dp, u32, u32, C.c_void_p, dp, u32, C.c_int32, dp, u32, C.c_void_p, u64, u64, dp, i64, i64,
                                                   dp, dp, dp, i64, vp]
    L.fdg_vegas_refine_discrete.argtypes = [C.c_void_p, C.c_void_p, u32, C.c_double, C.c_double]
    L.fdg_comm_unique_id.argtypes = [C.c_void_p, C.c_size_t]
    L.fdg_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.fdg_comm_destroy.argtypes = [vp]
    L.fdg_reduce_device.argtypes = [vp, dp, u32, C.c_int, vp]
    L.fdg_vegas_sample_device_polar.argtypes = [dp, u32, u32, C.c_void_p, dp, u32, C.c_int32, dp, u32, C.c_void_p, C.c_void_p, u32, u64, u64,
                                                dp, i64, i64, dp, dp, dp, i64, vp]
    L.fdg_sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.fdg_sincos.restype = None
    L.fdg_matsubara_phase.argtypes = [C.c_double, C.c_double, C.c_int32, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.fdg_matsubara_phase.restype = None
    L.fdg_vegas_sample_device_grouped.argtypes = [dp, u32, u32, C.c_void_p, dp, u32, C.c_int32, dp, u32, C.c_void_p, C.c_void_p, u32,
                                                  C.c_void_p, u32, i64, u64, u64, dp, i64, i64, dp, dp, dp, i64, vp]
    L.fdg_vegas_sample_device_strat.argtypes = [dp, u32, u32, C.c_void_p, C.c_void_p, dp, u64, u64, dp, i64, i64, dp, dp, dp, i64, vp]
    L.fdg_strat_allocate.argtypes = [C.c_void_p, C.c_void_p, u32, u32, C.c_void_p, u32, i64, C.c_double, C.c_void_p]
    L.fdg_vegas_sample_device_strat_grouped.argtypes = [dp, u32, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, i64, C.c_void_p, dp, u64,
                                                        u64, dp, i64, i64, dp, dp, dp, i64, vp]
    L.fdg_strat_allocate_cols.argtypes = [C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, u32, i64, C.c_double, C.c_void_p]
    # the accumulate entries: the leaf or the Monte-Carlo prefix, then one tail for both, composed of the pieces fdg.h names
    leaf = [vp, dp, i64, i64, i64]                                                       # g, d_leaf, ss, ls, lts
    mc = [vp, dp, i64, i64, dp, i64, i64, C.c_double, C.c_double, C.c_double]            # g, d_K, ks, kc, d_T, ts, tc, kF, beta, lam
    bins, w, end = [dp, C.c_int32, u32], [dp], [i64, vp]                                 # d_bin, bin_base, n_bin; d_weight; B, stream
    train = [vp, u64, u64, u32, u32]                                                     # coef, seed, sample_offset, n_dim, n_grid
    vegas = w + train + [dp, dp, dp]                                                     # .. d_acc, d_acc2, d_hist
    vegas_binned = bins + vegas + [dp]                                                   # .. d_hist_bin
    strat = vegas + [vp, dp, dp, dp]                                                     # .. strat, d_cube, d_cube_sum, d_cube_sum2
    tails = {"binned": bins + w + [dp], "moments": bins + w + [dp, dp], "vegas": vegas, "vegas_binned": vegas_binned,
             "matsubara": vegas_binned + [vp], "grouped": vegas_binned + [vp] * 2, "observables": vegas_binned + [vp] * 3,
             "freq_observables": vegas_binned + [vp] * 4, "strat": strat, "strat_grouped": strat + [vp]}      # (the descriptors)
    for entry, tail in tails.items():
        getattr(L, "fdg_accumulate_device_" + entry).argtypes = leaf + tail + end
        getattr(L, "fdg_mc_accumulate_device_" + entry).argtypes = mc + tail + end
    L.fdg_chain_propose_device.argtypes = [dp, u32, u32, C.c_void_p, u32, u64, u64, u64, dp, i64, dp, dp, i64, dp, i64, vp]
    L.fdg_chain_step_device.argtypes = [vp, dp, i64, dp, u32, u32, C.c_void_p, C.c_double, u64, u64, C.c_uint, dp, i64, dp, dp, dp, dp, dp,
                                        i64, vp]
    L.fdg_mc_chain_step_device.argtypes = [vp, dp, i64, C.c_double, C.c_double, C.c_double, dp, u32, u32, C.c_void_p, C.c_double, u64, u64,
                                           C.c_uint, dp, i64, dp, dp, dp, dp, dp, i64, vp]
    L.fdg_chain_reduce_device.argtypes = [dp, u32, i64, dp, vp]
    L.fdg_chain_step_device_matsubara.argtypes = L.fdg_chain_step_device.argtypes[:-2] + [C.c_void_p, i64, vp]
    L.fdg_mc_chain_step_device_matsubara.argtypes = L.fdg_mc_chain_step_device.argtypes[:-2] + [C.c_void_p, i64, vp]
    L.fdg_chain_step_device_grouped.argtypes = L.fdg_chain_step_device.argtypes[:-2] + [C.c_void_p, C.c_void_p, i64, vp]
    L.fdg_mc_chain_step_device_grouped.argtypes = L.fdg_mc_chain_step_device.argtypes[:-2] + [C.c_void_p, C.c_void_p, i64, vp]
    L.fdg_chain_propose_device_discrete.argtypes = L.fdg_chain_propose_device.argtypes[:-2] + [C.c_int, dp, u32, dp, u32, C.c_void_p, vp, vp, i64, vp]
    L.fdg_chain_step_device_binned.argtypes = L.fdg_chain_step_device.argtypes[:-2] + [C.c_void_p, C.c_void_p, u32, vp, vp, i64, vp]
    L.fdg_mc_chain_step_device_binned.argtypes = L.fdg_mc_chain_step_device.argtypes[:-2] + [C.c_void_p, C.c_void_p, u32, vp, vp, i64, vp]
    L.fdg_chain_propose_device_polar.argtypes = L.fdg_chain_propose_device_discrete.argtypes[:-2] + [C.c_void_p, u32, i64, vp]
    L.fdg_chain_propose_device_local.argtypes = (L.fdg_chain_propose_device_polar.argtypes[:6] + [u64, C.c_void_p]
                                                 + L.fdg_chain_propose_device_polar.argtypes[6:])
    L.fdg_chain_reduce_observables_work_bytes.argtypes = [u32, u32]
    L.fdg_chain_reduce_observables_work_bytes.restype = C.c_size_t
    L.fdg_chain_reduce_device_observables.argtypes = [dp, i64, u32, u32, u32, C.c_void_p, u32, dp, vp, vp]
    L.fdg_powi.argtypes = [C.c_double, C.c_int32]
    L.fdg_powi.restype = C.c_double
    _lib = L
    # the code objects and tuned parameters shipped with the package: a read-only secondary lookup (fdg_runtime.hip: read_cached), appended
    # to what the environment names -- as a process default of the library, not by editing os.environ
    ro = (L.fdg_get_default_option(b"FDG_CACHE_RO_DIR") or b"").decode()
    if KERNEL_CACHE not in ro.split(":"):
        L.fdg_set_default_option(b"FDG_CACHE_RO_DIR", ((ro + ":" if ro else "") + KERNEL_CACHE).encode())
    return L


def check(rc: int):
    if rc != 0:
        raise FdgError(rc, lib().fdg_last_error().decode("utf-8", "replace"))


def _ptr(v):
    """One Python value as what a ``c_void_p`` parameter takes: None and 0 are the null pointer, any other int is an address, a ctypes
    structure (a descriptor) stands for its own address and a numpy array (a host vector) for its data."""
    if v is None:
        return None
    if isinstance(v, int):
        return v or None
    if isinstance(v, C.Structure):
        return C.addressof(v)
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    raise TypeError(f"a pointer argument must be None, an int, a ctypes structure or a numpy array, not {type(v).__name__}")


_POINTERS = {}      # GraphHandle._accumulate: entry -> (function, number of arguments, positions of the c_void_p arguments behind the graph)


class GraphHandle:
    """Owns one ``fdg_graph*``."""

    def __init__(self, table: NodeTable):
        t = table.normalized()
        t.validate()
        self.table = t
        d = GraphDesc()
        d.n_leaf, d.n_node, d.n_root, d.n_edge = t.n_leaf, t.n_node, t.n_root, t.n_edge
        d.op = t.op.ctypes.data_as(C.POINTER(C.c_uint8))
        d.power = t.power.ctypes.data_as(C.POINTER(C.c_int32))
        d.child_off = t.child_off.ctypes.data_as(C.POINTER(C.c_uint32))
        d.child_idx = t.child_idx.ctypes.data_as(C.POINTER(C.c_uint32))
        d.child_fac = t.child_fac.ctypes.data_as(C.POINTER(C.c_double))
        d.root_slot = t.root_slot.ctypes.data_as(C.POINTER(C.c_uint32))
        h = C.c_void_p()
        check(lib().fdg_graph_create(C.byref(d), C.byref(h)))
        self._h = h
        if getattr(t, "sched_group", None) is not None:
            self.set_schedule_groups(t.sched_group)

    def complex_view(self) -> "GraphHandle":
        """A new handle for this graph on Complex{Float64} values spelled out on real and imaginary parts (fdg_graph_create_complex_view):
        a Float64 graph with 2 L leaves and 2 R roots.  ``table`` of the result is the host mirror's statement of the same construction."""
        from .nodetable import complex_to_real
        h = C.c_void_p()
        check(lib().fdg_graph_create_complex_view(self._h, C.byref(h)))
        v = GraphHandle.__new__(GraphHandle)
        v.table = complex_to_real(self.table)
        v._h = h
        return v

    def set_option(self, name: str, value=None):
        """fdg_graph_set_option: one option of this handle (``None`` removes it).  Options replace the FDG_* environment switches: the
        library reads the environment once per process, for the supported names only."""
        check(lib().fdg_graph_set_option(self._h, name.encode(), None if value is None else str(value).encode()))

    def set_options(self, options):
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def get_option(self, name: str):
        v = lib().fdg_graph_get_option(self._h, name.encode())
        return None if v is None else v.decode()

    def set_association(self, assoc: int):
        """FDG_ASSOC_STATIC (the generated code, static.jl) or FDG_ASSOC_INTERP (eval!, eval.jl); before any specialisation."""
        check(lib().fdg_graph_set_association(self._h, assoc))

    def set_schedule_groups(self, group):
        if group is None:
            check(lib().fdg_graph_set_schedule_groups(self._h, None, 0))
            return
        g = np.ascontiguousarray(group, dtype=np.uint32)
        check(lib().fdg_graph_set_schedule_groups(self._h, g.ctypes.data, g.shape[0]))

    def close(self):
        if getattr(self, "_h", None):
            lib().fdg_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ptr(self):
        return self._h

    def info(self) -> dict:
        gi = GraphInfo()
        check(lib().fdg_graph_query(self._h, C.byref(gi)))
        return gi.asdict()

    def kernel_info(self) -> dict:
        """What the ISA kernels of this handle execute per evaluation (slot 0 evaluator, 1 accumulate, 2 row-major) and the
        name of the kernel the last device call launched."""
        ki = KernelInfo()
        check(lib().fdg_graph_kernel_info(self._h, C.byref(ki)))
        out = {"last_kernel": ki.last_kernel.decode()}
        for k in ("n_valu", "n_ld_leaf", "n_panel", "n_lds", "waves_per_cu"):
            out[k] = [int(x) for x in getattr(ki, k)]
        for k in ("has_acc", "has_rm", "has_coop", "rm_bufs", "has_pool", "pool_fetch", "pool_valu", "has_rl", "rl_valu"):
            out[k] = int(getattr(ki, k))
        # the last evaluator launch: its workgroups, and whether its waves claimed their tiles from a counter (FDG_ISA_TILE_CLAIM) or walked w, w + n, ...
        out["last_grid"] = int(ki.last_launch) & 0x7FFFFFFF
        out["tile_walk"] = "claimed" if int(ki.last_launch) >> 31 else "static"
        return out

    def emit_source(self, flags: int = 0) -> str:
        s = C.c_char_p()
        check(lib().fdg_graph_emit_source(self._h, flags, C.byref(s)))
        try:
            return s.value.decode()
        finally:
            lib().fdg_free(s)

    def set_opt_params(self, n_reg=0, n_lds=0, lookahead_lds=0, lookahead_mem=0, lookahead_leaf=0, n_acc=0, vn_window=0, fma=0, remat_window=0, remat_cost=0):
        q = OptParams(n_reg, n_lds, lookahead_lds, lookahead_mem, lookahead_leaf, n_acc, vn_window, fma, remat_window, remat_cost)
        check(lib().fdg_graph_set_opt_params(self._h, C.byref(q)))

    def opt_program(self, n_reg=0, n_lds=0, lookahead_lds=0, lookahead_mem=0, lookahead_leaf=0, n_acc=0, vn_window=0, fma=0, remat_window=0, remat_cost=0):
        """Returns ``(ops, n_reg_used, n_lds_used, n_mem_used)``; ops is a numpy record array (MOP_DTYPE)."""
        q = OptParams(n_reg, n_lds, lookahead_lds, lookahead_mem, lookahead_leaf, n_acc, vn_window, fma, remat_window, remat_cost)
        ops = C.POINTER(MOp)()
        n = C.c_uint64()
        nr, nl, nm, na = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().fdg_graph_opt_program(self._h, C.byref(q), C.byref(ops), C.byref(n), C.byref(nr), C.byref(nl),
                                          C.byref(nm), C.byref(na)))
        try:
            buf = C.string_at(ops, n.value * C.sizeof(MOp))
            arr = np.frombuffer(buf, dtype=MOP_DTYPE).copy()
        finally:
            lib().fdg_free(ops)
        self.last_n_acc = na.value
        return arr, nr.value, nl.value, nm.value

    def mc_program(self, tables, n_reg=0, n_lds=0, lookahead_lds=0, lookahead_mem=0, lookahead_leaf=0, n_acc=0, vn_window=0, fma=0, remat_window=0, remat_cost=0):
        """The program of the fused ISA step (leaves computed from the input columns K components, then times;
        ``tables`` from make_leaf_tables with kF, beta, lam set).  Returns like :meth:`opt_program`."""
        q = OptParams(n_reg, n_lds, lookahead_lds, lookahead_mem, lookahead_leaf, n_acc, vn_window, fma, remat_window, remat_cost)
        ops = C.POINTER(MOp)()
        n = C.c_uint64()
        nr, nl, nm, na = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().fdg_graph_mc_program(self._h, C.byref(tables), C.byref(q), C.byref(ops), C.byref(n), C.byref(nr),
                                         C.byref(nl), C.byref(nm), C.byref(na)))
        try:
            arr = np.frombuffer(C.string_at(ops, n.value * C.sizeof(MOp)), dtype=MOP_DTYPE).copy()
        finally:
            lib().fdg_free(ops)
        return arr, nr.value, nl.value, nm.value

    def pool_program(self, **kw):
        """The per-wave programs of the pooled cooperative variant (fdg_graph_pool_program): ``([ops_w0, ..], info)`` like
        :meth:`coop_program`; ``info["n_transfer"]`` is the number of leaf fetches per tile."""
        return self.coop_program(_pooled=True, **kw)

    def coop_program(self, _pooled=False, **kw):
        """The four per-wave programs of the cooperative variant: ``([ops_w0, .., ops_w3], info)`` with
        ``info = dict(n_reg, n_lds, n_mem, n_acc per wave; n_shared, n_epoch, n_transfer, n_duplicate)``."""
        q = OptParams(kw.get("n_reg", 0), kw.get("n_lds", 0), kw.get("lookahead_lds", 0), kw.get("lookahead_mem", 0),
                      kw.get("lookahead_leaf", 0), kw.get("n_acc", 0), kw.get("vn_window", 0), 0, 0, 0)
        progs, per_wave = [], []
        info = None
        for w in range(16):         # four waves, or 8 / 16 with FDG_COOP_WAVES
            ops = C.POINTER(MOp)()
            n = C.c_uint64()
            inf = (C.c_uint32 * 8)()
            rc = (lib().fdg_graph_pool_program if _pooled else lib().fdg_graph_coop_program)(self._h, C.byref(q), w, C.byref(ops), C.byref(n), inf)
            if rc != 0 and w >= 4:
                break
            check(rc)
            try:
                progs.append(np.frombuffer(C.string_at(ops, n.value * C.sizeof(MOp)), dtype=MOP_DTYPE).copy())
            finally:
                lib().fdg_free(ops)
            per_wave.append(dict(n_reg=inf[0], n_lds=inf[1], n_mem=inf[2], n_acc=inf[3]))
            info = dict(n_shared=inf[4], n_epoch=inf[5], n_transfer=inf[6], n_duplicate=inf[7], waves=per_wave)
        return progs, info

    def specialize(self, cache_dir: Optional[str] = None, flags: int = 0):
        """``cache_dir`` None: the library's per-user cache ($FDG_CACHE_DIR, $XDG_CACHE_HOME/fdg, ~/.cache/fdg); the
        kernel_cache directory shipped inside the package is only *read* (``FDG_CACHE_RO_DIR``, set in :func:`lib`), so a
        root-owned or read-only installation works.  ``__graft_entry__.build()`` passes ``KERNEL_CACHE`` to fill it."""
        check(lib().fdg_graph_specialize(self._h, cache_dir.encode() if cache_dir else None, flags))

    def specialize_typed(self, dtype: int, cache_dir: Optional[str] = None, flags: int = 0):
        """The per-graph kernel for an element type other than Float64 (FDG_DT_*)."""
        check(lib().fdg_graph_specialize_typed(self._h, dtype, cache_dir.encode() if cache_dir else None, flags))

    def eval_device_typed(self, dtype: int, d_leaf: int, ss: int, ls: int, d_root: int, rs: int, rk: int, B: int, stream: int = 0):
        check(lib().fdg_eval_device_typed(self._h, dtype, d_leaf, ss, ls, d_root, rs, rk, B, stream))

    def accumulate_device_typed(self, dtype: int, d_leaf: int, ss: int, ls: int, d_weight: int, d_acc: int, d_acc2: int, B: int, stream: int = 0):
        """``acc[k] += sum_b w[b] * root_k(b)`` for leaves of an element type FDG_DT_* (``d_acc2``: the squares as well; 0 = not wanted)."""
        check(lib().fdg_accumulate_device_typed(self._h, dtype, d_leaf, ss, ls, d_weight or None, d_acc or None, d_acc2 or None, B, stream))

    # raw-pointer device entry points (ints are device addresses) ----------- #
    def eval_device(self, d_leaf: int, ss: int, ls: int, d_root: int, rs: int, rk: int, B: int, stream: int = 0):
        check(lib().fdg_eval_device(self._h, d_leaf, ss, ls, d_root, rs, rk, B, stream))

    def accumulate_device(self, d_leaf: int, ss: int, ls: int, d_weight: int, d_acc: int, B: int, stream: int = 0):
        check(lib().fdg_accumulate_device(self._h, d_leaf, ss, ls, d_weight or None, d_acc, B, stream))

    # tile-major batches: sample b at (b // 64) * tile stride + (b % 64) * sample stride (fdg.h) ------------------- #
    def eval_device_tiled(self, d_leaf: int, ss: int, ls: int, lts: int, d_root: int, rs: int, rk: int, rts: int, B: int, stream: int = 0):
        check(lib().fdg_eval_device_tiled(self._h, d_leaf, ss, ls, lts, d_root, rs, rk, rts, B, stream))

    def accumulate_device_tiled(self, d_leaf: int, ss: int, ls: int, lts: int, d_weight: int, d_acc: int, B: int, stream: int = 0):
        check(lib().fdg_accumulate_device_tiled(self._h, d_leaf, ss, ls, lts, d_weight or None, d_acc, B, stream))

    def _accumulate(self, entry: str, src, *tail):
        """fdg_[mc_]accumulate_device_ + ``entry``: ``src`` is ``(d_leaf, ss, ls, lts)`` (the leaf form) or
        ``(d_K, ks, kc, d_T, ts, tc, kF, beta, lam)`` (the Monte-Carlo form), ``tail`` the rest in the order of fdg.h.  Every pointer
        argument goes through :func:`_ptr`: 0 and None are null, a descriptor stands for its address, a host array for its data."""
        name = ("fdg_accumulate_device_" if len(src) == 4 else "fdg_mc_accumulate_device_") + entry
        if name not in _POINTERS:                   # the entry's function, its argument count and its pointer positions, looked up once
            fn = getattr(lib(), name)
            _POINTERS[name] = (fn, len(fn.argtypes), [i for i, t in enumerate(fn.argtypes) if i and t is C.c_void_p])
        fn, n, pointers = _POINTERS[name]
        args = [self._h, *src, *tail]
        if len(args) != n:
            raise TypeError(f"{name} takes {n - 1} arguments behind the graph ({len(args) - 1} given)")
        for i in pointers:
            args[i] = _ptr(args[i])
        check(fn(*args))

    # binned accumulation: d_acc[j * R + k] += w[b] root_k(b) for j = d_bin[b] - bin_base in [0, n_bin) (fdg.h) ---------------- #
    def accumulate_device_binned(self, d_leaf: int, ss: int, ls: int, lts: int, d_bin: int, bin_base: int, n_bin: int, d_weight: int,
                                 d_acc: int, B: int, stream: int = 0):
        self._accumulate("binned", (d_leaf, ss, ls, lts), d_bin, bin_base, n_bin, d_weight, d_acc, B, stream)

    def mc_accumulate_device_binned(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_bin, bin_base, n_bin, d_weight, d_acc, B, stream=0):
        self._accumulate("binned", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_bin, bin_base, n_bin, d_weight, d_acc, B, stream)

    # second moments as well: d_acc2[j * R + k] += (w[b] root_k(b))^2; d_bin 0 = every sample in bin 0 (n_bin 1) (fdg.h) ------- #
    def accumulate_device_moments(self, d_leaf: int, ss: int, ls: int, lts: int, d_bin: int, bin_base: int, n_bin: int, d_weight: int,
                                  d_acc: int, d_acc2: int, B: int, stream: int = 0):
        self._accumulate("moments", (d_leaf, ss, ls, lts), d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream)

    def mc_accumulate_device_moments(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B,
                                     stream=0):
        self._accumulate("moments", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream)

    # one VEGAS iteration's accumulate step: both moments (the bits of the moments calls with d_bin 0, n_bin 1) and the training histogram
    # d_hist[d * n_grid + c] += (w[b] sum_k coef[k] root_k(b))^2, c = the cell of counter (sample_offset + b, d); coef: host vector or None (fdg.h)
    def accumulate_device_vegas(self, d_leaf: int, ss: int, ls: int, lts: int, d_weight: int, coef, seed: int, sample_offset: int, n_dim: int,
                                n_grid: int, d_acc: int, d_acc2: int, d_hist: int, B: int, stream: int = 0):
        self._accumulate("vegas", (d_leaf, ss, ls, lts), d_weight, self._coef(coef), seed, sample_offset, n_dim, n_grid, d_acc, d_acc2,
                         d_hist, B, stream)

    def mc_accumulate_device_vegas(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_weight, coef, seed, sample_offset, n_dim, n_grid, d_acc,
                                   d_acc2, d_hist, B, stream=0):
        self._accumulate("vegas", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_weight, self._coef(coef), seed, sample_offset, n_dim, n_grid,
                         d_acc, d_acc2, d_hist, B, stream)

    # the same with a discrete variable: binned moments (the bits of the moments calls with this d_bin), the training histogram over the
    # samples whose bin is in range, and d_hist_bin[j] += (w[b] sum_k coef[k] root_k(b))^2 over the samples of bin j (0: not trained) (fdg.h)
    def accumulate_device_vegas_binned(self, d_leaf: int, ss: int, ls: int, lts: int, d_bin: int, bin_base: int, n_bin: int, d_weight: int,
                                       coef, seed: int, sample_offset: int, n_dim: int, n_grid: int, d_acc: int, d_acc2: int, d_hist: int,
                                       d_hist_bin: int, B: int, stream: int = 0):
        self._accumulate("vegas_binned", (d_leaf, ss, ls, lts), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed, sample_offset,
                         n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, B, stream)

    def mc_accumulate_device_vegas_binned(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_bin, bin_base, n_bin, d_weight, coef, seed,
                                          sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, B, stream=0):
        self._accumulate("vegas_binned", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_bin, bin_base, n_bin, d_weight, self._coef(coef),
                         seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, B, stream)

    # the projection onto Matsubara frequencies: desc = make_matsubara(...)[0]; d_bin 0: no discrete variable; d_acc and d_acc2 both 0: no
    # unprojected moments; n_dim 0 and d_hist 0: no training, else the bits of the VEGAS calls in d_hist (and d_hist_bin) (fdg.h)
    def accumulate_device_matsubara(self, d_leaf: int, ss: int, ls: int, lts: int, d_bin: int, bin_base: int, n_bin: int, d_weight: int,
                                    desc, coef=None, seed: int = 0, sample_offset: int = 0, n_dim: int = 0, n_grid: int = 0, d_acc: int = 0,
                                    d_acc2: int = 0, d_hist: int = 0, d_hist_bin: int = 0, B: int = 0, stream: int = 0):
        self._accumulate("matsubara", (d_leaf, ss, ls, lts), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed, sample_offset,
                         n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, B, stream)

    def mc_accumulate_device_matsubara(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_bin, bin_base, n_bin, d_weight, desc, coef=None,
                                       seed=0, sample_offset=0, n_dim=0, n_grid=0, d_acc=0, d_acc2=0, d_hist=0, d_hist_bin=0, B=0, stream=0):
        self._accumulate("matsubara", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed,
                         sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, B, stream)

    # weight groups: groups = make_weight_groups(...)[0], d_weight [n_group, stride]; desc None: no projection; the rest as the
    # projection calls take it (fdg.h)
    def accumulate_device_grouped(self, d_leaf: int, ss: int, ls: int, lts: int, d_bin: int, bin_base: int, n_bin: int, d_weight: int,
                                  groups, desc=None, coef=None, seed: int = 0, sample_offset: int = 0, n_dim: int = 0, n_grid: int = 0,
                                  d_acc: int = 0, d_acc2: int = 0, d_hist: int = 0, d_hist_bin: int = 0, B: int = 0, stream: int = 0):
        self._accumulate("grouped", (d_leaf, ss, ls, lts), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed, sample_offset, n_dim,
                         n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, groups, B, stream)

    def mc_accumulate_device_grouped(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_bin, bin_base, n_bin, d_weight, groups, desc=None,
                                     coef=None, seed=0, sample_offset=0, n_dim=0, n_grid=0, d_acc=0, d_acc2=0, d_hist=0, d_hist_bin=0, B=0,
                                     stream=0):
        self._accumulate("grouped", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed,
                         sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, groups, B, stream)

    # observables: obs = make_observables(...)[0]; groups None: one weight column (or none with d_weight 0); d_acc and d_acc2 both 0:
    # no per-root moments; the rest as the grouped calls take it (fdg.h)
    def accumulate_device_observables(self, d_leaf: int, ss: int, ls: int, lts: int, d_bin: int, bin_base: int, n_bin: int, d_weight: int,
                                      obs, groups=None, desc=None, coef=None, seed: int = 0, sample_offset: int = 0, n_dim: int = 0,
                                      n_grid: int = 0, d_acc: int = 0, d_acc2: int = 0, d_hist: int = 0, d_hist_bin: int = 0, B: int = 0,
                                      stream: int = 0):
        self._accumulate("observables", (d_leaf, ss, ls, lts), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed, sample_offset,
                         n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, groups, obs, B, stream)

    def mc_accumulate_device_observables(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_bin, bin_base, n_bin, d_weight, obs, groups=None,
                                         desc=None, coef=None, seed=0, sample_offset=0, n_dim=0, n_grid=0, d_acc=0, d_acc2=0, d_hist=0,
                                         d_hist_bin=0, B=0, stream=0):
        self._accumulate("observables", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed,
                         sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, groups, obs, B, stream)

    # frequency observables: fobs = make_freq_observables(...)[0] and desc (required: the frequencies, time labels, beta, T; its four
    # arrays all 0: no per-root projection); obs and groups may be None; the rest as the observables calls take it (fdg.h)
    def accumulate_device_freq_observables(self, d_leaf: int, ss: int, ls: int, lts: int, d_bin: int, bin_base: int, n_bin: int,
                                           d_weight: int, fobs, desc, obs=None, groups=None, coef=None, seed: int = 0, sample_offset: int = 0,
                                           n_dim: int = 0, n_grid: int = 0, d_acc: int = 0, d_acc2: int = 0, d_hist: int = 0,
                                           d_hist_bin: int = 0, B: int = 0, stream: int = 0):
        self._accumulate("freq_observables", (d_leaf, ss, ls, lts), d_bin, bin_base, n_bin, d_weight, self._coef(coef), seed, sample_offset,
                         n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, groups, obs, fobs, B, stream)

    def mc_accumulate_device_freq_observables(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_bin, bin_base, n_bin, d_weight, fobs, desc,
                                              obs=None, groups=None, coef=None, seed=0, sample_offset=0, n_dim=0, n_grid=0, d_acc=0, d_acc2=0,
                                              d_hist=0, d_hist_bin=0, B=0, stream=0):
        self._accumulate("freq_observables", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_bin, bin_base, n_bin, d_weight, self._coef(coef),
                         seed, sample_offset, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, desc, groups, obs, fobs, B, stream)

    # the stratified accumulate step: the _vegas calls plus the training cells by the stratified formula (d_cube: the sampler's
    # hypercubes) and the per-hypercube moments d_cube_sum, d_cube_sum2 [H, n_root + 1]; strat: host sequence of n_dim counts (fdg.h)
    def accumulate_device_strat(self, d_leaf: int, ss: int, ls: int, lts: int, d_weight: int, coef, seed: int, sample_offset: int, n_dim: int,
                                n_grid: int, d_acc: int, d_acc2: int, d_hist: int, strat, d_cube: int, d_cube_sum: int, d_cube_sum2: int,
                                B: int, stream: int = 0):
        self._accumulate("strat", (d_leaf, ss, ls, lts), d_weight, self._coef(coef), seed, sample_offset, n_dim, n_grid, d_acc, d_acc2,
                         d_hist, _strat_array(strat, n_dim), d_cube, d_cube_sum, d_cube_sum2, B, stream)

    def mc_accumulate_device_strat(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_weight, coef, seed, sample_offset, n_dim, n_grid, d_acc,
                                   d_acc2, d_hist, strat, d_cube, d_cube_sum, d_cube_sum2, B, stream=0):
        self._accumulate("strat", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_weight, self._coef(coef), seed, sample_offset, n_dim, n_grid,
                         d_acc, d_acc2, d_hist, _strat_array(strat, n_dim), d_cube, d_cube_sum, d_cube_sum2, B, stream)

    # the stratified grouped accumulate step: the _strat calls plus groups = make_weight_groups(...)[0], d_weight [n_group, stride];
    # d_cube_sum, d_cube_sum2 [H, n_root + n_group] (fdg.h)
    def accumulate_device_strat_grouped(self, d_leaf: int, ss: int, ls: int, lts: int, d_weight: int, coef, seed: int, sample_offset: int,
                                        n_dim: int, n_grid: int, d_acc: int, d_acc2: int, d_hist: int, strat, d_cube: int, d_cube_sum: int,
                                        d_cube_sum2: int, groups, B: int, stream: int = 0):
        self._accumulate("strat_grouped", (d_leaf, ss, ls, lts), d_weight, self._coef(coef), seed, sample_offset, n_dim, n_grid, d_acc,
                         d_acc2, d_hist, _strat_array(strat, n_dim), d_cube, d_cube_sum, d_cube_sum2, groups, B, stream)

    def mc_accumulate_device_strat_grouped(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_weight, coef, seed, sample_offset, n_dim, n_grid,
                                           d_acc, d_acc2, d_hist, strat, d_cube, d_cube_sum, d_cube_sum2, groups, B, stream=0):
        self._accumulate("strat_grouped", (d_K, ks, kc, d_T, ts, tc, kF, beta, lam), d_weight, self._coef(coef), seed, sample_offset, n_dim,
                         n_grid, d_acc, d_acc2, d_hist, _strat_array(strat, n_dim), d_cube, d_cube_sum, d_cube_sum2, groups, B, stream)

    # one step of the Markov chain on the VEGAS map after fdg_chain_propose_device: evaluate the proposals (d_xp: [n_col, B] with column
    # stride xpc), fold, accept, select into the state (x, fac, root, a), measure into sum [n_root + 1, B] with FDG_CHAIN_MEASURE (fdg.h)
    def chain_step_device(self, d_xp: int, xpc: int, d_facp: int, n_col: int, n_dim: int, coef, gamma: float, seed: int, sample_offset: int,
                          flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int, d_sum: int, d_n_accept: int, B: int,
                          stream: int = 0):
        self._chain_step("", None, d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac, d_root, d_a, d_sum,
                         d_n_accept, B, stream)

    def mc_chain_step_device(self, d_xp: int, xpc: int, kF, beta, lam, d_facp: int, n_col: int, n_dim: int, coef, gamma: float, seed: int,
                             sample_offset: int, flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int, d_sum: int,
                             d_n_accept: int, B: int, stream: int = 0):
        self._chain_step("", (kF, beta, lam), d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac, d_root,
                         d_a, d_sum, d_n_accept, B, stream)

    # the same steps with the Matsubara projection in the weight and in the measurement: desc = make_chain_matsubara(...)[0], d_sum
    # [2 n_freq n_root + 1, B] (fdg.h, "Markov chain with a Matsubara-projected weight and measurement")
    def chain_step_device_matsubara(self, d_xp: int, xpc: int, d_facp: int, n_col: int, n_dim: int, coef, gamma: float, seed: int,
                                    sample_offset: int, flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int, d_sum: int,
                                    d_n_accept: int, desc, B: int, stream: int = 0):
        self._chain_step("_matsubara", None, d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac, d_root,
                         d_a, d_sum, d_n_accept, B, stream, desc)

    def mc_chain_step_device_matsubara(self, d_xp: int, xpc: int, kF, beta, lam, d_facp: int, n_col: int, n_dim: int, coef, gamma: float,
                                       seed: int, sample_offset: int, flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int,
                                       d_sum: int, d_n_accept: int, desc, B: int, stream: int = 0):
        self._chain_step("_matsubara", (kF, beta, lam), d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac,
                         d_root, d_a, d_sum, d_n_accept, B, stream, desc)

    # the same steps with weight groups: groups = make_chain_groups(...)[0]; desc = make_chain_matsubara(...)[0] or None (no projection),
    # d_sum as in the plain or the projected step (fdg.h, "Markov chain with weight groups and reweighting between orders")
    def chain_step_device_grouped(self, d_xp: int, xpc: int, d_facp: int, n_col: int, n_dim: int, coef, gamma: float, seed: int,
                                  sample_offset: int, flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int, d_sum: int,
                                  d_n_accept: int, desc, groups, B: int, stream: int = 0):
        self._chain_step("_grouped", None, d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac, d_root,
                         d_a, d_sum, d_n_accept, B, stream, desc, groups)

    def mc_chain_step_device_grouped(self, d_xp: int, xpc: int, kF, beta, lam, d_facp: int, n_col: int, n_dim: int, coef, gamma: float,
                                     seed: int, sample_offset: int, flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int,
                                     d_sum: int, d_n_accept: int, desc, groups, B: int, stream: int = 0):
        self._chain_step("_grouped", (kF, beta, lam), d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac,
                         d_root, d_a, d_sum, d_n_accept, B, stream, desc, groups)

    # the same steps with one discrete variable behind the continuous ones: desc and groups as in the grouped step, each may be None;
    # d_fac / d_facp [n_dim + 1, B], d_bin / d_binp int32 [B], d_sum [n_bin n_root + 1, B] or [2 n_bin n_freq n_root + 1, B]
    # (fdg.h, "Markov chain with a discrete external variable and per-bin measurement")
    def chain_step_device_binned(self, d_xp: int, xpc: int, d_facp: int, n_col: int, n_dim: int, coef, gamma: float, seed: int,
                                 sample_offset: int, flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int, d_sum: int,
                                 d_n_accept: int, desc, groups, n_bin: int, d_binp: int, d_bin: int, B: int, stream: int = 0):
        self._chain_step("_binned", None, d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac, d_root,
                         d_a, d_sum, d_n_accept, B, stream, desc, groups, (n_bin, d_binp, d_bin))

    def mc_chain_step_device_binned(self, d_xp: int, xpc: int, kF, beta, lam, d_facp: int, n_col: int, n_dim: int, coef, gamma: float,
                                    seed: int, sample_offset: int, flags: int, d_x: int, xc: int, d_fac: int, d_root: int, d_a: int,
                                    d_sum: int, d_n_accept: int, desc, groups, n_bin: int, d_binp: int, d_bin: int, B: int, stream: int = 0):
        self._chain_step("_binned", (kF, beta, lam), d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac,
                         d_root, d_a, d_sum, d_n_accept, B, stream, desc, groups, (n_bin, d_binp, d_bin))

    def _chain_step(self, entry: str, mc, d_xp, xpc, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, xc, d_fac, d_root, d_a,
                    d_sum, d_n_accept, B, stream=0, desc=None, groups=None, binned=None):
        """fdg_[mc_]chain_step_device + ``entry``: ``mc`` None (the leaf form) or ``(kF, beta, lam)``; ``entry`` "" takes no descriptor,
        "_matsubara" ``desc``, "_grouped" ``desc`` and ``groups`` (each None: a null pointer), "_binned" those two and
        ``binned = (n_bin, d_binp, d_bin)``."""
        c = self._coef(coef)
        fn = getattr(lib(), ("fdg_chain_step_device" if mc is None else "fdg_mc_chain_step_device") + entry)
        descs = {"": (), "_matsubara": (desc,), "_grouped": (desc, groups), "_binned": (desc, groups)}[entry]
        bins = (binned[0], _ptr(binned[1]), _ptr(binned[2])) if entry == "_binned" else ()
        check(fn(self._h, _ptr(d_xp), xpc, *(mc or ()), _ptr(d_facp), n_col, n_dim, _ptr(c), gamma, seed, sample_offset, flags, _ptr(d_x), xc,
                 _ptr(d_fac), _ptr(d_root), _ptr(d_a), _ptr(d_sum), _ptr(d_n_accept), *(_ptr(d) for d in descs), *bins, B, stream))

    def _coef(self, coef):
        if coef is None:
            return None
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.shape != (self.table.n_root,):
            raise ValueError(f"coef must hold n_root = {self.table.n_root} factors")
        return c

    # fused Monte-Carlo step: leaves from (K, T) in registers, then the graph --------------------- #
    def specialize_fused(self, tables, cache_dir: Optional[str] = None, flags: int = 0):
        """``tables`` = the struct returned by make_leaf_tables."""
        check(lib().fdg_graph_specialize_fused(self._h, C.byref(tables), cache_dir.encode() if cache_dir else None, flags))

    def mc_eval_device(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_root, rs, rk, B, stream=0):
        check(lib().fdg_mc_eval_device(self._h, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_root, rs, rk, B, stream))

    def mc_accumulate_device(self, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_weight, d_acc, B, stream=0):
        check(lib().fdg_mc_accumulate_device(self._h, d_K, ks, kc, d_T, ts, tc, kF, beta, lam, d_weight or None, d_acc, B, stream))

    def eval_host(self, leaf: np.ndarray, root: Optional[np.ndarray] = None) -> np.ndarray:
        """Host matrices ``leaf [B, >= L]`` -> ``root [B, R]``, each C-ordered (compile_Python's row-major layout) or
        Fortran-ordered (what a Julia ``Matrix`` is); no transposition copy is made for either (fdg_eval_strided)."""
        leaf = np.asarray(leaf, dtype=np.float64)
        if leaf.ndim != 2 or leaf.shape[1] < self.table.n_leaf:
            raise IndexError("BoundsError: leafVal has fewer columns than the graph has leaves")
        if not (leaf.flags.c_contiguous or leaf.flags.f_contiguous):
            leaf = np.ascontiguousarray(leaf)
        B = leaf.shape[0]
        if root is None:
            root = np.zeros((B, self.table.n_root), dtype=np.float64, order="C" if leaf.flags.c_contiguous else "F")
        if root.dtype != np.float64 or not (root.flags.c_contiguous or root.flags.f_contiguous) or root.shape != (B, self.table.n_root):
            raise ValueError("root must be a contiguous (C- or Fortran-ordered) float64 [B, R] array")
        ss, ls = (leaf.shape[1], 1) if leaf.flags.c_contiguous else (1, B)
        rs, rk = (self.table.n_root, 1) if root.flags.c_contiguous else (1, B)
        check(lib().fdg_eval_strided(self._h, leaf.ctypes.data, ss, ls, root.ctypes.data, rs, rk, B))
        return root

    def release_device(self):
        check(lib().fdg_graph_release_device(self._h))


def fill_uniform_device(d_leaf: int, B: int, L: int, ss: int, ls: int, seed: int, sample_offset: int = 0,
                        stream: int = 0):
    check(lib().fdg_fill_uniform_device(d_leaf, B, L, ss, ls, seed, sample_offset, stream))


def fill_uniform_device_tiled(d_leaf: int, B: int, L: int, ss: int, ls: int, lts: int, seed: int, sample_offset: int = 0,
                               stream: int = 0):
    check(lib().fdg_fill_uniform_device_tiled(d_leaf, B, L, ss, ls, lts, seed, sample_offset, stream))


def _col_arg(col, n_dim: int, none_ok: bool = False):
    """The ``col`` argument of the samplers and proposals as a uint32 array, or None.  ``none_ok``: None entries stand for 0 (the
    polar wrappers: the entry of a grouped variable is not read)."""
    if col is None:
        return None
    c = np.ascontiguousarray([0 if v is None else v for v in col] if none_ok else col, dtype=np.uint32)
    if c.shape != (n_dim,):
        raise ValueError("col must name one column per variable")
    return c


def _ext_col_arg(ext_col) -> np.ndarray:
    """The ``ext_col`` argument of the discrete variable's table as a uint32 array (None: empty)."""
    e = np.ascontiguousarray([] if ext_col is None else ext_col, dtype=np.uint32)
    if e.ndim != 1:
        raise ValueError("ext_col must be a sequence of column numbers")
    return e


def vegas_sample_device(d_grid: int, n_dim: int, n_grid: int, col, seed: int, sample_offset: int, d_x: int, xs: int, xc: int, d_jac: int,
                        d_cell: int, B: int, stream: int = 0):
    """fdg_vegas_sample_device: ``x[b * xs + col[d] * xc]`` drawn through the map ``d_grid`` (device, ``[n_dim, n_grid + 1]`` edges),
    ``jac[b]`` its weight, ``cell[d * B + b]`` when ``d_cell`` is not 0.  ``col``: host sequence of ``n_dim`` column numbers or None."""
    c = _col_arg(col, n_dim)
    check(lib().fdg_vegas_sample_device(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, seed, sample_offset,
                                        d_x or None, xs, xc, d_jac or None, d_cell or None, B, stream))


def chain_propose_device(d_grid: int, n_dim: int, n_grid: int, col, n_col: int, mask: int, seed: int, sample_offset: int, d_x: int, xc: int,
                         d_fac: int, d_xp: int, xpc: int, d_facp: int, B: int, stream: int = 0):
    """fdg_chain_propose_device: the proposal ``xp [n_col, B]`` / ``facp [n_dim, B]`` of every walker -- the variables of ``mask`` redrawn
    through the map for counter ``(sample_offset + b, d)``, everything else copied from ``x`` / ``fac``."""
    c = _col_arg(col, n_dim)
    check(lib().fdg_chain_propose_device(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, n_col, mask, seed, sample_offset,
                                         d_x or None, xc, d_fac or None, d_xp or None, xpc, d_facp or None, B, stream))


def chain_propose_device_discrete(d_grid: int, n_dim: int, n_grid: int, col, n_col: int, mask: int, seed: int, sample_offset: int, d_x: int,
                                  xc: int, d_fac: int, d_xp: int, xpc: int, d_facp: int, move_discrete: bool, d_cdf: int, n_bin: int, d_ext: int,
                                  ext_col, d_bin: int, d_binp: int, B: int, stream: int = 0):
    """fdg_chain_propose_device_discrete: :func:`chain_propose_device` and, with ``move_discrete``, the discrete variable redrawn from
    ``d_cdf [n_bin + 1]`` for counter ``(sample_offset + b, n_dim)``: ``binp [B]`` (int32) its value, ``facp[n_dim]`` the factor
    ``1 / p_j``, the columns ``ext_col`` (a host sequence) of ``xp`` row ``j`` of ``d_ext [n_bin, len(ext_col)]``; otherwise copied."""
    c = _col_arg(col, n_dim)
    ec = _ext_col_arg(ext_col)
    check(lib().fdg_chain_propose_device_discrete(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, n_col, mask, seed,
                                                  sample_offset, d_x or None, xc, d_fac or None, d_xp or None, xpc, d_facp or None,
                                                  1 if move_discrete else 0, d_cdf or None, n_bin, d_ext or None, ec.shape[0],
                                                  ec.ctypes.data if ec.shape[0] else None, d_bin or None, d_binp or None, B, stream))


def chain_propose_device_polar(d_grid: int, n_dim: int, n_grid: int, col, n_col: int, mask: int, seed: int, sample_offset: int, d_x: int,
                               xc: int, d_fac: int, d_xp: int, xpc: int, d_facp: int, move_discrete: bool, d_cdf: int, n_bin: int, d_ext: int,
                               ext_col, d_bin: int, d_binp: int, polar, B: int, stream: int = 0):
    """fdg_chain_propose_device_polar: :func:`chain_propose_device_discrete` (``d_cdf`` 0: :func:`chain_propose_device`; the discrete
    variable's arguments are then ignored and ``fac`` / ``facp`` have ``n_dim`` rows) with groups of variables read as a modulus and a
    direction.  ``polar``: a sequence of ``(var, cols)`` as :func:`vegas_sample_device_polar` takes it; a group is redrawn whole (every
    one of its bits in ``mask``) or kept, and the factors of the polar measure go to the group's own rows of ``facp``.  The ``col``
    entry of a grouped variable is not read (None stands for 0 there)."""
    c = _col_arg(col, n_dim, none_ok=True)
    ec = _ext_col_arg(ext_col)
    arr, n_polar = _polar_array(polar)
    check(lib().fdg_chain_propose_device_polar(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, n_col, mask, seed,
                                               sample_offset, d_x or None, xc, d_fac or None, d_xp or None, xpc, d_facp or None,
                                               1 if move_discrete else 0, d_cdf or None, n_bin, d_ext or None, ec.shape[0],
                                               ec.ctypes.data if ec.shape[0] else None, d_bin or None, d_binp or None,
                                               C.addressof(arr) if n_polar else None, n_polar, B, stream))


def sincos_table(x):
    """``(s, c)`` of fdg_sincos for an array of doubles in ``[0, 2 pi]``: one call of the library's routine per entry."""
    x = np.asarray(x, dtype=np.float64)
    s, c = np.empty(x.shape), np.empty(x.shape)
    fn, vs, vc = lib().fdg_sincos, C.c_double(), C.c_double()
    ps, pc = C.byref(vs), C.byref(vc)
    for i, v in enumerate(x.ravel().tolist()):
        fn(v, ps, pc)
        s.flat[i], c.flat[i] = vs.value, vc.value
    return s, c


def chain_propose_polar_reference(grid, col, polar, state, mask: int, u, cdf=None, ext=None, ext_col=(), move_discrete: bool = False,
                                  u_disc=None, sincos=None):
    """fdg_chain_propose_device_polar restated in numpy, in the device's fp64 order: ``(xp, facp, binp)`` of the state's ``x``, ``fac``
    (and ``bin``), ``binp`` None without a discrete variable (``cdf`` None).  The variables of no group and the discrete variable are
    drawn by the statements of the chain mirrors' proposal (:func:`chain_reference`, :func:`chain_binned_reference`); ``polar`` holds
    ``(var, cols)`` pairs; ``u [B, D]`` the uniforms of the counters ``(sample_offset + b, d)`` (only the columns of ``mask`` are
    read), ``u_disc [B]`` those of column ``n_dim``.  ``sincos(x) -> (s, c)`` replaces :func:`sincos_table`, the library's own routine
    entry by entry, by a faster one with the same bits.  The step mirrors take the result as their ``proposal``."""
    sc = sincos_table if sincos is None else sincos
    grid = np.asarray(grid, dtype=np.float64)
    D, G = grid.shape[0], grid.shape[1] - 1
    x, fac = np.array(state["x"], dtype=np.float64), np.array(state["fac"], dtype=np.float64)
    B = x.shape[1]
    groups = [(int(var), tuple(int(c) for c in cols)) for var, cols in (polar or ())]
    grouped = set()
    for var, cols in groups:
        mine = set(range(var, var + len(cols)))
        if len(cols) not in (2, 3) or var < 0 or var + len(cols) > D or mine & grouped:
            raise ValueError("a polar group has 2 or 3 variables inside the map, apart from every other group's")
        has = [(mask >> d) & 1 for d in sorted(mine)]
        if any(has) and not all(has):
            raise ValueError("mask names some but not all variables of a polar group")
        grouped |= mine
    if fac.shape != (D + (cdf is not None), B):
        raise ValueError("fac must be [n_dim, n_walker], or [n_dim + 1, n_walker] with a discrete variable")
    cols_of = list(range(D)) if col is None else [None if c is None else int(c) for c in col]
    xp, facp = x.copy(), fac.copy()

    def draw(d):
        y = np.asarray(u, dtype=np.float64)[:, d] * np.float64(G)
        c = np.minimum(y.astype(np.int64), G - 1)
        lo = grid[d, c]
        wd = grid[d, c + 1] - lo
        return lo + (y - c.astype(np.float64)) * wd, np.float64(G) * wd

    for d in range(D):
        if d not in grouped and (mask >> d) & 1:
            xp[cols_of[d]], facp[d] = draw(d)
    for var, cols in groups:
        if not (mask >> var) & 1:
            continue
        k, fk = draw(var)
        va, fa = draw(var + 1)
        if len(cols) == 3:
            vp, fp = draw(var + 2)
            st, ct = sc(va)
            sp, cp = sc(vp)
            ks = k * st
            xp[cols[0]], xp[cols[1]], xp[cols[2]] = ks * cp, ks * sp, k * ct
            f0 = fk * k
            facp[var], facp[var + 1], facp[var + 2] = f0 * k, fa * st, fp
        else:
            sp, cp = sc(va)
            xp[cols[0]], xp[cols[1]] = k * cp, k * sp
            facp[var], facp[var + 1] = fk * k, fa
    binp = None
    if cdf is not None:
        cdf = np.asarray(cdf, dtype=np.float64)
        n_bin = cdf.shape[0] - 1
        binp = np.array(state["bin"], dtype=np.int32)
        if move_discrete:
            ud = np.asarray(u_disc, dtype=np.float64)
            jp = np.searchsorted(cdf[1:n_bin], ud, side="right")        # the number of interior edges <= u
            with np.errstate(all="ignore"):
                facp[D] = 1.0 / (cdf[jp + 1] - cdf[jp])
            binp = jp.astype(np.int32)
            for e, c in enumerate(ext_col):
                xp[int(c)] = np.asarray(ext, dtype=np.float64)[jp, e]
    return xp, facp, binp


def _width_arg(width, n_dim: int, local_mask: int):
    """The ``width`` argument of the shifted proposal as a float64 array ``[n_dim]`` (a scalar stands for every variable), or None
    where no variable is shifted and none is given."""
    if width is None:
        if local_mask:
            raise ValueError("a shift mask needs width")
        return None
    w = np.asarray(width, dtype=np.float64)
    w = np.full(n_dim, float(w)) if w.ndim == 0 else np.ascontiguousarray(w)
    if w.shape != (n_dim,):
        raise ValueError("width must be one number or one per variable")
    return w


def chain_propose_device_local(d_grid: int, n_dim: int, n_grid: int, col, n_col: int, mask: int, local_mask: int, width, seed: int,
                               sample_offset: int, d_x: int, xc: int, d_fac: int, d_xp: int, xpc: int, d_facp: int, move_discrete: bool = False,
                               d_cdf: int = 0, n_bin: int = 0, d_ext: int = 0, ext_col=None, d_bin: int = 0, d_binp: int = 0, polar=(),
                               B: int = 0, stream: int = 0):
    """fdg_chain_propose_device_local: :func:`chain_propose_device_polar` with the variables of ``local_mask`` SHIFTED in the map's
    coordinate, ``y' = y + t h (mod 1)`` with ``t`` uniform in ``[-1, 1)`` on the counter a redraw of the variable would use and
    ``h = width[d]`` in ``(0, 0.5]`` (``width``: a host sequence of ``n_dim`` numbers, or one number for all; read only where
    ``local_mask`` has a bit).  ``mask`` and ``local_mask`` share no bit.  Only variables of no polar group can be shifted; the groups
    and the discrete variable are redrawn or kept.  ``local_mask = 0`` is :func:`chain_propose_device_polar` bit for bit."""
    c = _col_arg(col, n_dim, none_ok=True)
    ec = _ext_col_arg(ext_col)
    arr, n_polar = _polar_array(polar)
    w = _width_arg(width, n_dim, local_mask)
    check(lib().fdg_chain_propose_device_local(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, n_col, mask, local_mask,
                                               None if w is None else w.ctypes.data, seed, sample_offset, d_x or None, xc, d_fac or None,
                                               d_xp or None, xpc, d_facp or None, 1 if move_discrete else 0, d_cdf or None, n_bin,
                                               d_ext or None, ec.shape[0], ec.ctypes.data if ec.shape[0] else None, d_bin or None,
                                               d_binp or None, C.addressof(arr) if n_polar else None, n_polar, B, stream))


def vegas_invert_reference(grid, d: int, xv):
    """The inverse of the map for variable ``d`` restated in numpy, in the device's fp64 order (include/fdg.h, "Markov chain with local
    shift moves"): ``(c, fr)`` of the values ``xv``, with ``yy = c + fr`` the coordinate in cells.  ``c`` is the number of interior
    edges ``<= xv``; ``fr`` is clamped into ``[0, 1]``, 0 for a cell without width and for a nan."""
    e = np.asarray(grid, dtype=np.float64)[d]
    G = e.shape[0] - 1
    xv = np.asarray(xv, dtype=np.float64)
    c = np.searchsorted(e[1:G], xv, side="right")            # the number of interior edges <= xv (a nan sorts behind them all ...)
    c = np.where(np.isnan(xv), 0, c)                         # ... but compares false with every edge on the device
    lo = e[c]
    wd = e[c + 1] - lo
    with np.errstate(all="ignore"):
        fr = (xv - lo) / wd
    fr = np.where((wd == 0.0) | ~(fr >= 0.0), 0.0, fr)
    fr = np.where(fr > 1.0, 1.0, fr)
    return c, fr


def chain_propose_local_reference(grid, col, polar, state, mask: int, local_mask: int, width, u, cdf=None, ext=None, ext_col=(),
                                  move_discrete: bool = False, u_disc=None, sincos=None):
    """fdg_chain_propose_device_local restated in numpy, in the device's fp64 order: :func:`chain_propose_polar_reference` for ``mask``,
    the groups and the discrete variable, then every variable of ``local_mask`` shifted from the state's value: the inverse of the map
    (:func:`vegas_invert_reference`), ``y1 = yy + ((u + u) - 1) * (width[d] * G)`` wrapped once into ``[0, G)``, the map again.
    ``u [B, D]`` holds the uniforms of the counters ``(sample_offset + b, d)``; the columns of ``mask`` and of ``local_mask`` are read.
    ``width``: one number or one per variable.  The step mirrors take the result as their ``proposal``, so stepping through
    :func:`chain_grouped_reference` or :func:`chain_binned_reference` works unchanged behind it."""
    grid = np.asarray(grid, dtype=np.float64)
    D, G = grid.shape[0], grid.shape[1] - 1
    mask, local_mask = int(mask), int(local_mask)
    if local_mask >> D:
        raise ValueError("local_mask names a variable >= n_dim")
    if mask & local_mask:
        raise ValueError("mask and local_mask name the same variable")
    for var, cols in (polar or ()):
        if local_mask & (((1 << len(cols)) - 1) << int(var)):
            raise ValueError("local_mask names a variable of a polar group")
    xp, facp, binp = chain_propose_polar_reference(grid, col, polar, state, mask, u, cdf, ext, ext_col, move_discrete, u_disc, sincos)
    if not local_mask:
        return xp, facp, binp
    w = _width_arg(width, D, local_mask)
    x = np.asarray(state["x"], dtype=np.float64)
    cols_of = list(range(D)) if col is None else [None if c is None else int(c) for c in col]
    g = np.float64(G)
    for d in range(D):
        if not (local_mask >> d) & 1:
            continue
        if not (np.isfinite(w[d]) and 0.0 < w[d] <= 0.5):
            raise ValueError("a width of a shifted variable is not in (0, 0.5]")
        hG = w[d] * g
        c, fr = vegas_invert_reference(grid, d, x[cols_of[d]])
        yy = c.astype(np.float64) + fr
        ud = np.asarray(u, dtype=np.float64)[:, d]
        t = (ud + ud) - 1.0
        y1 = yy + t * hG
        y1 = np.where(y1 < 0.0, y1 + g, y1)
        y1 = np.where(y1 >= g, y1 - g, y1)
        c1 = np.minimum(y1.astype(np.int64), G - 1)
        lo = grid[d, c1]
        wd = grid[d, c1 + 1] - lo
        xp[cols_of[d]] = lo + (y1 - c1.astype(np.float64)) * wd
        facp[d] = g * wd
    return xp, facp, binp


def chain_reduce_device(d_sum: int, n_root: int, B: int, d_out: int, stream: int = 0):
    """fdg_chain_reduce_device: ``out [3 R + 2] +=`` (S [R + 1], Q [R + 1], X [R]) of the walkers' sums ``[n_root + 1, B]``."""
    check(lib().fdg_chain_reduce_device(d_sum or None, n_root, B, d_out or None, stream))


def chain_reduce_reference(total) -> np.ndarray:
    """fdg_chain_reduce_device restated: ``(S, Q, X)`` of ``total [R + 1, B]`` as one ``[3 R + 2]`` vector.  The products are formed in
    fp64 as on the device; the sums over the walkers are exact (math.fsum), so the device's agree within its own rounding."""
    import math
    A = np.asarray(total, dtype=np.float64)
    R = A.shape[0] - 1
    out = [math.fsum(A[c]) for c in range(R + 1)] + [math.fsum(A[c] * A[c]) for c in range(R + 1)] + [math.fsum(A[k] * A[R]) for k in range(R)]
    return np.array(out, dtype=np.float64)


def chain_reduce_observables_work_bytes(n_obs: int, n_use: int) -> int:
    """fdg_chain_reduce_observables_work_bytes: the bytes of ``d_work`` for a call with these sizes, 0 where the call is refused."""
    return int(lib().fdg_chain_reduce_observables_work_bytes(n_obs, n_use))


def chain_reduce_observables_device(d_sum: int, B: int, col_base: int, n_use: int, norm_col: int, coef, d_out: int, d_work: int,
                                    stream: int = 0):
    """fdg_chain_reduce_device_observables: ``out [(M + 1) + (M + 1) (M + 2) / 2] +=`` (S, P packed) of the rows ``coef [M, n_use]``
    (host) over the window ``col_base .. col_base + n_use - 1`` of the walkers' sums, with the column ``norm_col`` as row ``M``;
    ``d_work`` holds :func:`chain_reduce_observables_work_bytes` bytes."""
    c = np.ascontiguousarray(coef, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != n_use:
        raise ValueError(f"coef must be [n_obs, n_use = {n_use}]")
    check(lib().fdg_chain_reduce_device_observables(d_sum or None, B, col_base, n_use, norm_col, c.ctypes.data, c.shape[0], d_out or None,
                                                    d_work or None, stream))


def _chain_obs_sum(x, W: int) -> float:
    """``x [n]`` added in the order of fdg_chain_reduce_device_observables with ``W`` workgroups: strided lane sums, the pairwise tree
    of a workgroup, the strided sums of the workgroups' partials, the tree again."""
    def tree(v):                                            # v [.., 256]: stride 128, 64, .., 1
        h = 128
        while h:
            v = v[..., :h] + v[..., h:2 * h]
            h >>= 1
        return v[..., 0]

    def strided(v, step):                                   # v [n] -> [step]: entry s adds v[s], v[s + step], .. ascending from +0.0
        k = -(-v.shape[0] // step)
        pad = np.zeros(k * step)
        pad[:v.shape[0]] = v                                 # (a missing term: nothing is added there -- + 0.0 keeps every bit but
        acc = np.zeros(step)                                 # -0.0's sign, which a sum begun at +0.0 cannot hold)
        for i in range(k):
            acc = acc + pad[i * step:(i + 1) * step]
        return acc
    part = tree(strided(np.asarray(x, dtype=np.float64), 256 * W).reshape(W, 256))
    return float(tree(strided(part, 256)))


def chain_reduce_observables_reference(total, col_base: int, n_use: int, norm_col: int, coef, out=None) -> np.ndarray:
    """fdg_chain_reduce_device_observables restated in the device's order, bit for bit: ``out`` (None: zeros) with the ``V = (M + 1) +
    (M + 1) (M + 2) / 2`` sums ``(S, P packed)`` of ``total [n_columns, B]`` added to it, as a new array.  The outputs of a row
    without a term are left as they are, as on the device."""
    A = np.asarray(total, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64)
    M, B = c.shape[0], A.shape[1]
    W = min(max(-(-B // 256), 1), FDG_CHAIN_OBS_GROUPS)
    O = []
    for m in range(M):
        o = None
        for k in range(n_use):
            if c[m, k] != 0.0:
                term = c[m, k] * A[col_base + k]
                o = term if o is None else o + term
        O.append(o)
    O.append(A[norm_col])
    V = (M + 1) + (M + 1) * (M + 2) // 2
    out = np.zeros(V) if out is None else np.array(out, dtype=np.float64)
    if out.shape != (V,):
        raise ValueError(f"out must hold {V} doubles")
    if B == 0:
        return out
    at = M + 1
    for p in range(M + 1):
        if O[p] is not None:
            out[p] = out[p] + _chain_obs_sum(O[p], W)
        for q in range(p, M + 1):
            if O[p] is not None and O[q] is not None:
                out[at] = out[at] + _chain_obs_sum(O[p] * O[q], W)
            at += 1
    return out


def chain_reference(grid, col, state, mask: int, u, u_acc, gamma: float, flags: int, eval_roots, coef=None, exists=None):
    """One chain step restated in numpy (include/fdg.h, "Markov-chain sampling on the VEGAS map"): fdg_chain_propose_device, then
    fdg_[mc_]chain_step_device, in the device's fp64 order, so that the state compares bit for bit.

    ``grid [D, G + 1]`` the map; ``col [D]`` the column of each variable (None: ``d``); ``state`` a dict of ``x [n_col, B]``,
    ``fac [D, B]``, ``root [R, B]``, ``a [B]``, ``sum [R + 1, B]``, ``n_accept [B]`` (int32); ``u [B, D]`` the uniforms of the counters
    ``(sample_offset + b, d)`` (only the columns of ``mask`` are read); ``u_acc [B]`` those of ``(sample_offset + b, FDG_VEGAS_DIM_MAX)``
    (not read with FDG_CHAIN_INIT); ``eval_roots(xp) -> [R, B]`` the roots of the proposals ``xp [n_col, B]``; ``exists`` a bool per
    root (None: all).  Returns the new state (new arrays; columns of roots that do not exist are carried over) with ``xp``, ``facp``
    (the proposal) and ``accept [B]`` beside it.  :func:`chain_reduce_reference` restates the reduction."""
    grid = np.asarray(grid, dtype=np.float64)
    D, G = grid.shape[0], grid.shape[1] - 1
    x, fac, root, a = (np.array(state[k], dtype=np.float64) for k in ("x", "fac", "root", "a"))
    total, n_acc = np.array(state["sum"], dtype=np.float64), np.array(state["n_accept"], dtype=np.int32)
    B, R = x.shape[1], root.shape[0]
    cols = list(range(D)) if col is None else [int(c) for c in col]
    live = [k for k in range(R) if exists is None or exists[k]]
    xp, facp = x.copy(), fac.copy()
    for d in range(D):
        if (mask >> d) & 1:
            y = np.asarray(u, dtype=np.float64)[:, d] * np.float64(G)
            c = np.minimum(y.astype(np.int64), G - 1)
            lo = grid[d, c]
            wd = grid[d, c + 1] - lo
            xp[cols[d]] = lo + (y - c.astype(np.float64)) * wd
            facp[d] = np.float64(G) * wd
    with np.errstate(all="ignore"):
        rp = np.asarray(eval_roots(xp), dtype=np.float64) if live else np.zeros((R, B))
        jp = facp[0].copy()
        for d in range(1, D):
            jp = jp * facp[d]
        s, bad = None, np.zeros(B, dtype=bool)
        for k in live:
            bad |= ~np.isfinite(rp[k])
            term = rp[k] if coef is None else np.float64(coef[k]) * rp[k]
            s = term if s is None else s + term
        if s is None:
            s = np.zeros(B)
        tp = jp * s
        bad |= ~np.isfinite(tp)
        ap = np.where(bad, 0.0, np.abs(tp))
        if flags & FDG_CHAIN_INIT:
            acc = np.ones(B, dtype=bool)
        else:
            acc = np.asarray(u_acc, dtype=np.float64) * (a + gamma) < (ap + gamma)
    x, fac, a = np.where(acc, xp, x), np.where(acc, facp, fac), np.where(acc, ap, a)
    for k in live:
        root[k] = np.where(acc, np.where(bad, 0.0, rp[k]), root[k])
    n_acc = n_acc + acc.astype(np.int32)
    if flags & FDG_CHAIN_MEASURE:
        jac = fac[0].copy()
        for d in range(1, D):
            jac = jac * fac[d]
        dd = 1.0 / (a + gamma)
        for k in live:
            total[k] = total[k] + (jac * root[k]) * dd
        total[R] = total[R] + dd
    return {"x": x, "fac": fac, "root": root, "a": a, "sum": total, "n_accept": n_acc, "xp": xp, "facp": facp, "accept": acc}


def make_chain_matsubara(freq, fermionic, weight_freq: int, root_col_in, root_col_out, beta: float):
    """``(fdg_chain_matsubara struct, keepalive)``: ``freq`` the n of every frequency, ``weight_freq`` the index of the one the chain's
    weight is projected onto, ``root_col_in`` / ``root_col_out`` the 0-based columns of ``x`` that hold every root's two times."""
    f = np.ascontiguousarray(freq, dtype=np.int32)
    cin, cout = (np.ascontiguousarray(v, dtype=np.uint32) for v in (root_col_in, root_col_out))
    if f.ndim != 1 or cin.ndim != 1 or cin.shape != cout.shape:
        raise ValueError("freq must be a sequence, root_col_in and root_col_out one column per root each")
    m = ChainMatsubara(f.shape[0], 1 if fermionic else 0, f.ctypes.data, int(weight_freq), cin.ctypes.data, cout.ctypes.data, float(beta))
    return m, (f, cin, cout)


def chain_matsubara_reference(grid, col, state, mask: int, u, u_acc, gamma: float, flags: int, eval_roots, freq, fermionic, weight_freq: int,
                              root_col_in, root_col_out, beta: float, coef=None, exists=None, phase_table=None):
    """One step of the projected chain restated in numpy (include/fdg.h, "Markov chain with a Matsubara-projected weight and
    measurement"): fdg_chain_propose_device, then fdg_[mc_]chain_step_device_matsubara, in the device's fp64 order, so that the state
    and the sums compare bit for bit.  The arguments of :func:`chain_reference`, with ``state["sum"]`` ``[2 F R + 1, B]``, and the
    descriptor's: ``freq [F]``, ``fermionic``, ``weight_freq``, the 0-based time columns ``root_col_in`` / ``root_col_out [R]`` and
    ``beta``.  The phases are the library's own (fdg_matsubara_phase through :func:`matsubara_phase_table`), one table per distinct
    pair of columns; ``phase_table(tau, beta, freq, fermionic) -> (s, c) [B, F]`` replaces that routine by a faster one with the
    same bits."""
    table = matsubara_phase_table if phase_table is None else phase_table
    grid = np.asarray(grid, dtype=np.float64)
    D, G = grid.shape[0], grid.shape[1] - 1
    x, fac, root, a = (np.array(state[k], dtype=np.float64) for k in ("x", "fac", "root", "a"))
    total, n_acc = np.array(state["sum"], dtype=np.float64), np.array(state["n_accept"], dtype=np.int32)
    B, R, F, wf = x.shape[1], root.shape[0], len(freq), int(weight_freq)
    if total.shape != (2 * F * R + 1, B) or not 0 <= wf < F:
        raise ValueError("sum must be [2 n_freq n_root + 1, n_walker] and weight_freq an index into freq")
    cols = list(range(D)) if col is None else [int(c) for c in col]
    live = [k for k in range(R) if exists is None or exists[k]]
    pairs = {k: (int(root_col_in[k]), int(root_col_out[k])) for k in live}

    def phases(p, fs):
        out = {}
        for pair in set(pairs.values()):
            tau = p[pair[1]] - p[pair[0]]
            out[pair] = table(tau, beta, fs, fermionic)
        return out

    xp, facp = x.copy(), fac.copy()
    for d in range(D):
        if (mask >> d) & 1:
            y = np.asarray(u, dtype=np.float64)[:, d] * np.float64(G)
            c = np.minimum(y.astype(np.int64), G - 1)
            lo = grid[d, c]
            wd = grid[d, c + 1] - lo
            xp[cols[d]] = lo + (y - c.astype(np.float64)) * wd
            facp[d] = np.float64(G) * wd
    with np.errstate(all="ignore"):
        rp = np.asarray(eval_roots(xp), dtype=np.float64) if live else np.zeros((R, B))
        jp = facp[0].copy()
        for d in range(1, D):
            jp = jp * facp[d]
        ph = phases(xp, [freq[wf]])
        re, im, bad = None, None, np.zeros(B, dtype=bool)
        for k in live:
            bad |= ~np.isfinite(rp[k])
            term = rp[k] if coef is None else np.float64(coef[k]) * rp[k]
            s, c = ph[pairs[k]]
            pr, pi = term * c[:, 0], term * s[:, 0]
            re, im = (pr, pi) if re is None else (re + pr, im + pi)
        if re is None:
            re, im = np.zeros(B), np.zeros(B)
        tre, tim = jp * re, jp * im
        bad |= ~np.isfinite(tre) | ~np.isfinite(tim)
        q0, q1 = tre * tre, tim * tim
        q = q0 + q1
        bad |= ~np.isfinite(q)
        ap = np.where(bad, 0.0, np.sqrt(np.where(bad, 0.0, q)))
        if flags & FDG_CHAIN_INIT:
            acc = np.ones(B, dtype=bool)
        else:
            acc = np.asarray(u_acc, dtype=np.float64) * (a + gamma) < (ap + gamma)
    x, fac, a = np.where(acc, xp, x), np.where(acc, facp, fac), np.where(acc, ap, a)
    for k in live:
        root[k] = np.where(acc, np.where(bad, 0.0, rp[k]), root[k])
    n_acc = n_acc + acc.astype(np.int32)
    if flags & FDG_CHAIN_MEASURE:
        jac = fac[0].copy()
        for d in range(1, D):
            jac = jac * fac[d]
        dd = 1.0 / (a + gamma)
        ph = phases(x, list(freq))
        for k in live:
            w = (jac * root[k]) * dd
            s, c = ph[pairs[k]]
            for f in range(F):
                o = 2 * (f * R + k)
                total[o] = total[o] + w * c[:, f]
                total[o + 1] = total[o + 1] + w * s[:, f]
        total[2 * F * R] = total[2 * F * R] + dd
    return {"x": x, "fac": fac, "root": root, "a": a, "sum": total, "n_accept": n_acc, "xp": xp, "facp": facp, "accept": acc}


def make_chain_groups(root_group, var_sets, reweight=None):
    """``(fdg_chain_groups struct, keepalive)``: ``root_group`` the group of every root, ``var_sets[g]`` the variables of group ``g``
    (an empty set is allowed), ``reweight`` one factor per group or None (no factor is applied).  Host sequences."""
    rg = np.ascontiguousarray(root_group, dtype=np.uint32)
    vm = var_masks(var_sets)
    rw = None if reweight is None else np.ascontiguousarray(reweight, dtype=np.float64)
    if rg.ndim != 1 or vm.shape[0] < 1 or (rw is not None and rw.shape != vm.shape):
        raise ValueError("root_group is a vector, there is at least one group, and reweight holds one factor per group")
    return ChainGroups(vm.shape[0], rg.ctypes.data, vm.ctypes.data, None if rw is None else rw.ctypes.data), (rg, vm, rw)


def chain_grouped_reference(grid, col, state, mask: int, u, u_acc, gamma: float, flags: int, eval_roots, root_group, var_sets,
                            reweight=None, coef=None, exists=None, matsubara=None, phase_table=None, proposal=None):
    """One step of the grouped chain restated in numpy (include/fdg.h, "Markov chain with weight groups and reweighting between
    orders"): fdg_chain_propose_device, then fdg_[mc_]chain_step_device_grouped, in the device's fp64 order, so that the state and the
    sums compare bit for bit.  The arguments of :func:`chain_reference` with ``root_group [R]``, ``var_sets[g]`` the variables of group
    ``g`` and ``reweight [n_group]`` or None.  ``matsubara``: None (``state["sum"]`` is ``[R + 1, B]``), or a dict of the projected
    step's descriptor -- ``freq``, ``fermionic``, ``weight_freq``, ``root_col_in``, ``root_col_out``, ``beta`` -- with
    ``state["sum"]`` ``[2 F R + 1, B]``; the phases are the library's own (fdg_matsubara_phase through
    :func:`matsubara_phase_table`, or ``phase_table`` as in :func:`chain_matsubara_reference`).  ``proposal``: None, or ``(xp, facp,
    binp)`` made elsewhere (:func:`chain_propose_polar_reference`), which the step then takes in place of its own; ``mask`` and ``u``
    are not read."""
    return _chain_grouped_step(grid, col, state, mask, u, u_acc, gamma, flags, eval_roots, root_group, var_sets, reweight, coef, exists,
                               matsubara, phase_table, None, proposal)


def chain_binned_reference(grid, col, state, mask: int, u, u_acc, gamma: float, flags: int, eval_roots, cdf, ext=None, ext_col=(),
                           move_discrete: bool = True, u_disc=None, root_group=None, var_sets=None, reweight=None, coef=None, exists=None,
                           matsubara=None, phase_table=None, proposal=None):
    """One step of the chain with a discrete variable restated in numpy (include/fdg.h, "Markov chain with a discrete external variable
    and per-bin measurement"): fdg_chain_propose_device_discrete, then fdg_[mc_]chain_step_device_binned, in the device's fp64 order,
    so that the state and the sums compare bit for bit.  These are :func:`chain_grouped_reference`'s statements, run by the same body,
    with the discrete variable's beside them; its arguments, and ``cdf [n_bin + 1]``, ``ext [n_bin, n_ext]`` / ``ext_col`` the table
    and its columns of ``x``, ``move_discrete`` whether the variable is redrawn, ``u_disc [B]`` the uniforms of the counters
    ``(sample_offset + b, n_dim)`` (read only then).  ``root_group`` and ``var_sets`` None: one group of every root and every variable
    (a NULL ``cg``).  ``state`` holds ``fac [D + 1, B]`` (row ``D``: ``1 / p_j``), ``bin [B]`` (int32) and ``sum``
    ``[n_bin R + 1, B]`` or ``[2 n_bin F R + 1, B]``; the result has ``bin`` and ``binp`` too.  ``proposal`` as in
    :func:`chain_grouped_reference` (``move_discrete`` and ``u_disc`` are then not read either)."""
    D, R = np.asarray(grid).shape[0], np.asarray(state["root"]).shape[0]
    if root_group is None and var_sets is None:
        root_group, var_sets = [0] * R, [tuple(range(D))]
    binned = dict(cdf=np.asarray(cdf, dtype=np.float64), ext=None if ext is None else np.asarray(ext, dtype=np.float64),
                  ext_col=[int(e) for e in ext_col], move=bool(move_discrete), u=u_disc)
    return _chain_grouped_step(grid, col, state, mask, u, u_acc, gamma, flags, eval_roots, root_group, var_sets, reweight, coef, exists,
                               matsubara, phase_table, binned, proposal)


def _chain_grouped_step(grid, col, state, mask, u, u_acc, gamma, flags, eval_roots, root_group, var_sets, reweight, coef, exists, matsubara,
                        phase_table, binned, proposal=None):
    """The body of :func:`chain_grouped_reference` (``binned`` None) and :func:`chain_binned_reference`: where ``binned`` is None no
    statement of the discrete variable runs.  With ``proposal`` the step's own proposal is not made."""
    if proposal is not None:
        mask = 0
        if binned is not None:
            binned = dict(binned, move=False)
    table = matsubara_phase_table if phase_table is None else phase_table
    grid = np.asarray(grid, dtype=np.float64)
    D, G = grid.shape[0], grid.shape[1] - 1
    x, fac, root, a = (np.array(state[k], dtype=np.float64) for k in ("x", "fac", "root", "a"))
    total, n_acc = np.array(state["sum"], dtype=np.float64), np.array(state["n_accept"], dtype=np.int32)
    B, R, n_group = x.shape[1], root.shape[0], len(var_sets)
    n_bin, lanes = 1, np.arange(x.shape[1])
    if binned is not None:
        cdf, n_bin = binned["cdf"], binned["cdf"].shape[0] - 1
        bins = np.array(state["bin"], dtype=np.int32)
        if fac.shape != (D + 1, B) or bins.shape != (B,):
            raise ValueError("fac must be [n_dim + 1, n_walker] and bin [n_walker]")
    cols = list(range(D)) if col is None else [int(c) for c in col]
    live = [k for k in range(R) if exists is None or exists[k]]
    members = [[k for k in live if int(root_group[k]) == g] for g in range(n_group)]
    if any(not 0 <= int(root_group[k]) < n_group for k in live) or any(not 0 <= int(d) < D for vs in var_sets for d in vs):
        raise ValueError("root_group names a group >= n_group, or a variable set a variable >= n_dim")
    mz = matsubara
    if mz is not None:
        freq, fermionic, wf, beta = list(mz["freq"]), mz["fermionic"], int(mz["weight_freq"]), float(mz["beta"])
        F = len(freq)
        pairs = {k: (int(mz["root_col_in"][k]), int(mz["root_col_out"][k])) for k in live}
        if (binned is None and total.shape != (2 * F * R + 1, B)) or not 0 <= wf < F:
            raise ValueError("sum must be [2 n_freq n_root + 1, n_walker] and weight_freq an index into freq")
    n_sum = R if mz is None else 2 * F * R                  # the columns of one bin
    if binned is not None and total.shape != (n_bin * n_sum + 1, B):
        raise ValueError("sum must be [n_bin n_root + 1, n_walker], or [2 n_bin n_freq n_root + 1, n_walker] with a projection")

    def phases(p, fs):
        return {pair: table(p[pair[1]] - p[pair[0]], beta, fs, fermionic) for pair in set(pairs.values())}

    def group_jac(f, g):
        j = None
        for d in sorted(set(int(d) for d in var_sets[g])):
            j = f[d].copy() if j is None else j * f[d]
        j = np.ones(B) if j is None else j
        return j if binned is None else j * f[D]

    xp, facp = x.copy(), fac.copy()
    for d in range(D):
        if (mask >> d) & 1:
            y = np.asarray(u, dtype=np.float64)[:, d] * np.float64(G)
            c = np.minimum(y.astype(np.int64), G - 1)
            lo = grid[d, c]
            wd = grid[d, c + 1] - lo
            xp[cols[d]] = lo + (y - c.astype(np.float64)) * wd
            facp[d] = np.float64(G) * wd
    if binned is not None:
        binp = bins.copy()
        if binned["move"]:
            ud = np.asarray(binned["u"], dtype=np.float64)
            jp = np.searchsorted(cdf[1:n_bin], ud, side="right")        # the number of interior edges <= u
            with np.errstate(all="ignore"):
                facp[D] = 1.0 / (cdf[jp + 1] - cdf[jp])
            binp = jp.astype(np.int32)
            for e, c in enumerate(binned["ext_col"]):
                xp[c] = binned["ext"][jp, e]
    if proposal is not None:
        xp, facp = (np.array(v, dtype=np.float64) for v in proposal[:2])
        if xp.shape != x.shape or facp.shape != fac.shape:
            raise ValueError("the proposal's xp and facp have the shapes of the state's x and fac")
        if binned is not None:
            binp = np.array(proposal[2], dtype=np.int32)
    with np.errstate(all="ignore"):
        rp = np.asarray(eval_roots(xp), dtype=np.float64) if live else np.zeros((R, B))
        ph = phases(xp, [freq[wf]]) if mz is not None else None
        asum, bad = None, np.zeros(B, dtype=bool)
        for g in range(n_group):
            if not members[g]:
                continue
            jg = group_jac(facp, g)
            s = re = im = None
            for k in members[g]:
                bad |= ~np.isfinite(rp[k])
                term = rp[k] if coef is None else np.float64(coef[k]) * rp[k]
                if mz is None:
                    s = term if s is None else s + term
                else:
                    sn, cs = ph[pairs[k]]
                    pr, pi = term * cs[:, 0], term * sn[:, 0]
                    re, im = (pr, pi) if re is None else (re + pr, im + pi)
            if mz is None:
                tg = jg * s
                bad |= ~np.isfinite(tg)
                ag = np.abs(tg)
            else:
                tre, tim = jg * re, jg * im
                bad |= ~np.isfinite(tre) | ~np.isfinite(tim)
                q0, q1 = tre * tre, tim * tim
                q = q0 + q1
                bad |= ~np.isfinite(q)
                ag = np.sqrt(q)
            wa = ag if reweight is None else np.float64(reweight[g]) * ag
            asum = wa if asum is None else asum + wa
        if asum is None:
            asum = np.zeros(B)
        bad |= ~np.isfinite(asum)
        ap = np.where(bad, 0.0, asum)
        if flags & FDG_CHAIN_INIT:
            acc = np.ones(B, dtype=bool)
        else:
            acc = np.asarray(u_acc, dtype=np.float64) * (a + gamma) < (ap + gamma)
    x, fac, a = np.where(acc, xp, x), np.where(acc, facp, fac), np.where(acc, ap, a)
    for k in live:
        root[k] = np.where(acc, np.where(bad, 0.0, rp[k]), root[k])
    n_acc = n_acc + acc.astype(np.int32)
    base = 0                                                 # the first column of the walker's bin: per walker with a discrete variable
    if binned is not None:
        bins = np.where(acc, binp, bins)
        base = bins.astype(np.int64) * n_sum
    if flags & FDG_CHAIN_MEASURE:
        dd = 1.0 / (a + gamma)
        ph = phases(x, freq) if mz is not None else None
        for g in range(n_group):
            if not members[g]:
                continue
            jac = group_jac(fac, g)
            for k in members[g]:
                w = (jac * root[k]) * dd
                if mz is None:
                    total[base + k, lanes] = total[base + k, lanes] + w
                    continue
                sn, cs = ph[pairs[k]]
                for f in range(F):
                    o = base + 2 * (f * R + k)
                    total[o, lanes] = total[o, lanes] + w * cs[:, f]
                    total[o + 1, lanes] = total[o + 1, lanes] + w * sn[:, f]
        last = n_bin * n_sum
        total[last] = total[last] + dd
    out = {"x": x, "fac": fac, "root": root, "a": a, "sum": total, "n_accept": n_acc, "xp": xp, "facp": facp, "accept": acc}
    if binned is not None:
        out.update(bin=bins, binp=binp)
    return out


def _strat_array(strat, n_dim: int) -> np.ndarray:
    sv = np.ascontiguousarray(strat, dtype=np.uint32)
    if sv.shape != (n_dim,):
        raise ValueError("strat must hold one count per variable")
    return sv


def vegas_sample_device_strat(d_grid: int, n_dim: int, n_grid: int, col, strat, d_start: int, seed: int, sample_offset: int, d_x: int,
                              xs: int, xc: int, d_jac: int, d_cube: int, d_cell: int, B: int, stream: int = 0):
    """fdg_vegas_sample_device_strat: :func:`vegas_sample_device` inside the strata of the sample's hypercube.  ``strat``: host sequence
    of ``n_dim`` counts; ``d_start``: device int64 ``[H + 1]`` prefix sums of the samples per hypercube (global indices);
    ``d_cube[b]`` (int32) receives the hypercube, and ``jac`` carries ``n_total / (H n_h)``."""
    c = _col_arg(col, n_dim)
    sv = _strat_array(strat, n_dim)
    check(lib().fdg_vegas_sample_device_strat(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, sv.ctypes.data,
                                              d_start or None, seed, sample_offset, d_x or None, xs, xc, d_jac or None, d_cube or None,
                                              d_cell or None, B, stream))


def strat_allocate(cube_sum, cube_sum2, col: int, start_old, H: int, n_total: int, beta: float = 0.75) -> np.ndarray:
    """fdg_strat_allocate: the prefix sums ``start_new [H + 1]`` (int64) of the next iteration's samples per hypercube, from column
    ``col`` of the per-hypercube moments ``[H, ld]`` of an iteration drawn with ``start_old`` (None: no history, the uniform
    allocation; the moments are then not read).  Every hypercube receives at least two samples."""
    out = np.zeros(int(H) + 1, dtype=np.int64)
    if start_old is None:
        check(lib().fdg_strat_allocate(None, None, 0, 0, None, H, n_total, float(beta), out.ctypes.data))
        return out
    s1 = np.ascontiguousarray(cube_sum, dtype=np.float64)
    s2 = np.ascontiguousarray(cube_sum2, dtype=np.float64)
    so = np.ascontiguousarray(start_old, dtype=np.int64)
    if s1.ndim != 2 or s1.shape != s2.shape or s1.shape[0] != H or so.shape != (H + 1,):
        raise ValueError("the moments must be [H, ld] and start_old [H + 1]")
    check(lib().fdg_strat_allocate(s1.ctypes.data, s2.ctypes.data, s1.shape[1], col, so.ctypes.data, H, n_total, float(beta), out.ctypes.data))
    return out


def strat_allocate_reference(cube_sum, cube_sum2, col: int, start_old, H: int, n_total: int, beta: float = 0.75) -> np.ndarray:
    """Steps 1-5 of fdg_strat_allocate (include/fdg.h) restated in Python, valid arguments taken for granted: the same fp64
    operations in the same order (``math.pow`` is the C library's ``pow``), so the result is the library's exactly."""
    return strat_allocate_cols_reference(cube_sum, cube_sum2, [col], start_old, H, n_total, beta)


def strat_allocate_cols(cube_sum, cube_sum2, cols, start_old, H: int, n_total: int, beta: float = 0.75) -> np.ndarray:
    """fdg_strat_allocate_cols: :func:`strat_allocate` from the columns ``cols`` (a sequence, in the order their variances are
    folded) of the per-hypercube moments ``[H, ld]``."""
    out = np.zeros(int(H) + 1, dtype=np.int64)
    cv = np.ascontiguousarray(cols, dtype=np.uint32)
    if cv.ndim != 1:
        raise ValueError("cols must be a sequence of column numbers")
    d_cols = cv.ctypes.data if cv.shape[0] else None
    if start_old is None:
        check(lib().fdg_strat_allocate_cols(None, None, 0, d_cols, cv.shape[0], None, H, n_total, float(beta), out.ctypes.data))
        return out
    s1 = np.ascontiguousarray(cube_sum, dtype=np.float64)
    s2 = np.ascontiguousarray(cube_sum2, dtype=np.float64)
    so = np.ascontiguousarray(start_old, dtype=np.int64)
    if s1.ndim != 2 or s1.shape != s2.shape or s1.shape[0] != H or so.shape != (H + 1,):
        raise ValueError("the moments must be [H, ld] and start_old [H + 1]")
    check(lib().fdg_strat_allocate_cols(s1.ctypes.data, s2.ctypes.data, s1.shape[1], d_cols, cv.shape[0], so.ctypes.data, H, n_total,
                                        float(beta), out.ctypes.data))
    return out


def strat_allocate_cols_reference(cube_sum, cube_sum2, cols, start_old, H: int, n_total: int, beta: float = 0.75) -> np.ndarray:
    """Steps 1-5 of fdg_strat_allocate_cols (include/fdg.h) restated in Python, valid arguments taken for granted: step 1's ``var_h``
    is the left fold over ``cols`` of each column's own; the same fp64 operations in the same order, so the result is the library's
    exactly."""
    H = int(H)
    if start_old is None:
        return _strat_allocate_from_var([0.0] * H, None, H, int(n_total), beta)
    so = np.asarray(start_old, dtype=np.int64)
    n_old = float(so[H])
    var = [0.0] * H
    for h in range(H):
        nd = float(so[h + 1] - so[h])
        fac = n_old / (float(H) * nd)
        for i, col in enumerate(cols):
            s1, s2 = float(cube_sum[h][col]), float(cube_sum2[h][col])
            vc = max(0.0, (s2 - s1 * s1 / nd) / (nd - 1.0)) / (fac * fac)
            var[h] = var[h] + vc if i else vc
    return _strat_allocate_from_var(var, so, H, int(n_total), beta)


def _strat_allocate_from_var(var, so, H: int, n_total: int, beta: float) -> np.ndarray:
    """Steps 2-5 of fdg_strat_allocate from the ``var_h`` of step 1, in the library's order (``math.pow`` is the C library's
    ``pow``); ``so`` None: no history."""
    import math
    spare = n_total - 2 * H
    dh, S = [0.0] * H, 0.0
    for h in range(H):
        dh[h] = 0.0 if var[h] == 0.0 else math.pow(var[h], beta / 2.0)
        S = S + dh[h] if h else dh[h]
    if so is None or not S > 0.0 or not math.isfinite(S) or beta == 0.0:
        cnt = [2 + spare // H] * H
    else:
        cnt = [2 + int(math.floor(float(spare) * (dh[h] / S))) for h in range(H)]
    have, h = sum(cnt), 0
    while have < n_total:
        cnt[h] += 1
        have += 1
        h = (h + 1) % H
    h = H
    while have > n_total:
        h = h - 1 if h else H - 1
        if cnt[h] > 2:
            cnt[h] -= 1
            have -= 1
    return np.concatenate([[0], np.cumsum(np.array(cnt, dtype=np.int64))]).astype(np.int64)


def strat_reference(grid, strat, start, u, sample_offset: int = 0, roots=None, weight=None, coef=None, exists=None, beta=None):
    """The stratified calls restated in numpy (include/fdg.h, "Adaptive stratified sampling"), in the device's fp64 order, so that the
    sampler compares bit for bit.  ``grid [D, G + 1]`` the map, ``strat [D]``, ``start [H + 1]`` the prefix sums in global indices,
    ``u [B, D]`` the uniforms of the counters ``(sample_offset + b, d)``.  Returns a dict: ``cube [B]``, ``x [B, D]``, ``jac [B]``,
    ``cell [B, D]``; with ``roots [B, R]`` also ``cube_sum`` / ``cube_sum2 [H, R + 1]`` of ``t_k = weight * root_k`` (``weight``
    None: the roots themselves) and, in column ``R``, of ``weight * (left fold of coef_k * root_k over the roots that exist)``
    (``exists``: bool per root, None: all) -- plain numpy sums, so these compare within rounding; with ``beta`` also ``start_new``,
    :func:`strat_allocate_reference` of column ``R``."""
    grid = np.asarray(grid, dtype=np.float64)
    sv = np.asarray(strat, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    B, D = u.shape
    G, H = grid.shape[1] - 1, int(np.prod(sv))
    i = np.int64(sample_offset) + np.arange(B, dtype=np.int64)
    cube = np.clip(np.searchsorted(start, i, side="right") - 1, 0, H - 1)
    n_h = (start[cube + 1] - start[cube]).astype(np.float64)
    rem = cube.copy()
    x, cell = np.empty((B, D)), np.empty((B, D), dtype=np.int64)
    jac = None
    for d in range(D):
        s_d = rem % sv[d]
        rem = rem // sv[d]
        v = (s_d.astype(np.float64) + u[:, d]) / np.float64(sv[d])
        y = v * np.float64(G)
        c = np.minimum(y.astype(np.int64), G - 1)
        lo = grid[d, c]
        wd = grid[d, c + 1] - lo
        x[:, d] = lo + (y - c.astype(np.float64)) * wd
        f = np.float64(G) * wd
        jac = f if jac is None else jac * f
        cell[:, d] = c
    jac = jac * (np.float64(start[H]) / (np.float64(H) * n_h))
    out = {"cube": cube.astype(np.int32), "x": x, "jac": jac, "cell": cell}
    if roots is not None:
        roots = np.asarray(roots, dtype=np.float64)
        R = roots.shape[1]
        live = [k for k in range(R) if exists is None or exists[k]]
        s1, s2 = np.zeros((H, R + 1)), np.zeros((H, R + 1))
        comb = None
        for k in live:
            term = roots[:, k] if coef is None else coef[k] * roots[:, k]
            comb = term if comb is None else comb + term
            t = roots[:, k] if weight is None else weight * roots[:, k]
            s1[:, k] = np.bincount(cube, weights=t, minlength=H)
            s2[:, k] = np.bincount(cube, weights=t * t, minlength=H)
        if comb is not None:
            t = comb if weight is None else weight * comb
            s1[:, R] = np.bincount(cube, weights=t, minlength=H)
            s2[:, R] = np.bincount(cube, weights=t * t, minlength=H)
        out["cube_sum"], out["cube_sum2"] = s1, s2
        if beta is not None:
            out["start_new"] = strat_allocate_reference(s1, s2, R, start, H, int(start[H]), beta)
    return out


def vegas_sample_device_strat_grouped(d_grid: int, n_dim: int, n_grid: int, col, polar, var_sets, jac_group_stride: int, strat, d_start: int,
                                      seed: int, sample_offset: int, d_x: int, xs: int, xc: int, d_jac: int, d_cube: int, d_cell: int, B: int,
                                      stream: int = 0):
    """fdg_vegas_sample_device_strat_grouped: :func:`vegas_sample_device_grouped` without a discrete variable, every variable drawn
    inside the stratum of the sample's hypercube (``strat``, ``d_start``, ``d_cube`` as :func:`vegas_sample_device_strat` takes them)
    and every group's jacobian times ``n_total / (H n_h)``.  ``var_sets`` None: one jacobian ``jac[b]``, the full fold (polar without
    groups)."""
    c = _col_arg(col, n_dim, none_ok=True)
    arr, n_polar = _polar_array(polar)
    vm = None
    if var_sets is not None:
        vm = var_sets if isinstance(var_sets, np.ndarray) and var_sets.dtype == np.uint64 else var_masks(var_sets)
        vm = np.ascontiguousarray(vm)
    sv = _strat_array(strat, n_dim)
    check(lib().fdg_vegas_sample_device_strat_grouped(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data,
                                                      C.addressof(arr) if n_polar else None, n_polar,
                                                      vm.ctypes.data if vm is not None and vm.shape[0] else None,
                                                      0 if vm is None else vm.shape[0], jac_group_stride, sv.ctypes.data, d_start or None,
                                                      seed, sample_offset, d_x or None, xs, xc, d_jac or None, d_cube or None,
                                                      d_cell or None, B, stream))


def strat_grouped_reference(grid, strat, start, u, col, polar=(), var_sets=None, n_col=None, sample_offset: int = 0, fill: float = 0.0,
                            roots=None, weight=None, coef=None, exists=None, root_group=None):
    """The stratified grouped calls restated in numpy (include/fdg.h), composed of :func:`strat_reference` (the hypercubes, the
    drawn values, the cells, the full fold times ``fac_h``), :func:`grouped_jacobian` (the per-group folds) and the polar sampler's
    Cartesian statements with :func:`sincos`; one numpy operation per rounded operation of the kernel and in its order, so the
    sampler compares bit for bit.  ``col[d]``: the column of variable ``d`` (None for a grouped one), ``polar``: ``(var, cols)``
    pairs, ``var_sets``: the weight groups' sets of variables (None: one jacobian).  Returns a dict: ``cube [B]``, ``cell [B, D]``,
    ``value [B, D]`` (the drawn variables), ``x [B, n_col]`` (the columns as the device writes them, ``fill`` elsewhere), ``jac``
    (``[n_group, B]``, or ``[B]`` without groups); with ``roots [B, R]``, ``weight [n_group, B]`` and ``root_group [R]`` also
    ``cube_sum`` / ``cube_sum2 [H, R + n_group]`` -- plain numpy sums, so these compare within rounding."""
    grid = np.asarray(grid, dtype=np.float64)
    start = np.asarray(start, dtype=np.int64)
    base = strat_reference(grid, strat, start, u, sample_offset)
    v, cell, cube = base["x"], base["cell"], base["cube"].astype(np.int64)
    B, D = v.shape
    G, H = grid.shape[1] - 1, int(np.prod(np.asarray(strat, dtype=np.int64)))
    d_idx = np.arange(D)[None, :]
    factor = np.float64(G) * (grid[d_idx, cell + 1] - grid[d_idx, cell])
    fac_h = np.float64(start[H]) / (np.float64(H) * (start[cube + 1] - start[cube]).astype(np.float64))
    polar = [(int(var), tuple(int(c) for c in cols)) for var, cols in polar]
    if var_sets is None:
        jac = grouped_jacobian(factor, [range(D)], polar, value=v)[0] * fac_h
    else:
        jac = grouped_jacobian(factor, var_sets, polar, value=v) * fac_h[None, :]
    grouped = {d for var, cols in polar for d in range(var, var + len(cols))}
    if n_col is None:
        n_col = 1 + max([c for d, c in enumerate(col) if d not in grouped] + [c for _, cols in polar for c in cols])
    x = np.full((B, n_col), fill)
    for d in range(D):
        if d not in grouped:
            x[:, col[d]] = v[:, d]
    sc = np.frompyfunc(sincos, 1, 2)
    for var, cols in polar:
        k = v[:, var]
        if len(cols) == 3:
            st, ct = (a.astype(np.float64) for a in sc(v[:, var + 1]))
            sp, cp = (a.astype(np.float64) for a in sc(v[:, var + 2]))
            ks = k * st
            x[:, cols[0]], x[:, cols[1]], x[:, cols[2]] = ks * cp, ks * sp, k * ct
        else:
            sp, cp = (a.astype(np.float64) for a in sc(v[:, var + 1]))
            x[:, cols[0]], x[:, cols[1]] = k * cp, k * sp
    out = {"cube": base["cube"], "cell": cell, "value": v, "x": x, "jac": jac}
    if roots is not None:
        roots = np.asarray(roots, dtype=np.float64)
        R = roots.shape[1]
        w = np.asarray(weight, dtype=np.float64).reshape(-1, B)
        NG = w.shape[0]
        rg = np.zeros(R, dtype=np.int64) if root_group is None else np.asarray(root_group, dtype=np.int64)
        inside = (cube >= 0) & (cube < H)
        hc = cube[inside]
        s1, s2 = np.zeros((H, R + NG)), np.zeros((H, R + NG))
        comb = [None] * NG
        for k in range(R):
            if exists is not None and not exists[k]:
                continue
            g = int(rg[k])
            term = roots[:, k] if coef is None else coef[k] * roots[:, k]
            comb[g] = term if comb[g] is None else comb[g] + term
            t = (w[g] * roots[:, k])[inside]
            s1[:, k] = np.bincount(hc, weights=t, minlength=H)
            s2[:, k] = np.bincount(hc, weights=t * t, minlength=H)
        for g in range(NG):
            if comb[g] is not None:
                t = (w[g] * comb[g])[inside]
                s1[:, R + g] = np.bincount(hc, weights=t, minlength=H)
                s2[:, R + g] = np.bincount(hc, weights=t * t, minlength=H)
        out["cube_sum"], out["cube_sum2"] = s1, s2
    return out


def vegas_sample_device_discrete(d_grid: int, n_dim: int, n_grid: int, col, d_cdf: int, n_bin: int, bin_base: int, d_ext: int, ext_col,
                                 seed: int, sample_offset: int, d_x: int, xs: int, xc: int, d_jac: int, d_bin: int, d_cell: int, B: int,
                                 stream: int = 0):
    """fdg_vegas_sample_device_discrete: :func:`vegas_sample_device` plus one discrete variable drawn by ``d_cdf`` (device,
    ``n_bin + 1`` doubles): ``bin[b] = j + bin_base``, ``jac[b]`` divided by the value's probability, row ``j`` of ``d_ext`` (device,
    ``[n_bin, len(ext_col)]``) copied into the columns ``ext_col`` (host sequence; empty or None with ``d_ext`` 0: no table)."""
    c = _col_arg(col, n_dim)
    e = _ext_col_arg(ext_col)
    check(lib().fdg_vegas_sample_device_discrete(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, d_cdf or None, n_bin,
                                                 bin_base, d_ext or None, e.shape[0], e.ctypes.data if e.shape[0] else None, seed,
                                                 sample_offset, d_x or None, xs, xc, d_jac or None, d_bin or None, d_cell or None, B, stream))


class VegasPolar(C.Structure):
    """fdg_vegas_polar: the variables ``var .. var + dim - 1`` are (k, phi) or (k, theta, phi); the components go to ``col[0 .. dim)``"""
    _fields_ = [("var", C.c_uint32), ("dim", C.c_uint32), ("col", C.c_uint32 * 3)]


def vegas_sample_device_polar(d_grid: int, n_dim: int, n_grid: int, col, d_cdf: int, n_bin: int, bin_base: int, d_ext: int, ext_col, polar,
                              seed: int, sample_offset: int, d_x: int, xs: int, xc: int, d_jac: int, d_bin: int, d_cell: int, B: int,
                              stream: int = 0):
    """fdg_vegas_sample_device_polar: :func:`vegas_sample_device_discrete` (``d_cdf`` 0: :func:`vegas_sample_device`; the discrete
    variable's arguments are then ignored) with groups of variables read as a modulus and a direction.  ``polar``: a sequence of
    ``(var, cols)`` with ``len(cols)`` 2 -- variables ``var, var + 1`` are (k, phi) -- or 3 -- ``var .. var + 2`` are (k, theta, phi) --;
    the Cartesian components go to the columns ``cols``.  ``col`` names a column per variable; the entry of a grouped variable is not
    read (None stands for 0 there)."""
    c = _col_arg(col, n_dim, none_ok=True)
    e = _ext_col_arg(ext_col)
    arr, n_polar = _polar_array(polar)
    check(lib().fdg_vegas_sample_device_polar(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, d_cdf or None, n_bin,
                                              bin_base, d_ext or None, e.shape[0], e.ctypes.data if e.shape[0] else None,
                                              C.addressof(arr) if n_polar else None, n_polar, seed, sample_offset, d_x or None, xs, xc,
                                              d_jac or None, d_bin or None, d_cell or None, B, stream))


def _polar_array(polar):
    groups = [] if polar is None else list(polar)
    arr = (VegasPolar * max(len(groups), 1))()
    for g, (var, cols) in enumerate(groups):
        cols = [int(v) for v in cols]
        if len(cols) not in (2, 3):
            raise ValueError("a polar group has 2 or 3 columns")
        arr[g].var, arr[g].dim = int(var), len(cols)
        for i, v in enumerate(cols):
            arr[g].col[i] = v
    return arr, len(groups)


def var_masks(var_sets) -> np.ndarray:
    """The ``var_mask`` words of ``fdg_weight_groups``: one uint64 per group, bit ``d`` set for every variable ``d`` of the group's set."""
    out = np.zeros(len(var_sets), dtype=np.uint64)
    for g, vs in enumerate(var_sets):
        for d in vs:
            if not 0 <= int(d) < FDG_VEGAS_DIM_MAX:
                raise ValueError(f"a variable must lie in [0, {FDG_VEGAS_DIM_MAX})")
            out[g] |= np.uint64(1) << np.uint64(int(d))
    return out


def make_weight_groups(root_group, var_sets, stride: int = 0):
    """``(fdg_weight_groups struct, keepalive)``: ``root_group`` the group of every root, ``var_sets[g]`` the VEGAS variables of group
    ``g`` (host sequences); ``stride`` the distance in doubles between the groups' weight columns."""
    rg = np.ascontiguousarray(root_group, dtype=np.uint32)
    vm = var_masks(var_sets)
    if rg.ndim != 1 or vm.shape[0] < 1:
        raise ValueError("root_group is a vector and there is at least one group")
    return WeightGroups(vm.shape[0], rg.ctypes.data, vm.ctypes.data, int(stride)), (rg, vm)


def make_observables(coef, d_obs: int, d_cov: int):
    """``(fdg_observables struct, keepalive)``: ``coef`` the ``[n_obs, n_root]`` coefficients (host), ``d_obs`` / ``d_cov`` the device
    addresses of the ``[n_bin, n_obs]`` and ``[n_bin, n_obs, n_obs]`` sums.  The struct points into the keepalive array."""
    c = np.ascontiguousarray(coef, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError("coef must be [n_obs, n_root]")
    return Observables(c.shape[0], c.ctypes.data, d_obs or None, d_cov or None), (c,)


def observables_reference(roots, coef, weight=None, root_group=None, bins=None, n_bin: int = 1, bin_base: int = 0, exists=None):
    """The numpy restatement of fdg_[mc_]accumulate_device_observables' definition: ``(obs [n_bin, n_obs], cov [n_bin, n_obs, n_obs],
    scale_obs, scale_cov)`` from ``roots [B, R]``, ``coef [n_obs, R]``, ``weight`` None, ``[B]`` or ``[n_group, B]`` with
    ``root_group [R]``, ``bins [B]`` or None (every sample in bin 0) and ``exists [R]`` (None: every root exists).  ``t_k = w_g(k) *
    root_k``; ``o_m`` the left fold of ``coef[m, k] * t_k`` over ascending ``k`` with ``coef[m, k] != 0`` among the roots that exist,
    the first product starting the fold; the samples of a bin are summed by numpy.  A row without a term leaves nan in its column of
    ``obs`` and its rows and columns of ``cov`` (the call leaves them untouched).  ``scale_*``: the sums of ``|o_m|`` and
    ``|o_a o_c|``, what a tolerance is measured against."""
    r = np.asarray(roots, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64)
    B, R = r.shape
    M = c.shape[0]
    live = np.ones(R, bool) if exists is None else np.asarray(exists, bool)
    if weight is None:
        t = r
    else:
        w = np.asarray(weight, dtype=np.float64)
        if w.ndim == 1:
            t = w[:B, None] * r
        else:
            rg = np.zeros(R, np.int64) if root_group is None else np.asarray(root_group, np.int64)
            t = w[np.where(live, rg, 0)][:, :B].T * r
    j = np.zeros(B, np.int64) if bins is None else np.asarray(bins, np.int64)[:B] - int(bin_base)
    ok = (j >= 0) & (j < n_bin)
    o = np.zeros((B, M))
    has = np.zeros(M, bool)
    for m in range(M):
        for k in range(R):
            if live[k] and c[m, k] != 0.0:
                p = c[m, k] * t[:, k]
                o[:, m] = o[:, m] + p if has[m] else p
                has[m] = True
    obs = np.full((n_bin, M), np.nan)
    cov = np.full((n_bin, M, M), np.nan)
    s_obs, s_cov = np.zeros((n_bin, M)), np.zeros((n_bin, M, M))
    jj = j[ok]
    for m in range(M):
        if not has[m]:
            continue
        om = o[ok, m]
        obs[:, m] = np.bincount(jj, om, n_bin)
        s_obs[:, m] = np.bincount(jj, np.abs(om), n_bin)
        for m2 in range(m, M):
            if not has[m2]:
                continue
            pr = om * o[ok, m2]
            cov[:, m, m2] = cov[:, m2, m] = np.bincount(jj, pr, n_bin)
            s_cov[:, m, m2] = s_cov[:, m2, m] = np.bincount(jj, np.abs(pr), n_bin)
    return obs, cov, s_obs, s_cov


def make_freq_observables(coef, d_fobs: int, d_fcov: int):
    """``(fdg_freq_observables struct, keepalive)``: ``coef`` the real ``[n_obs, n_root]`` coefficients (host), ``d_fobs`` / ``d_fcov``
    the device addresses of the ``[n_bin, n_freq, 2 n_obs]`` and ``[n_bin, n_freq, 2 n_obs, 2 n_obs]`` sums.  The struct points into the
    keepalive array."""
    c = np.ascontiguousarray(coef, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError("coef must be [n_obs, n_root]")
    return FreqObservables(c.shape[0], c.ctypes.data, d_fobs or None, d_fcov or None), (c,)


def matsubara_phase_table(tau, beta: float, freq, fermionic: bool = True):
    """``(s, c)``, each ``[len(tau), len(freq)]``: fdg_matsubara_phase's bits for every (sample, frequency), one call of the library's
    routine per entry (about a microsecond each)."""
    tau = np.asarray(tau, dtype=np.float64)
    s, c = np.empty((tau.shape[0], len(freq))), np.empty((tau.shape[0], len(freq)))
    fn, vs, vc = lib().fdg_matsubara_phase, C.c_double(), C.c_double()
    ps, pc, beta, fm = C.byref(vs), C.byref(vc), float(beta), 1 if fermionic else 0
    taus = tau.tolist()
    for f, n in enumerate(int(v) for v in freq):
        for b, tb in enumerate(taus):
            fn(tb, beta, n, fm, ps, pc)
            s[b, f] = vs.value
            c[b, f] = vc.value
    return s, c


def freq_observables_reference(roots, T, tin, tout, freq, beta, fermionic, coef, weight=None, root_group=None, bins=None, n_bin: int = 1,
                               bin_base: int = 0, exists=None, phases=None):
    """The numpy restatement of fdg_[mc_]accumulate_device_freq_observables' definition: ``(fobs [n_bin, F, 2 M], fcov [n_bin, F, 2 M,
    2 M], scale_fobs, scale_fcov)`` from ``roots [B, R]``, ``T [B, n_tau]``, the 1-based time labels ``tin`` / ``tout`` ``[R]``, the
    frequencies ``freq [F]`` and the real ``coef [M, R]``; ``weight``, ``root_group``, ``bins`` and ``exists`` as observables_reference
    takes them.  ``t_k = w_g(k) * root_k``, ``(s, c) = fdg_matsubara_phase(T[b, tout_k] - T[b, tin_k], beta, freq[f], fermionic)``
    (the library's routine through matsubara_phase_table; ``phases``: such tables ready-made, ``{(tin, tout): (s, c)}`` over ALL
    samples), ``tre = t_k * c``, ``tim = t_k * s``; ``a_m`` / ``b_m`` the left folds of ``coef[m, k] * tre_k`` / ``* tim_k`` over
    ascending ``k`` with ``coef[m, k] != 0`` among the roots that exist, the first product starting the fold; ``z = (a, b)``; the
    samples of a bin are summed by numpy.  A row without a term leaves nan in its components ``m`` and ``M + m`` (the call leaves them
    untouched).  ``scale_*``: the sums of ``|z_p|`` and ``|z_p z_q|``, what a tolerance is measured against."""
    r = np.asarray(roots, dtype=np.float64)
    c = np.asarray(coef, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    B, R = r.shape
    M, F = c.shape[0], len(freq)
    live = np.ones(R, bool) if exists is None else np.asarray(exists, bool)
    if weight is None:
        t = r
    else:
        w = np.asarray(weight, dtype=np.float64)
        if w.ndim == 1:
            t = w[:B, None] * r
        else:
            rg = np.zeros(R, np.int64) if root_group is None else np.asarray(root_group, np.int64)
            t = w[np.where(live, rg, 0)][:, :B].T * r
    j = np.zeros(B, np.int64) if bins is None else np.asarray(bins, np.int64)[:B] - int(bin_base)
    ok = (j >= 0) & (j < n_bin)
    jj = j[ok]
    tables = {} if phases is None else phases
    z = [np.zeros((int(ok.sum()), F)) for _ in range(2 * M)]                   # one contiguous [sample, frequency] array per component
    has = np.zeros(M, bool)
    for k in range(R):
        if not live[k] or not (c[:, k] != 0.0).any():
            continue
        pair = (int(tin[k]), int(tout[k]))
        if pair not in tables:
            tau = np.where(ok, T[:B, pair[1] - 1] - T[:B, pair[0] - 1], 0.0)      # (samples out of range are not projected)
            tables[pair] = matsubara_phase_table(tau, beta, freq, fermionic)
        s, cs = (v[:B][ok] for v in tables[pair])
        tre, tim = t[ok, k, None] * cs, t[ok, k, None] * s
        for m in range(M):
            if c[m, k] != 0.0:
                pa, pb = c[m, k] * tre, c[m, k] * tim
                z[m] = z[m] + pa if has[m] else pa
                z[M + m] = z[M + m] + pb if has[m] else pb
                has[m] = True
    has2 = np.concatenate([has, has])
    fobs = np.full((n_bin, F, 2 * M), np.nan)
    fcov = np.full((n_bin, F, 2 * M, 2 * M), np.nan)
    s_obs, s_cov = np.zeros((n_bin, F, 2 * M)), np.zeros((n_bin, F, 2 * M, 2 * M))
    cell = (jj[:, None] * F + np.arange(F)[None, :]).ravel()                    # (bin, frequency) of every entry of a component

    def per_bin(v):
        return np.bincount(cell, v.ravel(), n_bin * F).reshape(n_bin, F)

    for p in range(2 * M):
        if not has2[p]:
            continue
        fobs[:, :, p] = per_bin(z[p])
        s_obs[:, :, p] = per_bin(np.abs(z[p]))
        for q in range(p, 2 * M):
            if not has2[q]:
                continue
            pr = z[p] * z[q]
            fcov[:, :, p, q] = fcov[:, :, q, p] = per_bin(pr)
            s_cov[:, :, p, q] = s_cov[:, :, q, p] = per_bin(np.abs(pr))
    return fobs, fcov, s_obs, s_cov


def vegas_sample_device_grouped(d_grid: int, n_dim: int, n_grid: int, col, d_cdf: int, n_bin: int, bin_base: int, d_ext: int, ext_col, polar,
                                var_sets, jac_group_stride: int, seed: int, sample_offset: int, d_x: int, xs: int, xc: int, d_jac: int,
                                d_bin: int, d_cell: int, B: int, stream: int = 0):
    """fdg_vegas_sample_device_grouped: :func:`vegas_sample_device_polar` with one jacobian per weight group,
    ``jac[g * jac_group_stride + b]`` the fold over the variables ``var_sets[g]`` only (``var_sets``: a sequence of sets of variables, or
    the uint64 masks themselves)."""
    c = _col_arg(col, n_dim, none_ok=True)
    e = _ext_col_arg(ext_col)
    arr, n_polar = _polar_array(polar)
    vm = var_sets if isinstance(var_sets, np.ndarray) and var_sets.dtype == np.uint64 else var_masks(var_sets)
    vm = np.ascontiguousarray(vm)
    check(lib().fdg_vegas_sample_device_grouped(d_grid or None, n_dim, n_grid, None if c is None else c.ctypes.data, d_cdf or None, n_bin,
                                                bin_base, d_ext or None, e.shape[0], e.ctypes.data if e.shape[0] else None,
                                                C.addressof(arr) if n_polar else None, n_polar, vm.ctypes.data if vm.shape[0] else None,
                                                vm.shape[0], jac_group_stride, seed, sample_offset, d_x or None, xs, xc, d_jac or None,
                                                d_bin or None, d_cell or None, B, stream))


def grouped_jacobian(factor, var_sets, polar=(), value=None, prob=None) -> np.ndarray:
    """The numpy restatement of the grouped sampler's weights, ``[n_group, B]``, one numpy operation per rounded operation of the
    kernel and in its order.  ``factor [B, D]``: ``G * wd_d`` of every sample's cell; ``polar``: ``(var, cols)`` groups, whose modulus
    and polar angle are read from ``value [B, D]`` (the drawn values; the sine through :func:`sincos`); ``prob [B]``: the probability of
    the discrete variable's value, None without one."""
    f = np.asarray(factor, dtype=np.float64)
    B, D = f.shape
    sin_of = np.frompyfunc(lambda t: sincos(t)[0], 1, 1)
    out = np.empty((len(var_sets), B))
    for g, vs in enumerate(var_sets):
        mine = {int(d) for d in vs}
        j = np.ones(B)
        for d in range(D):
            if d in mine:
                j = j * f[:, d]
        for var, cols in polar:
            if var in mine:
                k = np.asarray(value, dtype=np.float64)[:, var]
                j = j * k
                if len(cols) == 3:
                    j = j * k
                    j = j * sin_of(np.asarray(value, dtype=np.float64)[:, var + 1]).astype(np.float64)
        out[g] = j if prob is None else j / np.asarray(prob, dtype=np.float64)
    return out


def vegas_refine_discrete(cdf: np.ndarray, hist_bin: np.ndarray, alpha: float = 0.5, floor: float = 0.05) -> np.ndarray:
    """fdg_vegas_refine_discrete: moves the probabilities of the discrete variable ``cdf [n_bin + 1]`` (float64, C-contiguous, in place)
    towards ``p_j ~ (hist_bin[j] * p_j) ** alpha``, every one at least ``floor / n_bin``; returns ``cdf``."""
    if not (isinstance(cdf, np.ndarray) and cdf.dtype == np.float64 and cdf.ndim == 1 and cdf.flags.c_contiguous and cdf.shape[0] >= 2):
        raise ValueError("cdf must be a C-contiguous float64 [n_bin + 1] array")
    h = np.ascontiguousarray(hist_bin, dtype=np.float64)
    if h.shape != (cdf.shape[0] - 1,):
        raise ValueError("hist_bin must be [n_bin]")
    check(lib().fdg_vegas_refine_discrete(cdf.ctypes.data, h.ctypes.data, cdf.shape[0] - 1, float(alpha), float(floor)))
    return cdf


def vegas_refine(grid: np.ndarray, hist: np.ndarray, alpha: float = 0.5) -> np.ndarray:
    """fdg_vegas_refine: moves the edges ``grid [n_dim, n_grid + 1]`` (float64, C-contiguous, in place) towards where the training
    histogram ``hist [n_dim, n_grid]`` is large; returns ``grid``."""
    if not (isinstance(grid, np.ndarray) and grid.dtype == np.float64 and grid.ndim == 2 and grid.flags.c_contiguous and grid.shape[1] >= 2):
        raise ValueError("grid must be a C-contiguous float64 [n_dim, n_grid + 1] array")
    h = np.ascontiguousarray(hist, dtype=np.float64)
    if h.shape != (grid.shape[0], grid.shape[1] - 1):
        raise ValueError("hist must be [n_dim, n_grid]")
    check(lib().fdg_vegas_refine(grid.ctypes.data, h.ctypes.data, grid.shape[0], grid.shape[1] - 1, float(alpha)))
    return grid


def set_default_option(name: str, value=None):
    """fdg_set_default_option: the option every handle created from now on starts with (``None`` removes it); also what the entry points
    without a handle see.  The library does not look at ``os.environ`` after its first use."""
    check(lib().fdg_set_default_option(name.encode(), None if value is None else str(value).encode()))


def get_default_option(name: str):
    v = lib().fdg_get_default_option(name.encode())
    return None if v is None else v.decode()


def batch_alloc(n_bytes: int, chunk_bytes: int = 0) -> int:
    """Device address of a batch backed by physical chunks of ``chunk_bytes`` (0: one allocation); :func:`batch_free` releases it."""
    p = C.c_void_p()
    check(lib().fdg_batch_alloc(n_bytes, chunk_bytes, C.byref(p)))
    return int(p.value)


def batch_free(ptr: int):
    check(lib().fdg_batch_free(ptr))


BATCH_PAIR_CALIBRATE = 1
BATCH_PAIR_ROW_MAJOR = 8
BATCH_PAIR_LEAF_MAJOR = 16


def batch_alloc_pair(handle: "GraphHandle", n_sample: int, chunk_bytes: int = 0, calibrate: bool = True, verbose: bool = False, extra_flags: int = 0):
    """fdg_batch_alloc_pair: device addresses (leaf, root) of a tile-major batch of ``handle`` whose root chunks were chosen by timing the
    handle's evaluator on (leaf chunk, root chunk) pairs, and the report as a dict.  Release both with :func:`batch_free`."""
    pl, pr, info = C.c_void_p(), C.c_void_p(), BatchPairInfo()
    check(lib().fdg_batch_alloc_pair(handle.ptr, n_sample, chunk_bytes, (BATCH_PAIR_CALIBRATE if calibrate else 0) | (2 if verbose else 0) | extra_flags, C.byref(pl), C.byref(pr), C.byref(info)))
    return int(pl.value), int(pr.value), {k: getattr(info, k) for k, _ in BatchPairInfo._fields_}


def isa_check_hazards(asm_text: str):
    """(number of violations, report) of a gfx950 listing against the emitter's wait-state table."""
    rep = C.c_char_p()
    n = lib().fdg_isa_check_hazards(asm_text.encode(), C.byref(rep))
    try:
        text = rep.value.decode() if rep.value else ""
    finally:
        lib().fdg_free(rep)
    if n < 0:
        check(n)
    return n, text


def copy_device(d_dst: int, d_src: int, n: int, stream: int = 0):
    check(lib().fdg_copy_device(d_dst, d_src, n, stream))


def repack_tile_major(d_src: int, ss: int, cs: int, d_tiled: int, n_sample: int, n_col: int, stream: int = 0):
    """fdg_repack_tile_major: matrix m[b*ss + c*cs] -> tile-major (64, n_col, cld(n_sample, 64))."""
    check(lib().fdg_repack_tile_major(d_src, ss, cs, d_tiled, n_sample, n_col, stream))


def unpack_tile_major(d_tiled: int, d_dst: int, ss: int, cs: int, n_sample: int, n_col: int, stream: int = 0):
    """fdg_unpack_tile_major: tile-major (64, n_col, cld(n_sample, 64)) -> matrix m[b*ss + c*cs]."""
    check(lib().fdg_unpack_tile_major(d_tiled, d_dst, ss, cs, n_sample, n_col, stream))


def read_device(d_src: int, n: int, d_sink: int, stream: int = 0):
    """Harness: a non-temporal read-only stream over n doubles (the memory system's ceiling for reads)."""
    check(lib().fdg_read_device(d_src, n, d_sink, stream))


def clock_probe_device(seconds: float, d_ticks: int, stream: int):
    """One sleeping wave on ``stream`` for ``seconds``; afterwards ``d_ticks[0] / d_ticks[1] * 0.1`` is the shader clock in GHz
    the chip sustained meanwhile (launch it on a side stream next to the kernels of interest)."""
    check(lib().fdg_clock_probe_device(seconds, d_ticks, stream))


def powi(x: float, n: int) -> float:
    return float(lib().fdg_powi(x, n))


def sincos(x: float):
    """fdg_sincos: ``(sin x, cos x)`` for ``0 <= x <= 2 pi`` by the routine the polar sampler uses (csrc/fdg_sincos.h)"""
    s, c = C.c_double(), C.c_double()
    lib().fdg_sincos(float(x), C.byref(s), C.byref(c))
    return s.value, c.value


def matsubara_phase(tau: float, beta: float, n: int, fermionic: bool = True):
    """``(sin, cos)`` of ``omega_n * tau`` by the routine the projection pass uses (fdg_matsubara_phase): the same bits on host and device."""
    s, c = C.c_double(), C.c_double()
    lib().fdg_matsubara_phase(tau, beta, int(n), 1 if fermionic else 0, C.byref(s), C.byref(c))
    return s.value, c.value


def make_matsubara(freq, fermionic, root_tau_in, root_tau_out, beta, n_tau, d_acc_re, d_acc_im, d_acc2_re, d_acc2_im, d_T=0, ts=0, tc=0):
    """``(fdg_matsubara struct, keepalive)``: ``freq`` the n of every frequency, ``root_tau_in`` / ``root_tau_out`` 1-based per root (host
    sequences); the four outputs and ``d_T`` device addresses (``d_T`` 0 in the Monte-Carlo form: the call's own T)."""
    a = [np.ascontiguousarray(v, dtype=np.int32) for v in (freq, root_tau_in, root_tau_out)]
    m = Matsubara(a[0].shape[0], 1 if fermionic else 0, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, float(beta), d_T or None,
                  int(ts), int(tc), int(n_tau), d_acc_re or None, d_acc_im or None, d_acc2_re or None, d_acc2_im or None)
    return m, a


class Comm:
    """One RCCL communicator per process/GPU for the single reduction of the observable (fdg.h, multi-GPU).
    ``Comm.unique_id()`` on rank 0, ship the 128 bytes to the other ranks, ``Comm(id, rank, world)`` everywhere
    (with the rank's device current), then ``reduce(d_acc_ptr, n)``."""

    def __init__(self, unique_id: bytes, rank: int, world: int):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % COMM_ID_BYTES)
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        check(lib().fdg_comm_create(buf, rank, world, C.byref(h)))
        self._h, self.rank, self.world = h, rank, world

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        check(lib().fdg_comm_unique_id(buf, COMM_ID_BYTES))
        return buf.raw

    def reduce(self, d_acc: int, n: int, root: int = -1, stream: int = 0):
        check(lib().fdg_reduce_device(self._h, d_acc, n, root, stream))

    def close(self):
        if self._h:
            lib().fdg_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_leaf_tables(leaf_type, leaf_order, tau_in, tau_out, loop_index, basis, dim, n_tau, kF=0.0, beta=0.0, lam=0.0):
    """``fdg_leaf_tables`` from the vectors of ``FrontEnds.leafstates`` (1-based indices); returns the
    struct and the arrays it points into (keep them alive)."""
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (leaf_type, leaf_order, tau_in, tau_out, loop_index)]
    bs = np.ascontiguousarray(basis, dtype=np.float64)
    t = LeafTables()
    t.n_leaf, t.n_basis, t.n_loop, t.dim, t.n_tau = a[0].shape[0], bs.shape[0], bs.shape[1], dim, n_tau
    t.leaf_type, t.leaf_order, t.tau_in, t.tau_out, t.loop_index = [x.ctypes.data for x in a]
    t.basis = bs.ctypes.data
    t.kF, t.beta, t.lambda_ = kF, beta, lam
    return t, (a, bs)


def leaf_eval_device(leaf_type, leaf_order, tau_in, tau_out, loop_index, basis, dim, n_tau, kF, beta, lam,
                     d_K: int, ks: int, kc: int, d_T: int, ts: int, tc: int, d_leaf: int, ss: int, ls: int, B: int,
                     stream: int = 0):
    """fdg_leaf_eval_device with the tables of ``FrontEnds.leafstates`` (1-based indices)."""
    t, _keep = make_leaf_tables(leaf_type, leaf_order, tau_in, tau_out, loop_index, basis, dim, n_tau, kF, beta, lam)
    check(lib().fdg_leaf_eval_device(C.byref(t), d_K, ks, kc, d_T, ts, tc, d_leaf, ss, ls, B, stream))


def leaf_eval_device_tiled(leaf_type, leaf_order, tau_in, tau_out, loop_index, basis, dim, n_tau, kF, beta, lam,
                           d_K: int, ks: int, kc: int, d_T: int, ts: int, tc: int, d_leaf: int, ss: int, ls: int, lts: int, B: int,
                           stream: int = 0):
    """fdg_leaf_eval_device_tiled: the leaves of a tile-major batch (sample b of leaf i at ``(b // 64) * lts + (b % 64) * ss + i * ls``)."""
    t, _keep = make_leaf_tables(leaf_type, leaf_order, tau_in, tau_out, loop_index, basis, dim, n_tau, kF, beta, lam)
    check(lib().fdg_leaf_eval_device_tiled(C.byref(t), d_K, ks, kc, d_T, ts, tc, d_leaf, ss, ls, lts, B, stream))
