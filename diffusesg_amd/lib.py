"""ctypes binding of libdsg.so (include/dsg.h, and include/dsg_debug.h for the test bench).  There is NO fallback: if the HIP library is
missing or no GPU is visible, construction fails loudly."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdsg.so")
MAX_LAYERS = 8

# every symbol include/dsg.h declares (tests/test_abi.py holds the header to this list and the built library to both lists)
EXPORTS = [
    "dsg_create", "dsg_destroy", "dsg_last_error", "dsg_version", "dsg_abi_version", "dsg_set_weight", "dsg_finalize_weights",
    "dsg_num_weight_keys", "dsg_weight_key", "dsg_workspace_bytes", "dsg_denoise", "dsg_precond", "dsg_sample", "dsg_sigma_schedule",
    "dsg_decode_bits", "dsg_decode", "dsg_set_option", "dsg_get_option", "dsg_gen_noise", "dsg_train_inputs", "dsg_rainbow_loss",
    "dsg_rainbow_loss_backward", "dsg_noise_embed", "dsg_affine_width", "dsg_block_train", "dsg_train_grads", "dsg_train_step_grads",
    "dsg_train_self_cond", "dsg_train_bind_params", "dsg_adam_step", "dsg_ema_update", "dsg_eval_bbox_prep_bytes", "dsg_eval_bbox_prep",
    "dsg_eval_bbox_f1", "dsg_eval_type_hist", "dsg_eval_degree_hist", "dsg_eval_hist_mmd", "dsg_sgstat_triplet_counts", "dsg_sgstat_layout",
    "dsg_sgstat_f1_rowstats", "dsg_sample_known", "dsg_encode", "dsg_sample_walk", "dsg_walk_steps", "dsg_multistep_coef",
    "dsg_sample_seeded", "dsg_gen_noise_seeded", "dsg_precond_vjp", "dsg_ode_run", "dsg_ode_evals", "dsg_guide_coef", "dsg_sample_guided",
    "dsg_sample_guided_rel", "dsg_sample_guided_content", "dsg_option_info", "dsg_create_patch", "dsg_train_set_precision", "dsg_train_get_precision",
    "dsg_attach_guide", "dsg_detach_guide", "dsg_guide_info", "dsg_guide_forwards", "dsg_train_enable_patch", "dsg_train_patch_enabled",
]

TRAIN_PRECISIONS = {"fp32": 0, "bf16": 1}   # DSG_TRAIN_F32 / DSG_TRAIN_BF16 of include/dsg.h

# dsg_grad_fn of include/dsg.h (dsg_precond_vjp): int fn(void *user, const float *D_adj, const float *D_node, float *g_adj, float *g_node)
GRAD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)

DSG_ERR_INVALID = -1   # dsg_status of include/dsg.h: bad argument / unsupported configuration


class DsgError(RuntimeError):
    pass


class DsgConfig(C.Structure):
    _fields_ = [("max_node_num", C.c_int32), ("c_adj", C.c_int32), ("c_node", C.c_int32), ("embed_dim", C.c_int32),
                ("num_layers", C.c_int32), ("depths", C.c_int32 * MAX_LAYERS), ("num_heads", C.c_int32 * MAX_LAYERS),
                ("window_size", C.c_int32), ("mlp_ratio", C.c_int32), ("self_condition", C.c_int32)]


class DsgSamplerCfg(C.Structure):
    _fields_ = [("num_steps", C.c_int32), ("heun", C.c_int32),
                ("S_churn", C.c_float), ("S_min", C.c_float), ("S_max", C.c_float), ("S_noise", C.c_float),
                ("sigma_min", C.c_double), ("sigma_max", C.c_double), ("rho", C.c_double),
                ("use_graph", C.c_int32), ("reserved", C.c_int32)]


class DsgSampleStats(C.Structure):
    _fields_ = [("precond_calls", C.c_int64), ("net_forwards", C.c_int64), ("graph_replays", C.c_int64)]


class DsgWalkCfg(C.Structure):
    _fields_ = [("start_step", C.c_int32), ("jump_len", C.c_int32), ("n_resample", C.c_int32),
                ("resample_lo", C.c_int32), ("resample_hi", C.c_int32), ("reserved", C.c_int32 * 3)]


class DsgOdeCfg(C.Structure):
    """dsg_ode_cfg of include/dsg.h (dsg_ode_run, dsg_ode_evals)"""
    _fields_ = [("direction", C.c_int32), ("probe", C.c_int32), ("reserved", C.c_int32 * 6)]


class DsgGuideCfg(C.Structure):
    """dsg_guide_cfg of include/dsg.h (dsg_sample_guided, dsg_debug_box_guide): sel / region device pointers, weights a host pointer"""
    _fields_ = [("w_overlap", C.c_float), ("w_region", C.c_float), ("w_align", C.c_float), ("tau", C.c_float), ("clip_ratio", C.c_float),
                ("reserved", C.c_int32), ("sel", C.c_void_p), ("region", C.c_void_p), ("weights", C.c_void_p)]


GUIDE_CLIP_NONE = float("inf")   # DSG_GUIDE_CLIP_NONE: unclipped, no norm pass


class DsgRelCfg(C.Structure):
    """dsg_rel_cfg of include/dsg.h (dsg_sample_guided_rel, dsg_debug_box_guide_rel): kinds a device pointer, pred_kind a host pointer"""
    _fields_ = [("w_rel", C.c_float), ("margin", C.c_float), ("source", C.c_int32), ("encoding", C.c_int32), ("n_adj_type", C.c_int32),
                ("reserved", C.c_int32), ("kinds", C.c_void_p), ("pred_kind", C.c_void_p)]


class DsgContentCfg(C.Structure):
    """dsg_content_cfg of include/dsg.h (dsg_sample_guided_content, dsg_debug_content_guide): subj / obj / pred / w_spo host pointers"""
    _fields_ = [("w_content", C.c_float), ("tau", C.c_float), ("clip_ratio", C.c_float), ("n_items", C.c_int32), ("node_chans", C.c_int32),
                ("reserved", C.c_int32), ("subj", C.c_void_p), ("obj", C.c_void_p), ("pred", C.c_void_p), ("w_spo", C.c_void_p)]


CONTENT_MAX_ITEMS = 16   # DSG_CONTENT_MAX_ITEMS

REL_GIVEN, REL_DECODED = 0, 1                                  # DSG_REL_GIVEN / DSG_REL_DECODED
REL_NONE, REL_LEFT_OF, REL_RIGHT_OF, REL_ABOVE, REL_BELOW, REL_INSIDE, REL_CONTAINS, REL_ON = range(8)   # DSG_REL_* kinds

ODE_ENCODE, ODE_DECODE = 0, 1                                  # DSG_ODE_ENCODE / DSG_ODE_DECODE
ODE_PROBES = {"none": 0, "rademacher": 1, "gaussian": 2}       # DSG_ODE_PROBE_*
ODE_PROBE_STREAM = 0x0DE00000                                  # DSG_ODE_PROBE_STREAM: the noise stream of the device-drawn probe


WALK_MAX_STEPS = 1 << 20   # DSG_WALK_MAX_STEPS


# ---- the test bench: include/dsg_debug.h (every dsg_debug_* / dsg_profile_* entry of the same library, its structs and selectors) ----
DEBUG_EXPORTS = [
    "dsg_debug_tap", "dsg_debug_clear_taps", "dsg_profile_forward", "dsg_debug_gemm", "dsg_debug_gemm_f32", "dsg_debug_gemm_form",
    "dsg_debug_qkv_attn_f32", "dsg_debug_window_attn_f32", "dsg_debug_fused_mlp_f32", "dsg_debug_fused_attn96_f32", "dsg_debug_t_gemm",
    "dsg_debug_t_attn", "dsg_debug_t_ln", "dsg_debug_t_modulate", "dsg_debug_t_colsum", "dsg_debug_t_grouped", "dsg_debug_gemm_bx",
    "dsg_debug_attn_bx", "dsg_debug_qkv_attn_bx", "dsg_debug_projmlp_bx", "dsg_debug_mlp_bx", "dsg_profile_clock_ghz",
    "dsg_debug_need_lists", "dsg_debug_dedup_lists", "dsg_debug_dedup_level_lists", "dsg_debug_dedup_launch_lists",
    "dsg_debug_dedup_qkv_lists", "dsg_debug_qk_split", "dsg_debug_readout_tiles", "dsg_debug_t_assemble_bwd", "dsg_debug_patch_embed_f32",
    "dsg_debug_assemble_f32", "dsg_debug_readout_f32", "dsg_debug_head_f32", "dsg_debug_row_f32", "dsg_debug_window_broadcast_f32",
    "dsg_debug_window_harvest_f32", "dsg_debug_graph_dot", "dsg_debug_poison", "dsg_debug_box_guide", "dsg_debug_box_guide_rel",
    "dsg_debug_content_guide",
    "dsg_debug_gemm_lp", "dsg_debug_convert", "dsg_debug_row_lp", "dsg_debug_window_attn_lp", "dsg_debug_patch_forms",
    "dsg_debug_assemble_patch_f32", "dsg_debug_head_patch_f32", "dsg_debug_patch_embed_patch_f32", "dsg_debug_readout_patch_f32",
    "dsg_debug_t_gemm_lp", "dsg_debug_t_cast_lp", "dsg_debug_train_routes", "dsg_debug_gemm_bx_args", "dsg_debug_mlp_bx_args",
    "dsg_debug_t_patch_pack", "dsg_debug_t_adj_out_patch", "dsg_debug_t_pool_bwd_patch", "dsg_debug_t_live_cols_patch",
    "dsg_debug_t_assemble_bwd_patch",
]


class DsgGemmF32Args(C.Structure):
    """dsg_gemm_f32_args of include/dsg_debug.h (dsg_debug_gemm_f32): device pointers as integers, leading dimensions in floats"""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "A2", "W", "bias", "ln_stats", "ln_part", "res", "C", "C2", "mod_aff", "stats_out",
                                           "row_list", "row_cnt")] +
                [(n, C.c_int32) for n in ("lda", "lda2", "K1", "ln_nparts", "ldres", "ldc", "ldc2", "M", "N", "K", "act", "mod_ld",
                                          "mod_off", "mod_T", "a4_res", "reserved")])


class DsgGemmLpArgs(C.Structure):
    """dsg_gemm_lp_args of include/dsg_debug.h (dsg_debug_gemm_lp): the fields of DsgGemmF32Args, the host pointer tile_used behind the device
    pointers, and mode / tile / a_bf16 / c_bf16 behind the int32 fields"""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "A2", "W", "bias", "ln_stats", "ln_part", "res", "C", "C2", "mod_aff", "stats_out",
                                           "row_list", "row_cnt", "tile_used")] +
                [(n, C.c_int32) for n in ("lda", "lda2", "K1", "ln_nparts", "ldres", "ldc", "ldc2", "M", "N", "K", "act", "mod_ld",
                                          "mod_off", "mod_T", "a4_res", "reserved", "mode", "tile", "a_bf16", "c_bf16")])


class DsgBxGemmArgs(C.Structure):
    """dsg_bx_gemm_args of include/dsg_debug.h (dsg_debug_gemm_bx_args): device pointers as integers (geo_used: a host int32), leading
    dimensions in elements of the tensor they belong to"""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "A2", "W", "bias", "res", "C", "Cb", "C2b", "mod_aff", "geo_used")] +
                [(n, C.c_int32) for n in ("lda", "lda2", "K1", "ldres", "ldc", "ldcb", "ldc2b", "M", "N", "K", "act", "mod_ld", "mod_off",
                                          "mod_T", "ln_out")])


class DsgBxMlpArgs(C.Structure):
    """dsg_bx_mlp_args of include/dsg_debug.h (dsg_debug_mlp_bx_args)"""
    _fields_ = ([(n, C.c_void_p) for n in ("xn", "att", "x", "W1", "W2", "Wp", "b1", "b2", "bp", "xn_out", "mod_aff")] +
                [(n, C.c_int32) for n in ("out_mode", "mod_ld", "mod_off", "mod_T", "M", "C", "kernel")])


ROWLP_MERGE_LN, ROWLP_BREAKUP_LN, ROWLP_LN_BX, ROWLP_COPY_BX = range(4)                            # DSG_ROWLP_* (dsg_debug_row_lp)
CONVERT_BF16, CONVERT_SPLIT3, CONVERT_WIDEN = range(3)                                             # kinds of dsg_debug_convert


class DsgTProb(C.Structure):
    """dsg_t_prob of include/dsg_debug.h (dsg_debug_t_grouped): one problem of a grouped launch"""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "B", "bias", "C")] + [(n, C.c_int32) for n in ("lda", "ldb", "ldc", "M", "N", "K")])


T_GROUP_MAX = 32
TGROUP_NT, TGROUP_TN, TGROUP_NN, TGROUP_NN_SUM, TGROUP_SUM, TGROUP_COLSUM, TGROUP_TT = range(7)   # DSG_TGROUP_* of include/dsg_debug.h

DD_OFF, DD_GRAPH, DD_BATCH, DD_TABLE = range(4)                                                    # DedupMode of csrc/kernels.h (mode of dsg_debug_window_broadcast_f32)
HEAD_ADJ, HEAD_POOL, HEAD_NODE = range(3)                                                          # DSG_HEAD_* (dsg_debug_head_f32)
ROW_MOD_STATS, ROW_LN_STATS, ROW_LN_MOD, ROW_MERGE_LN, ROW_BREAKUP_LN, ROW_MERGE_NORM_RUNS = range(6)   # DSG_ROW_* (dsg_debug_row_f32)

# DSG_BXK_*: the `kernel` argument of dsg_debug_mlp_bx / dsg_debug_projmlp_bx / dsg_debug_qkv_attn_bx (BXK_DEFAULT: what the forward runs)
(BXK_DEFAULT, BXK_MLP384_DMA, BXK_MLP384_WAVE, BXK_MLP384_R3, BXK_MLP384_SOLO, BXK_MLP96_STAGED, BXK_MLP96_RESIDENT, BXK_QA10_WAVE,
 BXK_QA10_HEAD) = range(9)


def _declare_debug(L: C.CDLL) -> None:
    """the prototypes of include/dsg_debug.h; load() calls this on the library it has just opened"""
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.dsg_debug_box_guide.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(DsgGuideCfg), C.c_float, vp, vp, vp, vp, vp, vp, vp]
    L.dsg_debug_box_guide_rel.argtypes = L.dsg_debug_box_guide.argtypes + [C.POINTER(DsgRelCfg), vp]
    L.dsg_debug_content_guide.argtypes = [i32, i32, i32, i32] + [vp] * 7 + [C.POINTER(DsgContentCfg), C.c_float] + [vp] * 12
    L.dsg_debug_tap.argtypes = [vp, C.c_char_p, vp, i64]
    L.dsg_debug_clear_taps.argtypes = [vp]
    L.dsg_debug_clear_taps.restype = None
    L.dsg_debug_need_lists.argtypes = [vp, i32, vp, i32, C.POINTER(i32), vp, i64, vp]
    L.dsg_debug_dedup_lists.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.dsg_debug_dedup_level_lists.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.dsg_debug_dedup_launch_lists.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    L.dsg_debug_dedup_qkv_lists.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.dsg_debug_readout_tiles.argtypes = [vp, i32, vp, vp, vp]
    L.dsg_debug_patch_forms.argtypes = [vp, i32, vp]
    L.dsg_debug_assemble_patch_f32.argtypes = [i32] * 7 + [vp] * 8
    L.dsg_debug_head_patch_f32.argtypes = [i32] * 6 + [vp] * 6
    L.dsg_debug_patch_embed_patch_f32.argtypes = [i32] * 7 + [vp] * 11 + [i32] * 3 + [vp] * 2
    L.dsg_debug_readout_patch_f32.argtypes = [i32] * 4 + [vp] * 12
    L.dsg_debug_qk_split.argtypes = [i32, i32]
    L.dsg_debug_qk_split.restype = i32
    L.dsg_profile_clock_ghz.argtypes = [vp]
    L.dsg_profile_clock_ghz.restype = C.c_double
    L.dsg_debug_gemm.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    L.dsg_debug_gemm_f32.argtypes = [C.POINTER(DsgGemmF32Args), vp]
    L.dsg_debug_gemm_form.argtypes = [i32, i32, i32]
    L.dsg_debug_gemm_lp.argtypes = [C.POINTER(DsgGemmLpArgs), vp]
    L.dsg_debug_convert.argtypes = [i32, vp, vp, C.c_int64, vp]
    L.dsg_debug_row_lp.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.dsg_debug_window_attn_lp.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, i32, i32, vp]
    L.dsg_debug_gemm_form.restype = i32
    L.dsg_debug_qkv_attn_f32.argtypes = [i32] * 6 + [vp] * 5 + [i32] + [vp] * 5
    L.dsg_debug_window_attn_f32.argtypes = [i32] * 5 + [vp] * 4
    L.dsg_debug_fused_mlp_f32.argtypes = [i32, i32] + [vp] * 11
    L.dsg_debug_fused_attn96_f32.argtypes = [i32] * 4 + [vp, vp, i32, i32] + [vp] * 7 + [i32, vp, vp, vp]
    L.dsg_debug_patch_embed_f32.argtypes = [i32] * 6 + [vp] * 11 + [i32] * 3 + [vp] * 4
    L.dsg_debug_assemble_f32.argtypes = [i32] * 6 + [vp] * 8
    L.dsg_debug_readout_f32.argtypes = [i32] * 3 + [vp] * 12
    L.dsg_debug_head_f32.argtypes = [i32] * 5 + [vp] * 6
    L.dsg_debug_row_f32.argtypes = [i32] * 4 + [vp] * 6 + [i32, i32, vp, i32] + [vp] * 5
    L.dsg_debug_window_broadcast_f32.argtypes = [i32] * 3 + [vp] * 3 + [i32] + [vp] * 4 + [i32, i64] + [i32] * 6 + [vp, vp]
    L.dsg_debug_window_harvest_f32.argtypes = [i32] * 3 + [vp] * 3 + [i32, vp, i64] + [i32] * 3 + [vp]
    L.dsg_debug_t_gemm.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, C.POINTER(i32), vp]
    L.dsg_debug_t_gemm_lp.argtypes = L.dsg_debug_t_gemm.argtypes
    L.dsg_debug_t_cast_lp.argtypes = [vp, i32, i32, vp, vp, vp]
    L.dsg_debug_train_routes.argtypes = [vp, vp, i32]
    L.dsg_debug_t_attn.argtypes = [i32] * 6 + [vp] * 6 + [i32, vp]
    L.dsg_debug_t_ln.argtypes = [i32] * 4 + [vp] * 13
    L.dsg_debug_t_modulate.argtypes = [i32] * 4 + [vp] * 6
    L.dsg_debug_t_colsum.argtypes = [vp, i32, vp, i32, i32, vp]
    L.dsg_debug_t_grouped.argtypes = [i32, i32, C.POINTER(DsgTProb), vp, i32, vp]
    L.dsg_debug_gemm_bx.argtypes = [i32, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, C.POINTER(C.c_float), vp]
    L.dsg_debug_attn_bx.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, i32, C.POINTER(C.c_float), vp]
    L.dsg_debug_projmlp_bx.argtypes = [i32, i32] + [vp] * 9 + [i32, vp, i32, i32, C.POINTER(C.c_float), vp]
    L.dsg_debug_qkv_attn_bx.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, C.POINTER(C.c_float), vp]
    L.dsg_debug_mlp_bx.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, C.POINTER(C.c_float), vp]
    L.dsg_debug_gemm_bx_args.argtypes = [C.POINTER(DsgBxGemmArgs), vp]
    L.dsg_debug_mlp_bx_args.argtypes = [C.POINTER(DsgBxMlpArgs), vp]
    L.dsg_debug_t_assemble_bwd.argtypes = [i32] * 5 + [vp, i32] + [vp] * 8
    L.dsg_debug_t_patch_pack.argtypes = [i32] * 6 + [vp] * 5
    L.dsg_debug_t_adj_out_patch.argtypes = [i32] * 5 + [vp] * 6
    L.dsg_debug_t_pool_bwd_patch.argtypes = [i32] * 4 + [vp] * 4
    L.dsg_debug_t_live_cols_patch.argtypes = [i32] * 5 + [vp, vp, C.POINTER(i32), vp]
    L.dsg_debug_t_assemble_bwd_patch.argtypes = [i32] * 5 + [vp, i32] + [vp] * 8
    L.dsg_debug_graph_dot.argtypes = [i32] * 4 + [vp] * 7
    L.dsg_debug_poison.argtypes = [vp, i32, i32, C.c_uint64, vp]
    L.dsg_profile_forward.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]


_lib = None


# ABI generation of include/dsg.h this binding was written against (DSG_ABI_VERSION there): argument lists changed between rounds
# (e.g. iou_loss_type in the loss entries), and a stale libdsg.so would take shifted arguments without any error
ABI_VERSION = 5


def load(path: Optional[str] = None) -> C.CDLL:
    """dlopen libdsg.so and declare the prototypes of include/dsg.h and include/dsg_debug.h.  `path`: another build of the library -- the kernel-variant
    A/B builds of the dev tools pass it explicitly (tools/bx_bench.py); the product and the tests always load the in-tree one, and
    no environment variable redirects the load."""
    global _lib
    if _lib is not None:
        if path is not None and os.path.abspath(path) != getattr(_lib, "_dsg_path", None):
            raise DsgError(f"libdsg.so is already loaded from {_lib._dsg_path}; cannot switch to {path}")
        return _lib
    lib_path = os.path.abspath(path) if path is not None else LIB_PATH
    if not os.path.exists(lib_path):
        raise DsgError(f"{lib_path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7.  Importing torch first makes the
    # dynamic loader resolve libdsg.so's NEEDED libamdhip64.so.7 to that already-loaded copy, so streams and device
    # pointers are shared with torch.  (Loaded the other way round, two runtimes end up in the process and the second
    # one to initialise cannot see the GPU.)
    import torch  # noqa: F401
    L = C.CDLL(lib_path)
    L._dsg_path = lib_path
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    try:
        L.dsg_abi_version.restype = i32
        abi = int(L.dsg_abi_version())
    except AttributeError:
        abi = -1
    if abi != ABI_VERSION:
        raise DsgError(f"{lib_path} has ABI generation {abi}, this binding needs {ABI_VERSION}: rebuild it "
                       f"(python -c 'import __graft_entry__ as g; g.build()')")
    L.dsg_create.argtypes = [C.POINTER(DsgConfig), C.POINTER(vp)]
    L.dsg_create_patch.argtypes = [C.POINTER(DsgConfig), i32, C.POINTER(vp)]
    L.dsg_destroy.argtypes = [vp]
    L.dsg_destroy.restype = None
    L.dsg_last_error.argtypes = [vp]
    L.dsg_last_error.restype = C.c_char_p
    L.dsg_version.restype = C.c_char_p
    L.dsg_set_weight.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32, i32]
    L.dsg_finalize_weights.argtypes = [vp]
    L.dsg_num_weight_keys.argtypes = [vp]
    L.dsg_weight_key.argtypes = [vp, i32]
    L.dsg_weight_key.restype = C.c_char_p
    L.dsg_workspace_bytes.argtypes = [vp, i32]
    L.dsg_workspace_bytes.restype = C.c_size_t
    L.dsg_denoise.argtypes = [vp, i32] + [vp] * 9
    L.dsg_precond.argtypes = [vp, i32] + [vp] * 6 + [i32] + [vp] * 3
    L.dsg_sample.argtypes = [vp, C.POINTER(DsgSamplerCfg), i32, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp,
                             vp, i32, vp, vp, vp, vp, C.POINTER(DsgSampleStats), vp]
    L.dsg_sample_known.argtypes = [vp, C.POINTER(DsgSamplerCfg), i32, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp,
                                   vp, i32, vp, vp, vp, vp, C.POINTER(DsgSampleStats), vp]
    L.dsg_sample_walk.argtypes = [vp, C.POINTER(DsgSamplerCfg), C.POINTER(DsgWalkCfg), i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64,
                                  vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, C.POINTER(DsgSampleStats), vp]
    L.dsg_sample_seeded.argtypes = [vp, C.POINTER(DsgSamplerCfg), C.POINTER(DsgWalkCfg), i32, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp,
                                    vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, C.POINTER(DsgSampleStats), vp]
    L.dsg_gen_noise_seeded.argtypes = [vp, i32, vp, vp, C.c_uint32, vp, vp, vp]
    L.dsg_sample_guided.argtypes = [vp, C.POINTER(DsgSamplerCfg), C.POINTER(DsgWalkCfg), i32, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp,
                                    vp, vp, vp, vp, vp, i32, vp, vp, C.POINTER(DsgGuideCfg), vp, vp, vp, vp, vp, C.POINTER(DsgSampleStats), vp]
    L.dsg_guide_coef.argtypes = [C.POINTER(DsgSamplerCfg), vp, vp, i32]
    L.dsg_guide_coef.restype = i32
    L.dsg_sample_guided_rel.argtypes = L.dsg_sample_guided.argtypes + [C.POINTER(DsgRelCfg)]
    L.dsg_sample_guided_content.argtypes = L.dsg_sample_guided_rel.argtypes + [C.POINTER(DsgContentCfg), vp]
    L.dsg_walk_steps.argtypes = [C.POINTER(DsgSamplerCfg), C.POINTER(DsgWalkCfg), vp, vp, i32]
    L.dsg_walk_steps.restype = i32
    L.dsg_multistep_coef.argtypes = [C.POINTER(DsgSamplerCfg), C.POINTER(DsgWalkCfg), vp, i32]
    L.dsg_multistep_coef.restype = i32
    L.dsg_sigma_schedule.argtypes = [C.POINTER(DsgSamplerCfg), vp, vp, vp, vp]
    L.dsg_set_option.argtypes = [vp, C.c_char_p, i32]
    L.dsg_get_option.argtypes = [vp, C.c_char_p, C.POINTER(i32)]
    L.dsg_option_info.argtypes = [i32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)] + [C.POINTER(i32)] * 3
    L.dsg_gen_noise.argtypes = [vp, i32, vp, C.c_uint64, C.c_uint32, vp, vp, vp]
    L.dsg_train_inputs.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp]
    L.dsg_rainbow_loss.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, i32, vp, vp, vp]
    L.dsg_block_train.argtypes = [vp, C.c_char_p, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), vp]
    L.dsg_train_grads.argtypes = [vp, i32] + [vp] * 10 + [i32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), vp]
    L.dsg_train_step_grads.argtypes = [vp, i32] + [vp] * 9 + [C.c_float] * 3 + [i32] + [vp] * 4 + [i32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), vp]
    L.dsg_train_self_cond.argtypes = [vp, i32] + [vp] * 7
    L.dsg_precond_vjp.argtypes = [vp, i32] + [vp] * 8 + [GRAD_FN, vp] + [vp] * 5
    L.dsg_ode_run.argtypes = [vp, C.POINTER(DsgSamplerCfg), C.POINTER(DsgOdeCfg), i32] + [vp] * 12
    L.dsg_ode_evals.argtypes = [C.POINTER(DsgSamplerCfg), C.POINTER(DsgOdeCfg), vp, vp, i32]
    L.dsg_ode_evals.restype = i32
    L.dsg_train_bind_params.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p)]
    L.dsg_train_set_precision.argtypes = [vp, i32]
    L.dsg_train_get_precision.argtypes = [vp, C.POINTER(i32)]
    L.dsg_train_enable_patch.argtypes = [vp, i32]
    L.dsg_train_patch_enabled.argtypes = [vp]
    L.dsg_train_patch_enabled.restype = i32
    L.dsg_attach_guide.argtypes = [vp, vp, C.c_float, C.c_float, C.c_float]
    L.dsg_detach_guide.argtypes = [vp]
    L.dsg_guide_info.argtypes = [vp, C.POINTER(vp)] + [C.POINTER(C.c_float)] * 3
    L.dsg_guide_forwards.argtypes = [vp, C.POINTER(i64)]
    L.dsg_adam_step.argtypes = [i32] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(C.c_int64), i32] + [C.c_float] * 6 + [C.POINTER(C.c_float), vp]
    L.dsg_ema_update.argtypes = [i32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_float, vp]
    L.dsg_noise_embed.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.dsg_affine_width.argtypes = [vp]
    L.dsg_affine_width.restype = i32
    L.dsg_rainbow_loss_backward.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, i32, vp, vp, vp, vp, vp, vp]
    L.dsg_decode_bits.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.dsg_decode.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.dsg_encode.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.dsg_eval_bbox_prep_bytes.argtypes = [i32, i32, i32]
    L.dsg_eval_bbox_prep_bytes.restype = C.c_size_t
    L.dsg_eval_bbox_prep.argtypes = [i32, i32, i32, vp, vp, vp, i32, vp, vp, vp]
    L.dsg_eval_bbox_f1.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, i32, C.POINTER(C.c_double), i32, i32, i32, i32, vp, vp]
    L.dsg_eval_type_hist.argtypes = [i32, i32, i32, i32, vp, vp, vp, i32, vp, vp]
    L.dsg_eval_degree_hist.argtypes = [i32, i32, vp, vp, i32, vp, vp]
    L.dsg_eval_hist_mmd.argtypes = [i32, vp, i32, i32, vp, i32, i32, vp, vp, vp]
    L.dsg_sgstat_triplet_counts.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.dsg_sgstat_layout.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp]
    L.dsg_sgstat_f1_rowstats.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp]
    _declare_debug(L)
    _lib = L
    return L


# `--edge_encoding` / `--node_encoding` of the reference (R/utils/arg_parser.py) -> DSG_ENC_* (include/dsg.h)
ENCODINGS = {"bits": 0, "one_hot": 1, "ddpm": 2}


# iou_loss_type of the trainer's bounding-box term (trainer_node_adj.py:138-153) -> DSG_IOU_* (include/dsg.h)
IOU_LOSS_TYPES = {"iou": 0, "giou": 1, "giou_squared": 2, "diou": 3, "ciou": 4}


def iou_loss_type_code(name: str) -> int:
    if name not in IOU_LOSS_TYPES:
        raise NotImplementedError(name)   # the reference's `else: raise NotImplementedError` (trainer_node_adj.py:153-154)
    return IOU_LOSS_TYPES[name]


def make_config(cfg) -> DsgConfig:
    c = DsgConfig()
    c.max_node_num, c.c_adj, c.c_node, c.embed_dim = cfg.max_node_num, cfg.c_adj, cfg.c_node, cfg.embed_dim
    c.num_layers = cfg.num_layers
    for i in range(cfg.num_layers):
        c.depths[i] = cfg.depths[i]
        c.num_heads[i] = cfg.num_heads[i]
    c.window_size, c.mlp_ratio, c.self_condition = cfg.window_size, cfg.mlp_ratio, int(cfg.self_condition)
    return c


# solver= of the sampler -> DSG_SOLVER_* (dsg_sampler_cfg.heun, include/dsg.h)
SOLVERS = {"euler": 0, "heun": 1, "dpmpp_2m": 2}


def make_sampler_cfg(num_steps: int, solver: str = "heun", S_churn: float = 40.0, S_min: float = 0.05,
                     S_max: float = 50.0, S_noise: float = 1.003, sigma_min: float = 0.002, sigma_max: float = 80.0,
                     rho: float = 7.0, use_graph: bool = True) -> DsgSamplerCfg:
    if solver not in SOLVERS:
        raise ValueError(solver)
    return DsgSamplerCfg(int(num_steps), SOLVERS[solver], S_churn, S_min, S_max, S_noise,
                         sigma_min, sigma_max, rho, int(bool(use_graph)), 0)


class Handle:
    """Owns one dsg_handle.  Raises DsgError with the library's message on any non-zero status."""

    def __init__(self, cfg):
        self.L = load()
        self.cfg = cfg
        self._c = make_config(cfg)
        self._h = C.c_void_p()
        ps = int(getattr(cfg, "patch_size", 1))   # the reference's patch_size is not a field of dsg_config: its own entry point
        rc = (self.L.dsg_create(C.byref(self._c), C.byref(self._h)) if ps == 1 else
              self.L.dsg_create_patch(C.byref(self._c), ps, C.byref(self._h)))
        if rc != 0:
            why = self.L.dsg_last_error(None)
            raise DsgError(f"dsg_create failed with status {rc}: {why.decode() if why else ''} (there is no CPU fallback)")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.L.dsg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, what: str):
        if rc != 0:
            raise DsgError(f"{what}: status {rc}: {self.L.dsg_last_error(self._h).decode()}")

    @property
    def raw(self):
        return self._h

    def weight_keys(self):
        return [self.L.dsg_weight_key(self._h, i).decode() for i in range(self.L.dsg_num_weight_keys(self._h))]

    def set_weight(self, key: str, ptr: int, shape, is_device: bool):
        shp = (C.c_int64 * len(shape))(*shape)
        self.check(self.L.dsg_set_weight(self._h, key.encode(), C.c_void_p(ptr), shp, len(shape), int(is_device)),
                   f"dsg_set_weight({key})")

    def set_option(self, name: str, value: int):
        self.check(self.L.dsg_set_option(self._h, name.encode(), int(value)), f"dsg_set_option({name})")

    def get_option(self, name: str) -> int:
        v = C.c_int32(0)
        self.check(self.L.dsg_get_option(self._h, name.encode(), C.byref(v)), f"dsg_get_option({name})")
        return int(v.value)

    def set_train_precision(self, precision: str):
        """Precision of the training entries' large products (dsg_train_set_precision): "fp32" (default) or "bf16"."""
        if precision not in TRAIN_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(TRAIN_PRECISIONS)}, not {precision!r}")
        self.check(self.L.dsg_train_set_precision(self._h, TRAIN_PRECISIONS[precision]), "dsg_train_set_precision")

    def get_train_precision(self) -> str:
        v = C.c_int32(0)
        self.check(self.L.dsg_train_get_precision(self._h, C.byref(v)), "dsg_train_get_precision")
        return {m: name for name, m in TRAIN_PRECISIONS.items()}[int(v.value)]

    def enable_patch_training(self, on: bool = True):
        """The training form at patch_size > 1 (dsg_train_enable_patch): off by default, a no-op at patch_size 1.  The Python training,
        input-gradient and ODE entry points call it themselves: calling them is the opt-in."""
        self.check(self.L.dsg_train_enable_patch(self._h, 1 if on else 0), "dsg_train_enable_patch")

    def patch_training_enabled(self) -> bool:
        return bool(self.L.dsg_train_patch_enabled(self._h))

    def attach_guide(self, guide: "Handle", scale: float, sigma_lo: float, sigma_hi: float):
        """Autoguidance (dsg_attach_guide): `guide` becomes this handle's weaker network, D~ = D + (scale - 1)(D - D_guide) at the noise
        levels in [sigma_lo, sigma_hi].  The caller keeps `guide` alive while it is attached."""
        self.check(self.L.dsg_attach_guide(self._h, guide._h, float(scale), float(sigma_lo), float(sigma_hi)), "dsg_attach_guide")

    def detach_guide(self):
        self.check(self.L.dsg_detach_guide(self._h), "dsg_detach_guide")

    def guide_info(self):
        """(guide handle address or None, scale, sigma_lo, sigma_hi) of the attachment (dsg_guide_info)."""
        g, s, lo, hi = C.c_void_p(), C.c_float(), C.c_float(), C.c_float()
        self.check(self.L.dsg_guide_info(self._h, C.byref(g), C.byref(s), C.byref(lo), C.byref(hi)), "dsg_guide_info")
        return g.value, float(s.value), float(lo.value), float(hi.value)

    def guide_forwards(self) -> int:
        """The guide's network forwards in this handle's last dsg_sample* call (dsg_guide_forwards)."""
        n = C.c_int64(0)
        self.check(self.L.dsg_guide_forwards(self._h, C.byref(n)), "dsg_guide_forwards")
        return int(n.value)

    def train_routes(self):
        """Test only (dsg_debug_train_routes): {(token rows, class): (products on the bf16 route, on an fp32 route)} of the covered
        products of the last training entry; class 0 y = x W^T, 1 dx = dy W, 2 dW = dy^T x.  Empty with the mode off."""
        buf = (C.c_int32 * (4 * 64))()
        n = self.L.dsg_debug_train_routes(self._h, buf, 64)
        if n < 0:
            raise DsgError("dsg_debug_train_routes failed")
        return {(buf[4 * k], buf[4 * k + 1]): (buf[4 * k + 2], buf[4 * k + 3]) for k in range(min(n, 64))}

    def poison(self, B: int, pattern: int, seed: int = 0, stream=None):
        """Test only (dsg_debug_poison): every scratch buffer of the handle and of batch B's workspace becomes `pattern` -- 1 zeros,
        2 NaN, 3 1e30, 4 pseudo-random finite values, a function of (seed, element) -- on `stream` (None: the null stream)."""
        self.check(self.L.dsg_debug_poison(self._h, int(B), int(pattern), C.c_uint64(int(seed)), stream), "dsg_debug_poison")

    def need_lists(self, B: int, stream=None):
        """Need lists of the masked-token pruning as the flags last staged for batch B left them (dsg_debug_need_lists): a list of
        dicts {kind ('runs' | 'windows'), res, shift, stage, block, full, entries (int32 array)}; [] when the configuration is not
        covered.  A run is 8 consecutive token rows (entry = first row / 8), a window entry is b * nW + window."""
        import numpy as np
        n = C.c_int32(0)
        self.check(self.L.dsg_debug_need_lists(self._h, B, None, 0, C.byref(n), None, 0, stream), "dsg_debug_need_lists")
        if n.value == 0:
            return []
        roles = np.zeros((n.value, 8), np.int32)
        self.check(self.L.dsg_debug_need_lists(self._h, B, roles.ctypes.data, n.value, C.byref(n), None, 0, stream), "dsg_debug_need_lists")
        total = int(roles[:, 5].sum())
        ents = np.zeros(max(total, 1), np.int32)
        self.check(self.L.dsg_debug_need_lists(self._h, B, roles.ctypes.data, n.value, C.byref(n), ents.ctypes.data, total, stream),
                   "dsg_debug_need_lists")
        return [dict(kind="windows" if r[0] else "runs", res=int(r[1]), shift=int(r[2]), stage=int(r[3]), block=int(r[4]),
                     full=int(r[7]), entries=ents[int(r[6]):int(r[6]) + int(r[5])].copy()) for r in roles]

    def dedup_lists(self, B: int, stream=None):
        """Lists of the pure-window deduplication as the flags last staged for batch B left them (dsg_debug_dedup_lists): dict of
        int32 arrays wins (unique windows b * nW + w), runs (the same set as 8-token runs), copy (pure windows filled by copy) and
        rep [B] (each graph's representative window, -1: none; in a sampler call under "dedup_batch" one global id, of whichever graph,
        for every graph), and fwd: what the batch size's last forward did (-1 no deduplication,
        0 the copy moved activation rows, 1 also their LayerNorm partials); None when the configuration has no such lists."""
        return self.dedup_level_lists(B, 0, stream)

    def dedup_level_lists(self, B: int, level: int, stream=None):
        """dedup_lists for level `level` of the down path (dsg_debug_dedup_level_lists; level 0 is dedup_lists itself): window ids
        b * nW + w and run ids on the grid of N >> level tokens per side; fwd: -1 the last forward did not deduplicate the level, 0 the
        copy moved rows of the activation and the skip, 1 also their row statistics.  None when the plan has no lists for the level."""
        import numpy as np
        res = self.cfg.max_node_num >> level
        nw = max(1, (res // 8) ** 2)
        counts = np.zeros(4, np.int32)
        wins, runs, copy = np.zeros(B * nw, np.int32), np.zeros(max(1, B * res * res // 8), np.int32), np.zeros(B * nw, np.int32)
        rep = np.zeros(B, np.int32)
        self.check(self.L.dsg_debug_dedup_level_lists(self._h, B, level, counts.ctypes.data, wins.ctypes.data, runs.ctypes.data,
                                                      copy.ctypes.data, rep.ctypes.data, stream), "dsg_debug_dedup_level_lists")
        if counts[0] < 0:
            return None
        return dict(wins=wins[:counts[0]].copy(), runs=runs[:counts[1]].copy(), copy=copy[:counts[2]].copy(), rep=rep, fwd=int(counts[3]))

    def dedup_launch_lists(self, B: int, level: int, stream=None):
        """The lists of level `level` as the launches iterate them (dsg_debug_dedup_launch_lists): wins / runs -- what is computed,
        copy -- what the fill writes, mode -- 0 every window unique, 1 a representative per graph, 2 one for the batch, 3 one for the
        batch taken from the sampler's table ("dedup_table": it is in copy, not in wins / runs).  None when the plan has no lists."""
        import numpy as np
        res = self.cfg.max_node_num >> level
        nw = max(1, (res // 8) ** 2)
        counts = np.zeros(4, np.int32)
        wins, runs, copy = np.zeros(B * nw, np.int32), np.zeros(max(1, B * res * res // 8), np.int32), np.zeros(B * nw, np.int32)
        self.check(self.L.dsg_debug_dedup_launch_lists(self._h, B, level, counts.ctypes.data, wins.ctypes.data, runs.ctypes.data,
                                                       copy.ctypes.data, stream), "dsg_debug_dedup_launch_lists")
        if counts[0] < 0:
            return None
        return dict(wins=wins[:counts[0]].copy(), runs=runs[:counts[1]].copy(), copy=copy[:counts[2]].copy(), mode=int(counts[3]))

    def dedup_qkv_lists(self, B: int, level: int, stream=None):
        """Option "dedup_qkv" at level `level`'s second block (dsg_debug_dedup_qkv_lists): runs -- the 8-row runs whose q, k, v the split
        form projects, src [B * nW] -- the window that holds every window's q, k, v, split -- what the device's rule picks for these
        lists, form -- what the last forward took there ('split' | 'fused' | None: no switch at that block).  None: no such lists."""
        import numpy as np
        res = self.cfg.max_node_num >> level
        nw = max(1, (res // 8) ** 2)
        counts = np.zeros(4, np.int32)
        runs, src = np.zeros(max(1, B * res * res // 8), np.int32), np.zeros(B * nw, np.int32)
        self.check(self.L.dsg_debug_dedup_qkv_lists(self._h, B, level, counts.ctypes.data, runs.ctypes.data, src.ctypes.data, stream),
                   "dsg_debug_dedup_qkv_lists")
        if counts[0] < 0:
            return None
        return dict(runs=runs[:counts[0]].copy(), src=src[:counts[1]].copy(), split=bool(counts[2]),
                    form={1: "split", 0: "fused"}.get(int(counts[3])))

    def readout_tiles(self, B: int, stream=None):
        """The fused read-out's working tiles (dsg_debug_readout_tiles): tiles -- ascending ids t of the 32-token tiles [32 t, 32 t + 32) of the
        flattened [B * N * N] token index that hold a pair with flag_i and flag_j, as the flags last staged for batch B left them;
        form -- what the last forward's fused read-out took ('list' | 'pos' | None: none yet).  None: the plan has no such list."""
        import numpy as np
        n = self.cfg.max_node_num
        counts = np.zeros(2, np.int32)
        tiles = np.zeros(max(1, (B * n * n + 31) // 32), np.int32)
        self.check(self.L.dsg_debug_readout_tiles(self._h, B, counts.ctypes.data, tiles.ctypes.data, stream), "dsg_debug_readout_tiles")
        if counts[0] < 0:
            return None
        return dict(tiles=tiles[:counts[0]].copy(), form={1: "list", 0: "pos"}.get(int(counts[1])))

    def patch_forms(self, B: int):
        """The route batch B's last forward took through (PatchEmbed, the read-out): 'fused' | 'chain' | None (no forward yet)
        (dsg_debug_patch_forms)."""
        forms = (C.c_int32 * 2)()
        self.check(self.L.dsg_debug_patch_forms(self._h, B, forms), "dsg_debug_patch_forms")
        return tuple({1: "fused", 0: "chain"}.get(int(f)) for f in forms)

    def precision_mode(self) -> str:
        """'f32' | 'f32-split' | 'bf16': the GEMM arithmetic the handle will actually run (options or DSG_* env defaults)."""
        return "f32-split" if self.get_option("gemm_split") else ("bf16" if self.get_option("gemm_bf16") else "f32")

    def finalize(self):
        self.check(self.L.dsg_finalize_weights(self._h), "dsg_finalize_weights")


def option_table():
    """The library's option table (dsg_option_info), in its order: a list of dicts {name, env (None: no environment default), default,
    lo, hi} -- host-only, no GPU needed."""
    L, rows = load(), []
    name, env, dflt, lo, hi = C.c_char_p(), C.c_char_p(), C.c_int32(), C.c_int32(), C.c_int32()
    while L.dsg_option_info(len(rows), C.byref(name), C.byref(env), C.byref(dflt), C.byref(lo), C.byref(hi)) == 0:
        rows.append(dict(name=name.value.decode(), env=env.value.decode() if env.value else None, default=dflt.value, lo=lo.value, hi=hi.value))
    return rows


def sigma_schedule(scfg: DsgSamplerCfg):
    """(sigma_steps f64, t_hat f32, noise_coef f32, h f32) of the loop -- host-only, no GPU needed."""
    import numpy as np
    T = scfg.num_steps
    sg, th, nz, hs = np.empty(T, np.float64), np.empty(T, np.float32), np.empty(T, np.float32), np.empty(T, np.float32)
    rc = load().dsg_sigma_schedule(C.byref(scfg), sg.ctypes.data, th.ctypes.data, nz.ctypes.data, hs.ctypes.data)
    if rc != 0:
        raise DsgError(f"dsg_sigma_schedule: status {rc}")
    return sg, th, nz, hs


def make_walk_cfg(start_step: int = 0, resample=None, resample_range=None) -> DsgWalkCfg:
    """dsg_walk_cfg from the sampler's keywords: resample = (jump_len, n_resample) or None (no resampling); resample_range = (lo, hi)
    or None = from start_step to the end of the schedule (hi <= 0 also means the end)."""
    j, r = (1, 1) if resample is None else (int(resample[0]), int(resample[1]))
    lo, hi = (int(start_step), 0) if resample_range is None else (int(resample_range[0]), int(resample_range[1]))
    return DsgWalkCfg(int(start_step), j, r, lo, hi, (C.c_int32 * 3)(0, 0, 0))


def walk_steps(scfg: DsgSamplerCfg, walk: DsgWalkCfg):
    """(sched_idx int32 [L], noise_coef float32 [L]) of the walk as the loop executes it (dsg_walk_steps) -- host-only, no GPU
    needed.  DsgError naming the walk when the library refuses it."""
    import numpy as np
    L = load()
    n = int(L.dsg_walk_steps(C.byref(scfg), C.byref(walk), None, None, 0))
    if n < 0:
        raise DsgError(f"dsg_walk_steps: status {n}: bad walk (start_step {walk.start_step}, jump_len {walk.jump_len}, n_resample "
                       f"{walk.n_resample}, resample range ({walk.resample_lo}, {walk.resample_hi})) for num_steps {scfg.num_steps}: need "
                       f"0 <= start_step < T, jump_len >= 1, n_resample >= 1, start_step <= lo <= hi <= T and at most {WALK_MAX_STEPS} "
                       f"executed steps")
    idx, coef = np.empty(n, np.int32), np.empty(n, np.float32)
    rc = int(L.dsg_walk_steps(C.byref(scfg), C.byref(walk), idx.ctypes.data, coef.ctypes.data, n))
    if rc != n:
        raise DsgError(f"dsg_walk_steps: status {rc}")
    return idx, coef


def multistep_coef(scfg: DsgSamplerCfg, walk: Optional[DsgWalkCfg] = None):
    """c_k float32 [L] of the second-order multistep update (dsg_multistep_coef) for every executed step of the walk (None = the
    trivial walk), as the loop runs them: 0 where the step is the Euler step, all 0 unless the solver is 'dpmpp_2m' -- host-only, no
    GPU needed.  DsgError when the library refuses the walk, or the multistep solver on a schedule with churn noise."""
    import numpy as np
    L = load()
    w = None if walk is None else C.byref(walk)
    n = int(L.dsg_multistep_coef(C.byref(scfg), w, None, 0))
    if n < 0:
        raise DsgError(f"dsg_multistep_coef: status {n}: a bad walk, or solver 'dpmpp_2m' on a schedule that draws churn noise "
                       f"(S_churn = {scfg.S_churn:g}; it needs S_churn = 0)")
    coef = np.empty(n, np.float32)
    rc = int(L.dsg_multistep_coef(C.byref(scfg), w, coef.ctypes.data, n))
    if rc != n:
        raise DsgError(f"dsg_multistep_coef: status {rc}")
    return coef


def guide_coef(scfg: DsgSamplerCfg, weights):
    """c_i float32 [T] of box guidance (dsg_guide_coef): w_i t_hat[i]^2 c_skip(t_hat[i]) per schedule index as the guided loop stages
    them -- host-only, no GPU needed.  DsgError when the library refuses the weights (not T of them, or one that is not finite)."""
    import numpy as np
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.shape != (scfg.num_steps,):
        raise DsgError(f"dsg_guide_coef: {scfg.num_steps} weights expected (one per schedule index), got shape {w.shape}")
    coef = np.empty(scfg.num_steps, np.float32)
    rc = int(load().dsg_guide_coef(C.byref(scfg), w.ctypes.data, coef.ctypes.data, scfg.num_steps))
    if rc != scfg.num_steps:
        raise DsgError(f"dsg_guide_coef: status {rc}: the weights must be finite")
    return coef


def make_ode_cfg(direction: str = "encode", probe: str = "none") -> DsgOdeCfg:
    if direction not in ("encode", "decode") or probe not in ODE_PROBES:
        raise ValueError((direction, probe))
    return DsgOdeCfg(ODE_ENCODE if direction == "encode" else ODE_DECODE, ODE_PROBES[probe], (C.c_int32 * 6)(*([0] * 6)))


def ode_evals(scfg: DsgSamplerCfg, ocfg: DsgOdeCfg):
    """(t_eval float32 [n_evals], weight float64 [n_evals]) of an ODE run (dsg_ode_evals): the evaluation levels in execution order
    and the quadrature weights w_k of sum_k w_k n_k ~ int n(t) / t dt -- host-only, no GPU needed.  DsgError when the library refuses
    the run: fewer than two levels, the multistep solver, a schedule that draws churn noise, a bad direction or probe."""
    import numpy as np
    L = load()
    n = int(L.dsg_ode_evals(C.byref(scfg), C.byref(ocfg), None, None, 0))
    if n < 0:
        raise DsgError(f"dsg_ode_evals: status {n}: the ODE needs num_steps >= 2 (it is {scfg.num_steps}), solver 'euler' or 'heun', "
                       f"a schedule that draws no churn noise (S_churn = {scfg.S_churn:g}; it needs S_churn = 0) and a known direction / probe")
    t, w = np.empty(n, np.float32), np.empty(n, np.float64)
    rc = int(L.dsg_ode_evals(C.byref(scfg), C.byref(ocfg), t.ctypes.data, w.ctypes.data, n))
    if rc != n:
        raise DsgError(f"dsg_ode_evals: status {rc}")
    return t, w
