"""ctypes binding of libbrepgen_hip.so -- the C ABI declared in include/brepgen_hip.h.

There is NO fallback: if the library is missing the import of any compute entry point raises.  The product
path never touches ``oracle/`` or torch math for the work the HIP kernels do.
"""
import contextlib
import ctypes as C
import enum
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbrepgen_hip.so")

BG_F32, BG_F16, BG_BF16 = 0, 1, 2
BG_ACT_NONE, BG_ACT_RELU = 0, 1
BG_SURFPOS, BG_SURFZ, BG_EDGEPOS, BG_EDGEZ = 0, 1, 2, 3
BG_MAX_LAYERS, BG_MAX_EMBEDS = 12, 5
BG_ATTN_BWD_AUTO, BG_ATTN_BWD_GENERAL, BG_ATTN_BWD_SHORT = 0, 1, 2      # enum bg_attn_bwd_variant
BG_CONV_SAME, BG_CONV_DOWN2, BG_CONV_UP2 = 0, 1, 2                      # enum bg_conv_geom

vp, fp, i64p, u8p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p   # device pointers travel as integers


class MlpWeights(C.Structure):
    _fields_ = [("w0", vp), ("b0", fp), ("ln_g", fp), ("ln_b", fp), ("w3", vp), ("b3", fp),
                ("k_in", C.c_int), ("n_out", C.c_int), ("n_out_pad", C.c_int), ("w0_dtype", C.c_int),
                ("w0_mfma", fp), ("w0_colsum", fp)]


class LayerWeights(C.Structure):
    _fields_ = [("ln1_g", fp), ("ln1_b", fp), ("ln2_g", fp), ("ln2_b", fp),
                ("w_qkv", vp), ("b_qkv", fp), ("w_o", vp), ("b_o", fp),
                ("w_1", vp), ("b_1", fp), ("w_2", vp), ("b_2", fp),
                ("qkv_colsum", fp), ("w1_colsum", fp), ("w_1f", vp), ("w_2f", vp)]


class DenoiserWeights(C.Structure):
    _fields_ = [("net", C.c_int), ("dtype", C.c_int), ("n_layer", C.c_int), ("_pad", C.c_int),
                ("layers", LayerWeights * BG_MAX_LAYERS),
                ("lnf_g", fp), ("lnf_b", fp),
                ("time_embed", MlpWeights), ("fc_out", MlpWeights),
                ("embed", MlpWeights * BG_MAX_EMBEDS),
                ("class_embed", fp), ("time_table", fp), ("time_table_rows", C.c_int), ("_pad3", C.c_int)]


class DenoiserInputs(C.Structure):
    _fields_ = [("B", C.c_int), ("S", C.c_int), ("E", C.c_int), ("n_timesteps", C.c_int),
                ("x", fp), ("surf_pos", fp), ("surf_z", fp), ("edge_pos", fp), ("mask", u8p),
                ("timesteps", i64p), ("class_label", i64p), ("cond_cache", fp),
                ("cond_cache_valid", C.c_int), ("varlen", C.c_int), ("rows_hint", C.c_double),
                ("pairs_hint", C.c_double), ("n_split", C.c_int), ("_pad2", C.c_int), ("rows_plan", C.c_double * 4)]


class GemmDesc(C.Structure):          # bg_gemm_desc
    _fields_ = [("a", vp), ("lda", C.c_int), ("w", vp), ("bias", fp), ("out", vp), ("ldc", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("N_pad", C.c_int), ("K", C.c_int),
                ("ab_dtype", C.c_int), ("out_dtype", C.c_int), ("act", C.c_int),
                ("add", fp), ("ld_add", C.c_int), ("add_div", C.c_int),
                ("add2", fp), ("ld_add2", C.c_int), ("add2_div", C.c_int),
                ("out_lo", vp), ("res_hi", vp), ("res_lo", vp), ("ld_res", C.c_int),
                ("stats_out", fp), ("stats_in", fp), ("colsum", fp), ("ln_eps", C.c_float)]


BG_E_ARG, BG_E_SHAPE, BG_E_WORKSPACE, BG_E_DTYPE, BG_E_ALIGN = -1, -2, -3, -4, -5      # enum bg_err


class ConvDesc(C.Structure):          # bg_conv_desc
    _fields_ = [("x", vp), ("S", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int),
                ("kh", C.c_int), ("kw", C.c_int), ("up", C.c_int),
                ("w", vp), ("bias", fp), ("N", C.c_int),
                ("out", fp), ("ldc", C.c_int),
                ("add", fp), ("ld_add", C.c_int),
                ("dtype", C.c_int), ("zero_page", vp)]


class VaeOp(C.Structure):             # bg_vae_op
    _fields_ = [("op", C.c_int), ("src", C.c_int), ("dst", C.c_int), ("res", C.c_int),
                ("kh", C.c_int), ("kw", C.c_int), ("up", C.c_int), ("stride", C.c_int), ("pad_mode", C.c_int),
                ("n_out", C.c_int), ("n_pad", C.c_int), ("w_dtype", C.c_int),
                ("w", vp), ("bias", fp), ("gn_gamma", fp), ("gn_beta", fp), ("gn_groups", C.c_int),
                ("gn_eps", C.c_float), ("act", C.c_int), ("heads", C.c_int), ("scale", C.c_float),
                ("n_pad2", C.c_int), ("w2_dtype", C.c_int), ("w2", vp), ("bias2", fp)]


class CadStore(C.Structure):         # bg_cad_store
    _fields_ = [("surf_ncs", fp), ("surf_pos", fp), ("edge_ncs", fp), ("edge_pos", fp), ("corner_wcs", fp),
                ("face_off", vp), ("edge_off", vp), ("adj_off", vp), ("adj_idx", vp),
                ("n_records", C.c_int), ("n_faces", C.c_int), ("n_edges", C.c_int), ("n_adj", C.c_int)]


class BatchDraws(C.Structure):       # bg_batch_draws
    _fields_ = [("u", fp), ("turns", vp), ("face_key1", vp), ("face_key2", vp), ("edge_key1", vp), ("edge_key2", vp)]


class BatchOut(C.Structure):         # bg_batch_out
    _fields_ = [("surf_pos", fp), ("surf_ncs", fp), ("surf_mask", u8p), ("edge_pos", fp), ("edge_ncs", fp), ("edge_mask", u8p),
                ("vertex_pos", fp)]


class MtRow(C.Structure):           # bg_mt_row
    _fields_ = [("p", fp), ("g", fp), ("m", fp), ("v", fp), ("numel", C.c_longlong), ("lr", C.c_double), ("decay", C.c_float),
                ("has_decay", C.c_int)]


class MtChunk(C.Structure):         # bg_mt_chunk
    _fields_ = [("first", C.c_longlong), ("tensor", C.c_int), ("_pad", C.c_int)]


class OptimState(C.Structure):      # bg_optim_state
    _fields_ = [("beta1_pow", C.c_double), ("beta2_pow", C.c_double), ("step", C.c_int), ("total_norm", C.c_float),
                ("found_inf", C.c_int), ("_pad", C.c_int)]


class ScalerState(C.Structure):     # bg_scaler_state
    _fields_ = [("scale", C.c_float), ("growth_tracker", C.c_int)]


class ProfileRow(C.Structure):
    _fields_ = [("kernel", C.c_char_p), ("launches", C.c_int), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


_SIGNATURES = {
    "bg_abi_version": (C.c_int, []),
    "bg_last_error": (C.c_char_p, []),
    "bg_sincos_embed": (C.c_int, [i64p, C.c_int, fp, vp]),
    "bg_layernorm_fwd": (C.c_int, [fp, fp, fp, vp, C.c_int, C.c_int, C.c_float, C.c_int, vp]),
    "bg_gemm_bias_act_fwd": (C.c_int, [vp, C.c_int, vp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, vp]),
    "bg_gemm_ex_fwd": (C.c_int, [C.POINTER(GemmDesc), vp]),
    "bg_conv_gemm_fwd": (C.c_int, [C.POINTER(ConvDesc), vp]),
    "bg_vae_workspace_bytes": (C.c_size_t, [C.POINTER(VaeOp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bg_vae_run": (C.c_int, [C.POINTER(VaeOp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, vp, vp,
                             C.c_size_t, vp]),
    "bg_layernorm_split_fwd": (C.c_int, [vp, vp, fp, fp, vp, C.c_int, C.c_int, C.c_float, vp]),
    "bg_embed_ln_silu_fwd": (C.c_int, [fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, vp, C.c_int, C.c_float, vp]),
    "bg_ln_silu_out_fwd": (C.c_int, [vp, fp, fp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "bg_attn_fwd": (C.c_int, [vp, u8p, vp, C.c_int, C.c_int, C.c_int, vp]),
    "bg_ffn_fused_fwd": (C.c_int, [vp, vp, fp, vp, fp, fp, vp, fp, C.c_int, C.c_int, vp, C.c_int, C.c_float, vp]),
    "bg_qkv_attn_fwd": (C.c_int, [vp, vp, fp, fp, fp, u8p, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "bg_qkv_attn_paired_fwd": (C.c_int, [vp, vp, fp, fp, fp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "bg_compact_rows_paired": (C.c_int, [u8p, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
    "bg_attn_varlen_fwd": (C.c_int, [vp, u8p, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bg_compact_rows": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "bg_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bg_denoiser_fwd": (C.c_int, [C.POINTER(DenoiserWeights), C.POINTER(DenoiserInputs), fp, vp, C.c_size_t, vp]),
    "bg_embed_mlp_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bg_embed_mlp_fwd": (C.c_int, [C.POINTER(MlpWeights), C.c_int, vp, C.c_int, C.c_int, fp, C.c_int, fp, C.c_int, C.c_int,
                                   vp, C.c_size_t, vp]),
    "bg_encoder_layer_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "bg_encoder_layer_fwd": (C.c_int, [C.POINTER(LayerWeights), C.c_int, fp, u8p, C.c_int, C.c_int, vp, C.c_size_t, vp]),
    "bg_cfg_ddpm_step": (C.c_int, [fp, fp, C.c_float, fp, fp, fp, C.c_size_t] + [C.c_float] * 6 + [vp]),
    "bg_pndm_step": (C.c_int, [fp, fp, C.c_float, fp, fp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float,
                               fp, fp, fp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, fp,
                               C.c_size_t, vp]),
    "bg_groupnorm_stats": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "bg_im2col": (C.c_int, [fp, vp] + [C.c_int] * 13 + [fp, fp, fp, C.c_int, C.c_int, fp, vp]),
    "bg_downsample1d_cubic": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, vp]),
    "bg_upsample1d_cubic": (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, vp]),
    "bg_small_attn": (C.c_int, [fp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "bg_dedup_surfaces": (C.c_int, [fp, C.c_float, fp, u8p, C.c_int, C.c_int, vp]),
    "bg_dedup_edges": (C.c_int, [fp, u8p, C.c_float, u8p, C.c_int, C.c_int, C.c_int, vp]),
    "bg_profile_begin": (C.c_int, [C.c_int]),
    "bg_profile_end": (C.c_int, [C.POINTER(ProfileRow), C.c_int]),
    "bg_tune_set": (C.c_int, [C.c_int, C.c_int]),
    "bg_allgather": (C.c_int, [vp, vp, C.c_size_t, vp, vp]),
    "bg_slot_packing_applies": (C.c_int, [C.c_int] * 6),
    "bg_gemm_p256_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bg_add_noise": (C.c_int, [fp, fp, fp, fp, fp, C.c_int, C.c_size_t, vp]),
    "bg_chamfer_offset_fit": (C.c_int, [fp, fp, vp, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 + [fp, fp, fp, vp]),
    "bg_philox_randn": (C.c_int, [fp, C.c_longlong, C.c_int, C.c_ulonglong, C.c_uint, C.c_longlong, C.c_int, vp]),
    "bg_masked_mse": (C.c_int, [fp, fp, u8p, C.c_longlong, C.c_int, C.c_int, C.c_int, vp, fp, vp]),
    "bg_chamfer_pairwise": (C.c_int, [fp, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, vp]),
    "bg_occupancy_counts": (C.c_int, [fp, C.c_int, C.c_int, fp, C.c_int, vp, vp, vp]),
    "bg_mesh_sample": (C.c_int, [fp, vp, C.c_int, C.c_int, C.c_ulonglong, C.c_uint, C.c_longlong, fp, fp, fp, vp, fp, vp]),
    "bg_vae_posterior": (C.c_int, [fp, fp, C.c_longlong, C.c_int, C.c_int, C.c_ulonglong, C.c_uint, C.c_longlong, fp, fp, fp, vp]),
    "bg_cad_filter": (C.c_int, [C.POINTER(CadStore), C.c_int, C.c_int, C.c_float, C.c_double, u8p, vp]),
    "bg_batch_plan": (C.c_int, [C.POINTER(CadStore), vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_uint,
                                C.POINTER(BatchDraws), vp, vp, vp, fp, vp]),
    "bg_batch_gather": (C.c_int, [C.POINTER(CadStore), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp, fp,
                                  C.POINTER(BatchOut), vp]),
    "bg_points_rotate_normalize": (C.c_int, [fp, C.c_longlong, C.c_int, C.c_int, C.c_ulonglong, C.c_uint, C.c_longlong, fp, vp, fp, vp]),
    "bg_points_sha256": (C.c_int, [fp, C.c_longlong, C.c_int, C.c_int, u8p, vp]),
    "bg_digest_group_keys": (C.c_int, [u8p, vp, C.c_int, C.c_int, u8p, vp]),
    "bg_first_occurrence": (C.c_int, [u8p, C.c_longlong, vp, C.c_longlong, u8p, vp]),
    "bg_mt_grad_stats": (C.c_int, [vp, vp, C.c_int, vp, vp]),
    "bg_mt_adamw_step": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_float, C.c_double, C.c_double, C.c_double, vp]),
    "bg_optim_finish": (C.c_int, [vp, C.c_int, vp, vp, C.c_float, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, vp]),
    "bg_mt_scale_grads": (C.c_int, [vp, vp, C.c_int, vp, C.c_float, fp, vp]),
    "bg_attn_train_fwd": (C.c_int, [vp, u8p, vp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_double, C.c_ulonglong, C.c_uint,
                                    C.c_longlong, vp]),
    "bg_attn_bwd_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "bg_attn_bwd": (C.c_int, [vp, u8p, fp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_double, C.c_ulonglong, C.c_uint,
                              C.c_longlong, C.c_int, vp, C.c_size_t, vp]),
    "bg_attn_dropout_mask": (C.c_int, [u8p, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_uint, C.c_longlong, vp]),
    "bg_linear_wgrad": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp,
                                  C.c_size_t, vp]),
    "bg_linear_wgrad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "bg_linear_wgrad_split": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "bg_weight_cast": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "bg_ln_train_fwd": (C.c_int, [vp, C.c_int, fp, fp, vp, C.c_int, fp, C.c_int, C.c_float, vp]),
    "bg_ln_bwd_workspace_bytes": (C.c_size_t, [C.c_int]),
    "bg_ln_bwd": (C.c_int, [vp, C.c_int, vp, C.c_int, fp, fp, vp, vp, fp, fp, C.c_int, vp, C.c_size_t, vp]),
    "bg_dropout_add_fwd": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_uint,
                                     C.c_int, C.c_longlong, vp]),
    "bg_dropout_bwd": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_uint, C.c_int,
                                 C.c_longlong, vp]),
    "bg_relu_dropout_fwd": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_uint, C.c_int,
                                      C.c_longlong, vp]),
    "bg_relu_dropout_bwd": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, vp]),
    "bg_dropout_mask": (C.c_int, [u8p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_ulonglong, C.c_uint, C.c_int, C.c_longlong, vp]),
    "bg_thin_expand": (C.c_int, [vp, C.c_int, C.c_int, fp, C.c_int, fp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "bg_thin_contract": (C.c_int, [vp, C.c_int, fp, fp, fp, C.c_int, C.c_int, vp]),
    "bg_thin_wgrad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bg_thin_wgrad": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, fp, C.c_int, fp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]),
    "bg_ln_silu_train_fwd": (C.c_int, [vp, C.c_int, fp, fp, vp, C.c_int, fp, C.c_int, C.c_float, vp]),
    "bg_ln_silu_bwd_workspace_bytes": (C.c_size_t, [C.c_int]),
    "bg_ln_silu_bwd": (C.c_int, [vp, C.c_int, vp, C.c_int, fp, fp, fp, vp, fp, fp, C.c_int, vp, C.c_size_t, vp]),
    "bg_masked_mse_bwd": (C.c_int, [fp, fp, u8p, C.c_longlong, C.c_int, C.c_int, C.c_int, fp, fp, fp, vp]),
    "bg_conv_wgrad": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp] + [C.c_int] * 10 + [vp, C.c_size_t, vp]),
    "bg_conv_wgrad_workspace_bytes": (C.c_size_t, [C.c_int] * 8),
    "bg_conv_wgrad_split": (C.c_int, [C.c_int] * 7),
    "bg_conv_weight_pack": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "bg_gn_act_bwd_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "bg_gn_act_bwd": (C.c_int, [fp, fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]),
    "bg_conv_wgrad_geom": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp] + [C.c_int] * 11 + [vp, C.c_size_t, vp]),
    "bg_conv_wgrad_geom_workspace_bytes": (C.c_size_t, [C.c_int] * 9),
    "bg_conv_wgrad_geom_split": (C.c_int, [C.c_int] * 8),
    "bg_conv_weight_pack_down": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "bg_conv_down_dgrad_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "bg_conv_down_dgrad": (C.c_int, [vp, C.c_int, vp, fp] + [C.c_int] * 6 + [vp, C.c_size_t, vp]),
    "bg_pool2x2_sum": (C.c_int, [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
}
EXPORTS = tuple(_SIGNATURES)

ABI_VERSION = 7          # BG_ABI_VERSION of include/brepgen_hip.h this binding was written against

_lib = None


class BrepgenHipError(RuntimeError):
    pass


def load():
    """dlopen the HIP library (once).  Raises if it has not been built: no silent CPU/torch fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BrepgenHipError(
                f"{LIB_PATH} is missing -- build it with `python -m brepgen_amd.build` "
                "(hipcc --offload-arch=gfx950); brepgen_amd has no fallback path")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the .so does not export the ABI
            fn.restype, fn.argtypes = res, args
        if lib.bg_abi_version() != ABI_VERSION:
            raise BrepgenHipError("libbrepgen_hip.so ABI version mismatch")
        at_load = parse_tune(os.environ.get("BG_TUNE", ""))      # A/B knobs, e.g. BG_TUNE="P256_MODE=2,13=1".  Read BEFORE the library
        _lib = lib                                               # is published: a bad string raises at every load(), none of it applied
        for key, value in at_load.items():
            _tune_set(key, value)
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().bg_last_error().decode(errors="replace")
        raise BrepgenHipError(f"{what} failed (code {rc}): {msg}")


class Tune(enum.IntEnum):
    """enum bg_tune_key of include/brepgen_hip.h, which describes every key (0 always = the library's own choice)"""
    GEMM_STAGGER = 8
    P256_MODE = 10
    SPLIT_PIPE = 12
    QKV_ATTN = 13
    QKV_WALK = 14
    SMALL_TILES = 15
    FFN_FUSED = 16
    VAE_GN1_FUSED = 19
    ATTN_WALK = 20


_tuned = {}        # Tune -> the value in force, of every key this process has set (the library starts with 0 everywhere and has no getter:
#                    _tune_set below is the only caller of bg_tune_set with a valid key on the package's library -- a tripwire in
#                    tests/test_abi_cpu.py -- so the record is exact)


def _tune_key(key):
    """Tune of a member, its name, its number or the number as a string"""
    try:
        return Tune(int(key)) if isinstance(key, int) or key.lstrip("-").isdigit() else Tune[key]
    except (KeyError, ValueError):
        raise BrepgenHipError(f"bg_tune: unknown key {key!r} (the keys: {', '.join(f'{k.name} = {int(k)}' for k in Tune)})") from None


def _tune_set(key, value):
    key = _tune_key(key)
    check(load().bg_tune_set(int(key), int(value)), f"bg_tune_set({key.name}, {value})")
    _tuned[key] = int(value)


def parse_tune(text):
    """"P256_MODE=2,13=1" -> {Tune.P256_MODE: 2, Tune.QKV_ATTN: 1}: the one parser of BG_TUNE and of the tools' command lines"""
    return {_tune_key(k.strip()): int(v) for k, v in (kv.split("=") for kv in filter(None, text.split(",")))}


@contextlib.contextmanager
def tune(parsed=(), **settings):
    """`with tune(P256_MODE=2, SMALL_TILES=-1): ...` (or `with tune(parse_tune(text)): ...`) -- kernel-selection knobs (process-global)
    for the length of a block.  Yields the setter `set_key(key, value)` for further changes inside the block; on exit, by exception
    too, EVERY key is back at the value that was in force on entry, so blocks nest."""
    entry = dict(_tuned)
    try:
        for key, value in {**dict(parsed), **settings}.items():
            _tune_set(key, value)
        yield _tune_set
    finally:
        for key, value in list(_tuned.items()):
            if value != entry.get(key, 0):
                _tune_set(key, entry.get(key, 0))


def ptr(t):
    """Device (or host, for CPU-side tests of argument checking) address of a contiguous tensor, or None."""
    if t is None:
        return None
    assert t.is_contiguous(), "libbrepgen_hip takes dense row-major tensors"
    return t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class profile:
    """Context manager around bg_profile_begin/end: `with profile() as p: ...; p.rows` -> list of dicts."""

    def __init__(self, max_launches=20000):
        self.max_launches, self.rows = max_launches, []

    def __enter__(self):
        check(load().bg_profile_begin(self.max_launches), "bg_profile_begin")
        return self

    def __exit__(self, *exc):
        buf = (ProfileRow * 16)()
        n = load().bg_profile_end(buf, 16)
        if n < 0:
            check(n, "bg_profile_end")
        self.rows = [{"kernel": buf[i].kernel.decode(), "launches": buf[i].launches, "total_ms": buf[i].total_ms,
                      "flops": buf[i].flops, "bytes": buf[i].bytes} for i in range(n)]
        return False
