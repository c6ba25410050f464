"""ctypes binding of ``libbya_hip.so`` (C ABI declared in ``include/bya.h``).

Loading fails LOUDLY: there is no CPU / PyTorch fallback for the product path.
"""
import ctypes
import os

from .build import LIB_PATH as _BUILT_LIB

# tools/ A/B runs may point at a side build of the same library (never set in production)
LIB_PATH = os.environ.get("BYA_HIP_LIB") or _BUILT_LIB

_c = ctypes
_vp, _i32, _i64, _f32 = _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_float


class GemmDesc(_c.Structure):
    _fields_ = [("M", _i32), ("N", _i32), ("K", _i32), ("batch", _i32),
                ("lda", _i32), ("ldw", _i32), ("ldc", _i32), ("ldres", _i32),
                ("a_batch_stride", _i64), ("c_batch_stride", _i64), ("res_batch_stride", _i64),
                ("gate_batch_stride", _i64), ("gate_split", _i32), ("act", _i32),
                ("n_split", _i32), ("c_split_stride", _i64), ("bias_rowscale", _vp), ("alpha", _f32)]


class GemmPlan(_c.Structure):
    _fields_ = [("path", _i32), ("m0", _i32), ("tail", _i32), ("split_k", _i32), ("row_chunks", _i32)]


class QkNormDesc(_c.Structure):
    _fields_ = [("qw", _vp), ("qb", _vp), ("kw", _vp), ("kb", _vp), ("cos", _vp), ("sin", _vp),
                ("text_rows", _i32), ("width", _i32), ("eps", _f32), ("k_scale", _f32)]


MX_KERNEL_FP6 = 16      # BYA_MX_KERNEL_FP6: flag bit of MxGemmCall.kernel (mxfp6 operands / output may take path "p256")


class MxGemmCall(_c.Structure):
    """bya_mx_gemm_call: the operands, epilogue and kernel of one bya_gemm_mx_call (kernel: 0, 1, 2, or MX_KERNEL_FP6 + one of
    them)."""
    _fields_ = [("A", _vp), ("a_scales", _vp), ("W", _vp), ("w_scales", _vp), ("bias", _vp), ("C", _vp),
                ("res", _vp), ("gate0", _vp), ("gate1", _vp), ("q_scales", _vp), ("norm", _c.POINTER(QkNormDesc)),
                ("a_fmt", _i32), ("w_fmt", _i32), ("out_fmt", _i32), ("kernel", _i32)]


class AttnDesc(_c.Structure):
    _fields_ = [("head_dim", _i32), ("heads", _i32), ("nb1", _i32), ("nb2", _i32), ("Sq", _i32), ("Skv", _i32),
                ("q_s1", _i64), ("q_s2", _i64), ("q_row", _i64),
                ("k_s1", _i64), ("k_s2", _i64), ("k_row", _i64),
                ("v_s1", _i64), ("v_s2", _i64), ("v_row", _i64),
                ("o_s1", _i64), ("o_s2", _i64), ("o_row", _i64),
                ("scale", _f32), ("scores_prescaled", _i32), ("score_bound", _f32),
                ("bound_dev", _vp), ("bound_slots", _i32), ("bound_heads", _i32), ("bound_bh0", _i32), ("fallback_flags", _vp)]


class AttnMixDesc(_c.Structure):
    _fields_ = [("head_dim", _i32), ("heads", _i32), ("n_id", _i32), ("n_grp", _i32), ("Sq", _i32), ("Skv", _i32),
                ("q_grp", _i64), ("q_row", _i64), ("k_id", _i64), ("k_grp", _i64), ("k_row", _i64),
                ("v_id", _i64), ("v_grp", _i64), ("v_row", _i64), ("z_grp", _i64), ("z_row", _i64), ("scale", _f32)]


MIX_MAX_SEGMENTS = 16   # BYA_MIX_MAX_SEGMENTS


class AttnMixSegments(_c.Structure):
    """bya_attn_mix_segments: the table of bya_attn_kv_mix_seg / _mx_seg, (K / V group, first row, rows) per segment."""
    _fields_ = [("n", _i32), ("grp", _i32 * MIX_MAX_SEGMENTS), ("start", _i32 * MIX_MAX_SEGMENTS), ("len", _i32 * MIX_MAX_SEGMENTS)]


class AttnMixSamples(_c.Structure):
    """bya_attn_mix_samples: n and the distance from one sample to the next of every pointer of bya_attn_kv_mix_batch (elements)."""
    _fields_ = [("n", _i32), ("reserved", _i32), ("q", _i64), ("k", _i64), ("v", _i64), ("r", _i64), ("af", _i64), ("z", _i64),
                ("wsum", _i64)]


class AttnMixMxSamples(_c.Structure):
    """bya_attn_mix_mx_samples: the same for bya_attn_kv_mix_mx_batch (codes, scales: bytes)."""
    _fields_ = [("n", _i32), ("reserved", _i32), ("q", _i64), ("k", _i64), ("v", _i64), ("r", _i64), ("af", _i64), ("codes", _i64),
                ("scales", _i64), ("wsum", _i64)]


class RouterScoresSamples(_c.Structure):
    """bya_router_scores_samples (bya_router_scores_batch)."""
    _fields_ = [("n", _i32), ("reserved", _i32), ("qr", _i64), ("kr", _i64), ("out", _i64)]


class RouterHeadSamples(_c.Structure):
    """bya_router_head_samples (bya_router_head_batch)."""
    _fields_ = [("n", _i32), ("reserved", _i32), ("x", _i64), ("r", _i64)]


class AttnPlan(_c.Structure):
    _fields_ = [("variant", _i32), ("grid", _i32), ("q_tile", _i32), ("stream_k", _i32), ("sk_rem", _i32), ("sk_cut", _i32),
                ("o_wide", _i32), ("second_launch", _i32)]


class AttnMixPlan(_c.Structure):
    _fields_ = [("form", _i32), ("head_dim", _i32), ("grid", _i32), ("row_chunks", _i32), ("lds_bytes", _i32), ("big_lds", _i32)]


class AttnTinyPlan(_c.Structure):
    _fields_ = [("instance", _i32), ("grid", _i32), ("waves", _i64)]


class RowGemmPlan(_c.Structure):
    _fields_ = [("form", _i32), ("ln", _i32), ("res", _i32), ("act", _i32), ("grid", _i32), ("crosses_row_block", _i32),
                ("work_items", _i64)]


class GroupAttnPlan(_c.Structure):
    _fields_ = [("P", _i32), ("G", _i32), ("wide", _i32), ("blocks", _i32), ("tiles", _i64)]


class LayerNormPlan(_c.Structure):
    _fields_ = [("kernel", _i32), ("vec", _i32), ("nv", _i32), ("modulated", _i32), ("rows_per_wave", _i32), ("grid", _i32),
                ("waves", _i64)]


class QkNormRopePlan(_c.Structure):
    _fields_ = [("stats", _i32), ("only", _i32), ("grid", _i32), ("slots", _i32), ("pairs", _i64), ("waves", _i64)]


class RouterChainPlan(_c.Structure):
    _fields_ = [("tiles", _i32), ("tp0", _i32), ("grid", _i32), ("passes", _i32), ("tiles_last", _i32), ("wgs_last", _i32)]


class StepPlan(_c.Structure):
    """bya_step_plan_info: the plan of bya_linear_small_m / bya_router_scores / bya_act_add / bya_cfg_scheduler_step."""
    _fields_ = [("kernel", _i32), ("grid", _i32), ("rounds", _i32), ("reserved", _i32), ("items", _i64), ("items_per_round", _i64)]


class StepCachePlan(_c.Structure):
    """bya_step_cache_plan_info: the grid the probe, the capture and the apply share, and the probe's partials."""
    _fields_ = [("grid", _i32), ("vec", _i32), ("wg_pass_elems", _i32), ("passes", _i32), ("partials_bytes", _i64)]


class SchedCoef(_c.Structure):
    _fields_ = [("guidance", _f32), ("sqrt_alpha", _f32), ("sqrt_beta", _f32), ("k_sample", _f32),
                ("k_denoised", _f32), ("k_noise", _f32), ("k_cur", _f32), ("k_old", _f32)]


# name -> argtypes (all return int32 status); mirrors include/bya.h one-to-one
SIGNATURES = {
    "bya_abi_version": [],
    "bya_set_option": [_i32, _i32],
    "bya_get_option": [_i32, _c.POINTER(_i32)],
    "bya_mfma_calibration": [_vp, _i64, _vp, _i32, _vp],
    "bya_gemm_bf16": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _vp],
    "bya_gemm_skinny_bf16": [_vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _vp],
    "bya_gemm_qkv_norm_rope": [_vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _vp],
    "bya_gemm_bf16_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(GemmPlan)],
    "bya_gemm_qkv_norm_rope_plan": [_vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _c.POINTER(GemmPlan)],
    "bya_gemm_qkv_norm_rope_stats": [_vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _vp, _i32, _vp],
    "bya_gemm_qkv_norm_rope_stats_plan": [_vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _vp, _i32, _c.POINTER(GemmPlan)],
    "bya_set_gemm_workspace": [_vp, _i64],
    "bya_gemm_workspace_bytes": [_c.POINTER(_i64)],
    "bya_gemm_workspace_status": [_c.POINTER(_i32), _vp],
    "bya_quantize_rows_fp8": [_vp, _vp, _vp, _i32, _i32, _i64, _i64, _vp],
    "bya_gemm_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _vp],
    "bya_gemm_fp8_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(GemmPlan)],
    "bya_gemm_fp8_qkv_norm_rope": [_vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _vp],
    "bya_gemm_fp8_qkv_norm_rope_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc),
                                        _c.POINTER(GemmPlan)],
    "bya_gemm_fp8_qkv_norm_rope_stats": [_vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _vp, _i32, _vp],
    "bya_gemm_fp8_qkv_norm_rope_stats_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _vp, _i32,
                                              _c.POINTER(GemmPlan)],
    "bya_layernorm_fp8": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _i64, _i64, _i64, _i64, _i64,
                          _f32, _vp],
    "bya_quantize_mx": [_vp, _vp, _vp, _i32, _i32, _i64, _i32, _vp],
    "bya_layernorm_mx": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _i64, _i64, _i64, _i64, _i64,
                         _f32, _i32, _vp],
    "bya_gemm_mx": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _i32, _vp],
    "bya_gemm_mx_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _i32, _c.POINTER(GemmPlan)],
    "bya_gemm_mx_mixed": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _i32, _i32, _vp],
    "bya_gemm_mx_mixed_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _i32, _i32,
                               _c.POINTER(GemmPlan)],
    "bya_gemm_mx_quant": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _i32, _i32, _i32, _vp],
    "bya_gemm_mx_quant_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(GemmDesc), _i32, _i32, _i32,
                               _c.POINTER(GemmPlan)],
    "bya_gemm_mx_qkv_norm_rope": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _vp],
    "bya_gemm_mx_qkv_norm_rope_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc),
                                       _c.POINTER(GemmPlan)],
    "bya_gemm_mx_qkv_norm_rope_on": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _i32,
                                     _vp],
    "bya_gemm_mx_qkv_norm_rope_on_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc),
                                          _i32, _c.POINTER(GemmPlan)],
    "bya_gemm_mx_qkv_norm_rope_stats": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _i32, _vp, _i32, _vp],
    "bya_gemm_mx_qkv_norm_rope_stats_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _c.POINTER(GemmDesc), _c.POINTER(QkNormDesc), _i32, _vp, _i32,
                                             _c.POINTER(GemmPlan)],
    "bya_gemm_mx_call": [_c.POINTER(MxGemmCall), _c.POINTER(GemmDesc), _vp],
    "bya_gemm_mx_call_plan": [_c.POINTER(MxGemmCall), _c.POINTER(GemmDesc), _c.POINTER(GemmPlan)],
    "bya_linear_small_m": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "bya_linear_small_m_plan": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _c.POINTER(StepPlan)],
    "bya_timestep_features": [_vp, _vp, _i32, _i32, _i32, _f32, _vp],
    "bya_layernorm": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _i64, _i64, _i64, _i64, _i64,
                      _f32, _vp],
    "bya_layernorm_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i64, _i64, _i64, _i64, _i64, _i64,
                           _i32, _c.POINTER(LayerNormPlan)],
    "bya_qknorm_rope_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _i64, _i32, _vp, _i32,
                             _c.POINTER(QkNormRopePlan)],
    "bya_qknorm_rope": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _i64, _i32, _f32, _f32, _vp, _i32, _vp],
    "bya_attn_fwd": [_vp, _vp, _vp, _vp, _c.POINTER(AttnDesc), _vp],
    "bya_attn_variant": [_c.POINTER(AttnDesc)],
    "bya_attn_plan": [_c.POINTER(AttnDesc), _vp, _i32, _c.POINTER(AttnPlan)],
    "bya_attn_fwd_mx": [_vp, _vp, _vp, _vp, _vp, _c.POINTER(AttnDesc), _i32, _i64, _i64, _i64, _i64, _i64, _i64, _vp],
    "bya_attn_mx_plan": [_c.POINTER(AttnDesc), _vp, _vp, _i32, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _c.POINTER(AttnPlan)],
    "bya_set_attn_workspace": [_vp, _i64],
    "bya_attn_workspace_bytes": [_c.POINTER(_i64)],
    "bya_attn_workspace_status": [_c.POINTER(_i32), _vp],
    "bya_attn_kv_mix": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(AttnMixDesc), _vp],
    "bya_attn_kv_mix_plan": [_vp, _vp, _c.POINTER(AttnMixDesc), _c.POINTER(AttnMixPlan)],
    "bya_attn_kv_mix_mx": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(AttnMixDesc), _i32, _i64, _i64, _i64, _i64, _vp],
    "bya_attn_kv_mix_mx_plan": [_vp, _vp, _vp, _c.POINTER(AttnMixDesc), _i32, _i64, _i64, _i64, _i64, _c.POINTER(AttnMixPlan)],
    "bya_attn_kv_mix_seg": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(AttnMixDesc), _c.POINTER(AttnMixSegments), _vp],
    "bya_attn_kv_mix_seg_plan": [_vp, _vp, _c.POINTER(AttnMixDesc), _c.POINTER(AttnMixSegments), _c.POINTER(AttnMixPlan)],
    "bya_attn_kv_mix_mx_seg": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(AttnMixDesc), _c.POINTER(AttnMixSegments), _i32,
                               _i64, _i64, _i64, _i64, _vp],
    "bya_attn_kv_mix_mx_seg_plan": [_vp, _vp, _vp, _c.POINTER(AttnMixDesc), _c.POINTER(AttnMixSegments), _i32, _i64, _i64, _i64,
                                    _i64, _c.POINTER(AttnMixPlan)],
    "bya_attn_kv_mix_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(AttnMixDesc), AttnMixSamples, _vp],
    "bya_attn_kv_mix_batch_plan": [_vp, _vp, _c.POINTER(AttnMixDesc), AttnMixSamples, _c.POINTER(AttnMixPlan)],
    "bya_attn_kv_mix_mx_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(AttnMixDesc), _i32, _i64, _i64, _i64, _i64,
                                 AttnMixMxSamples, _vp],
    "bya_attn_kv_mix_mx_batch_plan": [_vp, _vp, _vp, _c.POINTER(AttnMixDesc), _i32, _i64, _i64, _i64, _i64, AttnMixMxSamples,
                                      _c.POINTER(AttnMixPlan)],
    "bya_attn_tiny": [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp],
    "bya_attn_tiny_plan": [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i64, _i64, _c.POINTER(AttnTinyPlan)],
    "bya_router_scores": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _vp],
    "bya_router_scores_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _c.POINTER(StepPlan)],
    "bya_router_head": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp],
    "bya_router_scores_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, RouterScoresSamples, _vp],
    "bya_router_scores_batch_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, RouterScoresSamples, _c.POINTER(StepPlan)],
    "bya_router_head_batch": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, RouterHeadSamples, _vp],
    "bya_router_head_batch_plan": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, RouterHeadSamples, _c.POINTER(StepPlan)],
    "bya_forcing_max_over_frames": [_vp, _vp, _i32, _i64, _i32, _vp],
    "bya_masked_combine": [_vp, _vp, _vp, _vp, _i32, _f32, _i32, _i32, _i64, _i32, _i64, _i64, _i64, _vp],
    "bya_routed_mix": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _i32, _i64, _vp],
    "bya_patchify": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "bya_unpatchify": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "bya_act_add": [_vp, _vp, _vp, _i64, _i32, _vp],
    "bya_act_add_plan": [_vp, _vp, _vp, _i64, _i32, _c.POINTER(StepPlan)],
    "bya_step_cache_probe": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "bya_step_cache_probe_plan": [_vp, _vp, _vp, _vp, _i64, _c.POINTER(StepCachePlan)],
    "bya_step_cache_capture": [_vp, _vp, _vp, _i64, _vp],
    "bya_step_cache_apply": [_vp, _vp, _i64, _vp],
    "bya_rowgemm512": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp],
    "bya_rowgemm512_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c.POINTER(RowGemmPlan)],
    "bya_router_group_attn_plan": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64,
                                   _c.POINTER(GroupAttnPlan)],
    "bya_router_mlp_fused_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _c.POINTER(RouterChainPlan)],
    "bya_router_group_attn_out_plan": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _i32,
                                       _c.POINTER(RouterChainPlan)],
    "bya_router_group_attn": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _f32, _f32, _vp],
    "bya_router_mlp_fused": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _i32, _vp],
    "bya_router_group_attn_out": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _f32, _f32,
                                  _i32, _vp],
    "bya_masks_to_routing_logits": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp],
    "bya_vae_patches": [_vp, _vp, _vp] + [_i32] * 14 + [_vp],
    "bya_vae_groupnorm_stats": [_vp, _vp, _vp, _i64, _i32, _i32, _vp],
    "bya_vae_norm_act": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _i32, _i32, _i32,
                         _i32, _i64, _i32, _vp],
    "bya_vae_groupnorm_moments": [_vp, _vp, _vp, _i64, _i32, _i32, _vp],
    "bya_vae_norm_act_moments": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _i32, _i32, _i32,
                                 _i32, _i64, _i32, _vp],
    "bya_vae_conv3d": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _vp],
    "bya_vae_upsample_pad": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp],
    "bya_allgather_kv": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "bya_alltoall_router": [_vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "bya_p2p_push": [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp],
    "bya_p2p_wait": [_vp, _i32, _vp, _i64, _vp],
    "bya_p2p_exchange": [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _i64, _vp],
    "bya_p2p_push_verified": [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "bya_p2p_exchange_verified": [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "bya_p2p_verify": [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp],
    "bya_p2p_poison": [_vp, _i32, _vp, _i64, _vp],
    "bya_p2p_alloc": [_i64, _i32, _c.POINTER(_vp)],
    "bya_p2p_free": [_vp],
    "bya_p2p_ipc_export": [_vp, _vp],
    "bya_p2p_ipc_import": [_vp, _c.POINTER(_vp)],
    "bya_p2p_ipc_release": [_vp],
    "bya_cfg_scheduler_step": [_vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _c.POINTER(SchedCoef), _vp],
    "bya_cfg_scheduler_step_plan": [_vp, _i32, _i64, _vp, _vp, _i64, _c.POINTER(SchedCoef), _c.POINTER(StepPlan)],
}

# bya_option keys / BYA_REF_* bits of include/bya.h
OPTIONS = {"gemm_splitk": 0, "gemm_splitk_min": 1, "gemm_tile": 2, "gemm_variant": 3, "attn_streamk": 4, "fp8_kernel": 5,
           "p2p_groups": 6, "reference_forms": 7, "mx_kernel": 8}
REFERENCE_FORMS = {"rowgemm_chunked": 1, "kv_mix_generic": 2, "ln_generic": 4, "router_scores_wave": 8, "attn_narrow_store": 16}
def _named_value(var, v, table):
    """The option value a variable's text stands for; an unknown text is an error, not a silent default."""
    if v not in table:
        raise ValueError(f"{var}={v!r}: expected one of {sorted(table)}")
    return table[v]


# environment variable -> (option, parser): read ONCE, when the library is loaded (the C entry points never call getenv)
ENV_OPTIONS = {
    "BYA_GEMM_SPLITK": ("gemm_splitk", int),
    "BYA_GEMM_SPLITK_MIN": ("gemm_splitk_min", int),
    "BYA_GEMM_TILE": ("gemm_tile", int),
    "BYA_GEMM_VARIANT": ("gemm_variant", lambda v: {"w8": 1, "no128": 2}.get(v, 0)),
    "BYA_ATTN_STREAMK": ("attn_streamk", int),
    "BYA_FP8_KERNEL": ("fp8_kernel", lambda v: 1 if v.startswith("1") else 0),
    "BYA_P2P_GROUPS": ("p2p_groups", int),
    "BYA_MX_KERNEL": ("mx_kernel", lambda v: _named_value("BYA_MX_KERNEL", v, {"0": 0, "1": 1, "p256": 1, "2": 2, "always": 2})),
}

# BYA_GEMM_PATH_* of include/bya.h: the kernels of a GEMM launch (bya_gemm_plan.path / .tail)
GEMM_PATHS = {0: "t128x64", 1: "t128x128", 2: "t256x128", 3: "t256x256", 4: "p256", 5: "p128", 6: "p128s", 7: "w8_256"}

# BYA_ATTN_* / BYA_KV_MIX_* / BYA_TINY* of include/bya.h: the kernels of the attention launches (the *_plan queries)
ATTN_VARIANTS = {0: "d64_running_max", 1: "d64_prescaled_running_max", 2: "d64_static_bound", 3: "d128_running_max",
                 4: "d64_static_bound_w4", 5: "d64_device_bound_w4"}
KV_MIX_FORMS = {0: "mix32", 1: "one_tile"}
TINY_INSTANCES = {0: "tiny8<2>", 1: "tiny8<3>", 2: "tiny8<13>", 3: "tiny8<25>", 4: "generic<2>", 5: "generic<4>",
                  6: "generic<16>", 7: "generic<32>"}

ROWGEMM_FORMS = {0: "chunk_balanced", 1: "w_stationary"}       # BYA_ROWGEMM_* (bya_rowgemm512_plan)

ROUTER_SCORES_KERNELS = {0: "wave", 1: "lds"}                   # BYA_ROUTER_SCORES_* (bya_router_scores_plan)

LN_KERNELS = {0: "generic", 1: "rows"}                          # BYA_LN_KERNEL_* (bya_layernorm_plan)
LN_OUT_KINDS = {"bf16": 0, "fp8": 1, "mxfp8": 2, "mxfp6": 3}    # BYA_LN_OUT_*

ERRORS = {-1: "BYA_ERR_SHAPE", -2: "BYA_ERR_ALIGN", -3: "BYA_ERR_LAUNCH", -4: "BYA_ERR_UNSUPPORTED"}

_lib = None


def load():
    """Load the HIP library; raises if it is not built (run ``python -m ...build`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    # ONE HIP runtime per process: torch must map its (bundled) libamdhip64 first so that this library binds to
    # the same runtime that owns torch's device pointers and streams.  Loading in the other order gives two
    # runtimes and hipErrorNoDevice at the first launch.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the Bind-Your-Avatar MI355X engine has no fallback path. "
            "Build it with `python -m bind_your_avatar_implementation_amd.build`.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export what bya.h declares
        fn.argtypes = argtypes
        fn.restype = _i32
    _lib = lib
    apply_env_options()
    return lib


def set_option(name, value):
    """bya_set_option by name (``OPTIONS``); raises on an unknown name or a value outside the option's range."""
    check(load().bya_set_option(OPTIONS[name], int(value)), f"bya_set_option({name}={value})")


def get_option(name):
    v = _i32(0)
    check(load().bya_get_option(OPTIONS[name], _c.byref(v)), f"bya_get_option({name})")
    return v.value


OPTION_DEFAULTS = {"gemm_splitk": 0, "gemm_splitk_min": 0, "gemm_tile": -1, "gemm_variant": 0, "attn_streamk": 1, "fp8_kernel": 0,
                   "p2p_groups": 0, "reference_forms": 0, "mx_kernel": 0}


def apply_env_options():
    """Hand the BYA_* tuning variables of the environment to the library's option table; an option whose variable is unset
    goes back to its default.  Runs when the library is loaded; call it again after changing one of the variables in a live
    process (tools/ do)."""
    for var, (name, parse) in ENV_OPTIONS.items():
        v = os.environ.get(var)
        set_option(name, parse(v) if v not in (None, "") else OPTION_DEFAULTS[name])


class ByaError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise ByaError(f"{what} failed: {ERRORS.get(rc, rc)}")
