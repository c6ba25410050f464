"""Drop-in replacement for the reference denoiser ``BindyouravatarTransformer3DModel``.

Same constructor keywords (reference models/transformer.py:322-366), same state-dict key names and
shapes (checked against ``tests/golden/ref_state_dict_keys.json``, dumped from the reference class), same
``forward`` signature and 5-tuple return (models/transformer.py:615-633, 963-964).  The modules below are
parameter CONTAINERS only: nothing here computes with torch ops -- ``forward`` hands the tensors to
``engine.DenoiseEngine`` which runs the step on the hand-written HIP kernels of ``libbya_hip.so``.
There is no CPU / eager fallback: calling ``forward`` without a GPU or without the built library raises.
"""
from types import SimpleNamespace
from typing import Any, Dict, NamedTuple, Optional, Tuple, Union

import os
import torch
from torch import nn


class GraphEntry(NamedTuple):
    """One captured step of ``_graphed_step``: the graph, its static input buffers and output, and what it keeps alive -- the
    workspace its launches point into, the engine, and (``cache_hold``: None for a graph that recomputes the conditioning) the
    entries of the engine's conditioning cache it reads in place.  The engine drops entries with a ``cache_hold`` together with
    the cache they were captured against."""
    graph: Any
    static: list
    static_out: Any
    ws: Any
    engine: Any
    cache_hold: Any


# ------------------------------------------------------------------------------------------ containers
class _Lin(nn.Module):
    def __init__(self, i, o, bias=True, **fk):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(o, i, **fk), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.empty(o, **fk), requires_grad=False)
        else:
            self.register_parameter("bias", None)


class _LN(nn.Module):
    def __init__(self, d, eps=1e-5, affine=True, **fk):
        super().__init__()
        self.eps = eps
        if affine:
            self.weight = nn.Parameter(torch.empty(d, **fk), requires_grad=False)
            self.bias = nn.Parameter(torch.empty(d, **fk), requires_grad=False)
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)


class _Conv(nn.Module):
    def __init__(self, shape, **fk):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*shape, **fk), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(shape[0], **fk), requires_grad=False)


def _seq(*mods):
    """nn.Sequential-style numbering ('0', '1', ...) with None -> parameter-free placeholder."""
    return nn.ModuleList([m if m is not None else nn.Identity() for m in mods])


class _Attn(nn.Module):
    """Key layout of diffusers ``Attention`` (to_q/to_k/to_v/to_out.0[/norm_q/norm_k])."""

    def __init__(self, q_dim, inner, kv_dim=None, bias=True, qk_norm_dim=None, qk_eps=1e-6, **fk):
        super().__init__()
        kv_dim = q_dim if kv_dim is None else kv_dim
        self.to_q = _Lin(q_dim, inner, bias, **fk)
        self.to_k = _Lin(kv_dim, inner, bias, **fk)
        self.to_v = _Lin(kv_dim, inner, bias, **fk)
        if qk_norm_dim:
            self.norm_q = _LN(qk_norm_dim, qk_eps, **fk)
            self.norm_k = _LN(qk_norm_dim, qk_eps, **fk)
        self.to_out = _seq(_Lin(inner, q_dim, True, **fk), None)


class _NormZero(nn.Module):
    def __init__(self, cond, dim, eps, affine, chunks, **fk):
        super().__init__()
        self.linear = _Lin(cond, chunks * dim, True, **fk)
        self.norm = _LN(dim, eps, affine, **fk)


class _Block(nn.Module):
    def __init__(self, dim, heads, head_dim, temb, eps, affine, attn_bias, **fk):
        super().__init__()
        self.norm1 = _NormZero(temb, dim, eps, affine, 6, **fk)
        self.attn1 = _Attn(dim, heads * head_dim, bias=attn_bias, qk_norm_dim=head_dim, **fk)
        self.norm2 = _NormZero(temb, dim, eps, affine, 6, **fk)
        self.ff = nn.Module()
        gelu = nn.Module()
        gelu.proj = _Lin(dim, 4 * dim, True, **fk)
        self.ff.net = _seq(gelu, None, _Lin(4 * dim, dim, True, **fk), None)


class _PatchEmbed(nn.Module):
    def __init__(self, in_ch, dim, text_dim, patch, n_rows, learned, **fk):
        super().__init__()
        self.proj = _Conv((dim, in_ch, patch, patch), **fk)
        self.text_proj = _Lin(text_dim, dim, True, **fk)
        self.register_buffer("pos_embedding", torch.zeros(1, n_rows, dim, **fk), persistent=learned)


class _Perceiver(nn.Module):
    def __init__(self, dim, inner, kv_dim=None, **fk):
        super().__init__()
        self.norm1 = _LN(dim if kv_dim is None else kv_dim, **fk)
        self.norm2 = _LN(dim, **fk)
        self.to_q = _Lin(dim, inner, False, **fk)
        self.to_kv = _Lin(dim if kv_dim is None else kv_dim, 2 * inner, False, **fk)
        self.to_out = _Lin(inner, dim, False, **fk)


def _mapper(d_in, d_out, **fk):
    return _seq(_Lin(d_in, 1024, **fk), _LN(1024, **fk), None, _Lin(1024, 1024, **fk), _LN(1024, **fk), None,
                _Lin(1024, d_out, **fk))


class _LFE(nn.Module):
    """LocalFacialExtractor parameters (reference models/router.py:78-155)."""

    def __init__(self, dim=1024, depth=10, dim_head=64, heads=16, num_id_token=5, num_queries=32, output_dim=2048,
                 ff_mult=4, **fk):
        super().__init__()
        self.dim, self.depth, self.heads, self.dim_head = dim, depth // 5, heads, dim_head
        self.num_id_token, self.num_queries = num_id_token, num_queries
        self.latents = nn.Parameter(torch.empty(1, num_queries, dim, **fk), requires_grad=False)
        self.proj_out = nn.Parameter(torch.empty(dim, output_dim, **fk), requires_grad=False)
        self.layers = nn.ModuleList([
            _seq(_Perceiver(dim, dim_head * heads, **fk),
                 _seq(_LN(dim, **fk), _Lin(dim, dim * ff_mult, False, **fk), None, _Lin(dim * ff_mult, dim, False, **fk)))
            for _ in range(depth)])
        for i in range(5):
            setattr(self, f"mapping_{i}", _mapper(1024, dim, **fk))
        self.id_embedding_mapping = _mapper(1280, dim * num_id_token, **fk)


class _STBlock(nn.Module):
    def __init__(self, dim, **fk):
        super().__init__()
        self.spatial_attn = _Attn(dim, dim, **fk)
        self.temporal_attn = _Attn(dim, dim, **fk)
        self.multi_id_attn = _Attn(dim, dim, **fk)
        self.norm1, self.norm2, self.norm3, self.norm4 = (_LN(dim, **fk) for _ in range(4))
        self.mlp = _seq(_Lin(dim, dim, **fk), None, _Lin(dim, dim, **fk))


class _Router(nn.Module):
    """MultiIPRouter parameters (reference models/router.py:280-332); ``layer_merge`` is dead but loadable."""

    def __init__(self, num_layers, frames, height, width, q_k_dim=2048, num_id_token=32, num_heads=16, **fk):
        super().__init__()
        wdim = num_id_token * num_heads
        self.heads, self.feat_dim = num_heads, wdim
        self.frames, self.height, self.width = frames, height, width
        self.norm = _LN(wdim, **fk)
        self.norm_q, self.norm_k = _LN(q_k_dim, **fk), _LN(q_k_dim, **fk)
        self.to_q = nn.ModuleList([_Lin(q_k_dim, q_k_dim, False, **fk) for _ in range(num_layers)])
        self.to_k = nn.ModuleList([_Lin(q_k_dim, q_k_dim, False, **fk) for _ in range(num_layers)])
        self.layer_merge = nn.ModuleList([_seq(_Lin(wdim + 3, 256, True, **fk), None, _Lin(256, 128, False, **fk), None)
                                          for _ in range(num_layers)])
        self.register_buffer("pos_emb", router_pos_emb(frames, height, width, wdim).to(**fk))
        self.spatial_temporal_layers = nn.ModuleList([_STBlock(wdim, **fk) for _ in range(4)])
        self.final_proj = _seq(_Lin(wdim, 1, **fk), None)


def router_pos_emb(frames, height, width, feat_dim):
    """3-D sin/cos table of the router (reference models/router.py:334-362), index [t, a, b, :]."""
    third = feat_dim // 3
    div = torch.pow(10000, torch.arange(0, third, 2).float() / third)

    def axis(n):
        e = torch.arange(n).float().unsqueeze(-1) / div
        return torch.stack([torch.sin(e), torch.cos(e)], dim=-1).flatten(-2)

    t = axis(frames)[:, None, None, :].expand(-1, height, width, -1)
    h = axis(height)[None, :, None, :].expand(frames, -1, width, -1)
    w = axis(width)[None, None, :, :].expand(frames, height, -1, -1)
    pe = torch.cat([t, h, w], dim=-1)
    if pe.size(-1) < feat_dim:
        pe = torch.cat([pe, torch.zeros(frames, height, width, feat_dim - pe.size(-1))], dim=-1)
    return pe.contiguous()


class _AudioProj(nn.Module):
    def __init__(self, seq_len=5, blocks=12, channels=768, intermediate_dim=512, output_dim=768, context_tokens=32, **fk):
        super().__init__()
        self.seq_len, self.blocks, self.channels = seq_len, blocks, channels
        self.context_tokens, self.output_dim = context_tokens, output_dim
        self.proj1 = _Lin(seq_len * blocks * channels, intermediate_dim, **fk)
        self.proj2 = _Lin(intermediate_dim, intermediate_dim, **fk)
        self.proj3 = _Lin(intermediate_dim, context_tokens * output_dim, **fk)
        self.norm = _LN(output_dim, **fk)
        self.conv1 = _Conv((context_tokens * output_dim, context_tokens * output_dim, 2), **fk)


class _AudioLayer(nn.ModuleDict):
    pass


class _AudioModel(nn.Module):
    def __init__(self, dim, heads, head_dim, eps, affine, num_layers, audio_dim=768, **fk):
        super().__init__()
        self.window_size, self.window_stride = 5, 1
        self.learnable_scale = nn.Parameter(torch.empty(1, **fk), requires_grad=False)
        self.audio_proj_model = _AudioProj(**fk)
        self.layers = nn.ModuleList([
            nn.ModuleDict({"norm_q": _LN(dim, eps, affine, **fk),
                           "attn": _Attn(dim, heads * head_dim, kv_dim=audio_dim, bias=True, **fk)})
            for _ in range(num_layers)])
        self.mute_learnable_tokens = nn.Parameter(torch.empty(1, 32, 768, **fk), requires_grad=False)
        # single-stream audio (models/audio_model.py:201-221): the "mute" embedding the reference loads from
        # tests/input/ae_mute.pt.  Set it with BindyouravatarTransformer3DModel.set_mute_audio_embeds(); left unset,
        # the same relative path is read, as in the reference
        self.mute_audio_embeds = None


# ------------------------------------------------------------------------------------------ the model
class BindyouravatarTransformer3DModel(nn.Module):
    """See module docstring.  Extra keyword-only arguments ``device`` / ``dtype`` place the parameters."""

    def __init__(
        self,
        num_attention_heads: int = 48,
        attention_head_dim: int = 64,
        in_channels: int = 16,
        out_channels: Optional[int] = 16,
        flip_sin_to_cos: bool = True,
        freq_shift: int = 0,
        time_embed_dim: int = 512,
        text_embed_dim: int = 4096,
        num_layers: int = 30,
        dropout: float = 0.0,
        attention_bias: bool = True,
        sample_width: int = 90,
        sample_height: int = 60,
        sample_frames: int = 49,
        patch_size: int = 2,
        temporal_compression_ratio: int = 4,
        max_text_seq_length: int = 226,
        activation_fn: str = "gelu-approximate",
        timestep_activation_fn: str = "silu",
        norm_elementwise_affine: bool = True,
        norm_eps: float = 1e-5,
        spatial_interpolation_scale: float = 1.875,
        temporal_interpolation_scale: float = 1.0,
        use_rotary_positional_embeddings: bool = False,
        use_learned_positional_embeddings: bool = False,
        is_train_face: bool = True,
        is_kps: bool = False,
        cross_attn_interval: int = 1,
        LFE_num_tokens: int = 32,
        LFE_output_dim: int = 768,
        LFE_heads: int = 12,
        local_face_scale: float = 1.0,
        is_train_audio: bool = False,
        audio_attn_interval: int = 1,
        draw_routing_logits: bool = False,
        draw_routing_logits_suffix: str = "default",
        draw_routing_logits_video_save_dir: str = None,
        draw_routing_logits_use_softmax: bool = True,
        debug_routing_logits: bool = False,
        debug_routing_logits_zeros: bool = False,
        debug_routing_logits_ones: bool = False,
        is_teacher_forcing: bool = False,
        *,
        device=None,
        dtype=torch.bfloat16,
    ):
        super().__init__()
        cfg = {k: v for k, v in locals().items() if k not in ("self", "__class__", "device", "dtype")}
        self.config = SimpleNamespace(**cfg)
        if not use_rotary_positional_embeddings and use_learned_positional_embeddings:
            raise ValueError(
                "There are no CogVideoX checkpoints available with disable rotary embeddings and learned positional "
                "embeddings. If you're using a custom model and/or believe this should be supported, please open an "
                "issue at https://github.com/huggingface/diffusers/issues.")
        if patch_size != 2 or attention_head_dim != 64 or activation_fn != "gelu-approximate" or not attention_bias:
            raise ValueError("the MI355X engine covers the CogVideoX-5B-I2V lineage only "
                             "(patch 2, head_dim 64, gelu-approximate, attention bias)")
        if debug_routing_logits or debug_routing_logits_zeros or debug_routing_logits_ones or is_teacher_forcing:
            raise ValueError("training / debug routing branches are outside the inference hot path")
        fk = dict(device=device, dtype=dtype)
        inner = num_attention_heads * attention_head_dim
        self.inner_dim = inner
        frames = (sample_frames - 1) // temporal_compression_ratio + 1
        ht, wt = sample_height // patch_size, sample_width // patch_size
        self.token_grid = (frames, ht, wt)

        self.patch_embed = _PatchEmbed(in_channels, inner, text_embed_dim, patch_size,
                                       max_text_seq_length + frames * ht * wt,
                                       use_learned_positional_embeddings, **fk)
        self.time_embedding = nn.Module()
        self.time_embedding.linear_1 = _Lin(inner, time_embed_dim, **fk)
        self.time_embedding.linear_2 = _Lin(time_embed_dim, time_embed_dim, **fk)
        self.transformer_blocks = nn.ModuleList([
            _Block(inner, num_attention_heads, attention_head_dim, time_embed_dim, norm_eps, norm_elementwise_affine,
                   attention_bias, **fk) for _ in range(num_layers)])
        self.norm_final = _LN(inner, norm_eps, norm_elementwise_affine, **fk)
        self.norm_out = _NormZero(time_embed_dim, inner, norm_eps, norm_elementwise_affine, 2, **fk)
        self.proj_out = _Lin(inner, patch_size * patch_size * out_channels, **fk)

        self.is_train_face, self.is_kps = is_train_face, is_kps
        self.is_train_audio = is_train_audio
        if is_train_face:
            self.cross_attn_interval = cross_attn_interval
            self.num_ca = num_layers // cross_attn_interval
            self.LFE_final_output_dim = int(inner / 3 * 2)
            self.local_face_scale = local_face_scale
            self.local_facial_extractor = _LFE(**fk)
            self.perceiver_cross_attention = nn.ModuleList([
                _Perceiver(inner, 128 * 16, kv_dim=self.LFE_final_output_dim, **fk) for _ in range(self.num_ca)])
            # the reference hard-codes (13, 45, 30); generalised as (frames, Wt, Ht) -- see DESIGN.md "geometry"
            self.router = _Router(self.num_ca, frames, wt, ht, **fk)
        if is_train_audio:
            self.audio_attn_interval = audio_attn_interval
            self.audio_model = _AudioModel(inner, num_attention_heads, attention_head_dim, norm_eps,
                                           norm_elementwise_affine, num_layers // audio_attn_interval, **fk)
        self._engine = None
        # opt-in: replay the whole step (about 3000 kernel launches) from one captured hipGraph per input signature
        self.use_hip_graph = False
        self._graphs = {}
        # opt-in, read when the engine is built (set it before the first call, or call invalidate_engine()): a batch of
        # B >= 2 samples runs the face / audio kv-mix and the router's scores and head as ONE launch per layer (BYA_BATCH_LAUNCHES)
        self.batch_launches = False
        self._step_cache = None        # enable_step_cache: the first-block step cache's policy and state (engine.StepCache)

    # ---- API the reference pipeline touches -------------------------------------------------------
    @property
    def device(self):
        return self.proj_out.weight.device

    @property
    def dtype(self):
        return self.proj_out.weight.dtype

    def fuse_qkv_projections(self):
        """Reference models/transformer.py:576-599.  The engine already reads q/k/v as one pass; no-op."""
        return None

    def unfuse_qkv_projections(self):
        return None

    def load_face_modules(self, path: str, strict: bool = True):
        """Reference models/transformer.py:493-501 (dict with LFE state + list of perceiver states)."""
        ckpt = torch.load(path, map_location=self.device)
        self.local_facial_extractor.load_state_dict(ckpt["local_facial_extractor"], strict=strict)
        for ca, sd in zip(self.perceiver_cross_attention, ckpt["perceiver_cross_attention"]):
            ca.load_state_dict(sd, strict=strict)
        self.invalidate_engine()

    def load_audio_modules(self, path: str, strict: bool = True):
        """Reference models/transformer.py:464-472."""
        self.audio_model.load_state_dict(torch.load(path, map_location=self.device), strict=strict)
        self.invalidate_engine()

    def load_router_modules(self, path: str, strict: bool = True):
        """Reference models/transformer.py:509-513 -> models/router.py:417-423."""
        self.router.load_state_dict(torch.load(path, map_location=self.device), strict=strict)
        self.invalidate_engine()

    @classmethod
    def from_pretrained_cus(cls, pretrained_model_path, subfolder=None, config_path=None,
                            transformer_additional_kwargs={}, device=None, dtype=torch.bfloat16):
        """Reference models/transformer.py:1024-1093 (see ``weights.py``)."""
        from .weights import from_pretrained_cus
        return from_pretrained_cus(cls, pretrained_model_path, subfolder, config_path, transformer_additional_kwargs,
                                   device=device, dtype=dtype)

    def load_lora_weights(self, path_or_state):
        """Stage rank-r adapters for ``attn1.to_q`` / ``attn1.to_k`` (reference util/utils.py:1027-1048); they take
        effect when ``fuse_lora`` folds them into the base weights."""
        from .weights import read_lora
        self._pending_lora = getattr(self, "_pending_lora", []) + [read_lora(path_or_state)]
        return self

    def fuse_lora(self, lora_scale=1.0, lora_alpha=128):
        """Reference infer.py:279 (``pipe.fuse_lora(lora_scale=1/lora_rank)``): fold every staged adapter."""
        from .weights import fold_lora
        n = sum(fold_lora(self, l, lora_scale, lora_alpha) for l in getattr(self, "_pending_lora", []))
        self._pending_lora = []
        return n

    def enable_fp8_weights(self, enabled: bool = True, linears=None, *, fuse_qk_norm: bool = False):
        """BASELINE configs[4]: run attn1.to_q|k|v / to_out and the MLP of every DiT block on OCP e4m3 operands (weights
        quantised per output channel when the engine packs them, activations per row on the fly; everything else stays
        bf16).  ``linears``: which of engine.FP8_LINEARS ("qkv", "out", "ff1", "ff2", "pq", "aq") to quantise, a subset or "all";
        default engine.FP8_DEFAULT = the four DiT Linears -- the perceiver / audio query projections stay bf16 because the
        routing amplifies their error (tools/fp8_error_by_linear.py measures what each costs).
        ``fuse_qk_norm`` (keyword only, a bool): when attn1.to_q|k|v is an fp8 Linear fed by the LayerNorm-fused quantiser, its
        GEMM norms and rotates q and k in its own epilogue (bya_gemm_fp8_qkv_norm_rope, on the kernel the plain launch would
        take) instead of writing them in bf16 for a bya_qknorm_rope launch to read and rewrite -- the same bits; off by default
        (opt-in; a layer whose attention wants the norm statistics keeps the two launches).  No reference counterpart (the
        reference is bf16/fp16 only); returns self."""
        if not isinstance(fuse_qk_norm, bool):
            raise TypeError(f"fuse_qk_norm: expected a bool, got {type(fuse_qk_norm).__name__}")
        self._fp8_weights = bool(enabled)
        self._fp8_linears = (linears if isinstance(linears, str) else tuple(linears)) if linears else None
        # (set only when on -- absent means off: a call without the keyword sets the attributes it always set)
        if enabled and fuse_qk_norm:
            self._fp8_fuse_qk_norm = True
        elif hasattr(self, "_fp8_fuse_qk_norm"):
            del self._fp8_fuse_qk_norm
        self.invalidate_engine()
        return self

    def enable_mx_weights(self, fmt: str = "mxfp6", enabled: bool = True, linears=None, weight_format=None, *,
                          fuse_activation_quant: bool = True, fuse_attention_quant: bool = False,
                          fuse_qk_norm: bool = False, persistent_gemm=False, persistent_gemm_mxfp6=False,
                          fuse_cross_attention_quant: bool = True):
        """Run the selected Linears on OCP MX operands: 32-element blocks along K with one e8m0 scale each, applied by
        gfx950's block-scaled matrix instruction (include/bya.h, "MX weights").  ``fmt``: "mxfp6" (e2m3 elements, the
        instruction's fastest dense rate) or "mxfp8" (e4m3 elements, the more accurate).  Weights are quantised when the
        engine packs them, activations per block on the fly (by the AdaLN LayerNorm itself where it feeds the Linear).
        ``linears``: as for enable_fp8_weights (a subset of engine.FP8_LINEARS or "all"; default engine.FP8_DEFAULT) -- and, by
        name only (an explicit tuple or comma list; "all" stays the six kinds), engine.MX_CROSS_OUT = ("po", "ao"): the
        cross-attention output projections perceiver_cross_attention[*].to_out and audio_model.layers[*].attn.to_out[0], which
        enable_fp8_weights refuses.  They are in no default.
        ``weight_format``: the weights' element format -- None or ``fmt`` (the same as the activations), or "mxfp4" (e2m1
        elements, 4.25 bits per parameter) under the activations of ``fmt``; no other combination, and "mxfp4" is never an
        activation format.  ``fuse_activation_quant`` (keyword only): when ff.net.0 and ff.net.2 are both MX Linears, the
        ff.net.0 GEMM writes ff.net.2's MX operand from its own epilogue (bya_gemm_mx_quant) instead of a bf16 tensor that a
        quantiser launch reads back -- the same bytes, so on by default; False keeps the two launches.
        ``fuse_attention_quant`` (keyword only, a bool): when attn1.to_out is an MX Linear, the joint attention writes to_out's
        MX operand from its own epilogue (bya_attn_fwd_mx) instead of a bf16 tensor that a quantiser launch reads back -- the
        same bytes; off by default (opt-in; the head-parallel sharded step keeps the two launches).
        ``fuse_qk_norm`` (keyword only, a bool): when attn1.to_q|k|v is an MX Linear fed by the LayerNorm-fused quantiser, its
        GEMM norms and rotates q and k in its own epilogue (bya_gemm_mx_qkv_norm_rope) instead of writing them in bf16 for a
        bya_qknorm_rope launch to read and rewrite -- the same bits; off by default (opt-in; a layer whose attention wants
        the norm statistics keeps the two launches).
        ``persistent_gemm`` (keyword only; False, True or "always"): with "mxfp8" activations and weights, the MX Linear
        launches (bya_gemm_mx, bya_gemm_mx_quant) are issued under library option mx_kernel = 1 -- those that fill it run on
        the persistent one-wave-per-SIMD 256 x 256 kernel (csrc/gemm_mx_v4.hip), the same bits -- or, "always" (tests),
        mx_kernel = 2: every eligible launch does.  It composes with ``fuse_qk_norm``: with both on, the fused q|k|v launch
        runs on the persistent kernel too (bya_gemm_mx_qkv_norm_rope_on, kernel = 1 or 2 -- one launch per block, the same
        bits).  With ``weight_format="mxfp4"`` under "mxfp8" activations the same launches (the fused q|k|v one
        included) go through bya_gemm_mx_call with kernel = 1 (or 2) instead -- the persistent kernel's e2m1-weight instances,
        the same bits.  Off by default; with "mxfp6" activations the switch does nothing.
        ``persistent_gemm_mxfp6`` (keyword only; False, True or "always"): the same for "mxfp6" activations, with "mxfp6" or
        "mxfp4" weights -- every MX Linear launch (q|k|v plain or fused with ``fuse_qk_norm``, to_out, ff.net.0 with its
        quantising epilogue, ff.net.2) goes through bya_gemm_mx_call with kernel = 17 (or 18): the persistent kernel's e2m3
        instances where a launch fills it, the same bits.  Off by default (opt-in: its time against the tiled kernel's is
        shape by shape, tools/mx_p256_fp6_probe.py); with "mxfp8" activations it does nothing.
        ``fuse_cross_attention_quant`` (keyword only, a bool): acts only when "po" or "ao" is chosen -- the cross-attention's
        kv-mix launch (bya_attn_kv_mix_mx) writes that to_out's MX operand from its own epilogue instead of a bf16 tensor that a
        quantiser launch reads back -- the same bytes, so on by default; False, or a launch the library declines (more than
        32 keys), keeps the two launches.  Cannot be combined with enable_fp8_weights: the engine build raises ValueError.  No reference
        counterpart (the reference is bf16/fp16 only); returns self."""
        from .ops import MX_FORMATS, MX_WEIGHT_FORMATS
        if not isinstance(fuse_attention_quant, bool):
            raise TypeError(f"fuse_attention_quant: expected a bool, got {type(fuse_attention_quant).__name__}")
        if not isinstance(fuse_cross_attention_quant, bool):
            raise TypeError(f"fuse_cross_attention_quant: expected a bool, got {type(fuse_cross_attention_quant).__name__}")
        if not isinstance(fuse_qk_norm, bool):
            raise TypeError(f"fuse_qk_norm: expected a bool, got {type(fuse_qk_norm).__name__}")
        if persistent_gemm not in (False, True, "always"):
            raise ValueError(f"persistent_gemm: expected False, True or 'always', got {persistent_gemm!r}")
        if persistent_gemm_mxfp6 not in (False, True, "always"):
            raise ValueError(f"persistent_gemm_mxfp6: expected False, True or 'always', got {persistent_gemm_mxfp6!r}")
        if fmt not in MX_FORMATS:
            raise ValueError(f"MX format {fmt!r}: expected one of {sorted(MX_FORMATS)}")
        if weight_format is not None and weight_format not in MX_WEIGHT_FORMATS:
            raise ValueError(f"MX weight format {weight_format!r}: expected one of {sorted(MX_WEIGHT_FORMATS)}")
        if weight_format not in (None, fmt, "mxfp4"):
            raise ValueError(f"MX weight format {weight_format!r} under {fmt!r} activations: expected {fmt!r} or 'mxfp4'")
        self._mx_weights = fmt if enabled else None
        self._mx_weight_format = weight_format if enabled else None
        self._mx_linears = (linears if isinstance(linears, str) else tuple(linears)) if linears else None
        self._mx_fuse_activation_quant = bool(fuse_activation_quant)
        self._mx_fuse_attention_quant = fuse_attention_quant
        self._mx_fuse_qk_norm = fuse_qk_norm
        # (set only when off -- absent means on: a call without the keyword sets the attributes it always set)
        if enabled and not fuse_cross_attention_quant:
            self._mx_fuse_cross_attention_quant = False
        elif hasattr(self, "_mx_fuse_cross_attention_quant"):
            del self._mx_fuse_cross_attention_quant
        # (set only when on -- absent means off: the attributes a call without the keyword sets are those it always set)
        if enabled and persistent_gemm:
            self._mx_persistent_gemm = persistent_gemm
        elif hasattr(self, "_mx_persistent_gemm"):
            del self._mx_persistent_gemm
        if enabled and persistent_gemm_mxfp6:
            self._mx_persistent_gemm_mxfp6 = persistent_gemm_mxfp6
        elif hasattr(self, "_mx_persistent_gemm_mxfp6"):
            del self._mx_persistent_gemm_mxfp6
        self.invalidate_engine()
        return self

    def enable_step_cache(self, threshold, *, max_consecutive_hits=None, enabled: bool = True):
        """First-block step cache (include/bya.h "First-block step cache"; no reference counterpart, off
        by default): every step runs block 0 and measures d = sum |r_new - r_ref| / sum |r_ref| of its first-block residual
        against the last fully computed step's; a step with d < ``threshold`` -- and fewer than ``max_consecutive_hits`` re-used
        steps in a row before it (None: unbounded) -- adds that step's residual of the whole block stack to the stream instead of
        running blocks 1..L-1.  ``threshold`` has no default: none is defensible without a trained checkpoint (0 never re-uses,
        inf always where a reference exists).  One host synchronisation per step; four stream-sized buffers.  The state is
        dropped (the next step is full) when the geometry, batch or identity count changes, when the conditioning inputs are
        other tensors than the reference was taken under, on ``invalidate_engine()`` / an in-place weight edit and on
        ``reset_step_cache()``.  A sequence-parallel step and the CFG rank split refuse the mode (NotImplementedError).  With
        ``use_hip_graph`` on, ``forward`` takes the eager path while the cache is enabled: the decision is the host's, a graph
        cannot branch on it -- nothing about capture or replay changes.  ``enabled=False`` switches the mode off.  Returns self."""
        from .engine import StepCache
        if not isinstance(enabled, bool):
            raise TypeError(f"enabled: expected a bool, got {type(enabled).__name__}")
        if not enabled:
            self._step_cache = None
            return self
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
            raise TypeError(f"threshold: expected a number, got {type(threshold).__name__}")
        if not threshold >= 0:                       # (NaN too)
            raise ValueError(f"threshold: expected a number >= 0 (0 never re-uses, inf always), got {threshold}")
        if max_consecutive_hits is not None:
            if isinstance(max_consecutive_hits, bool) or not isinstance(max_consecutive_hits, int):
                raise TypeError(f"max_consecutive_hits: expected an int or None, got {type(max_consecutive_hits).__name__}")
            if max_consecutive_hits < 0:
                raise ValueError(f"max_consecutive_hits: expected None or an int >= 0, got {max_consecutive_hits}")
        self._step_cache = StepCache(float(threshold), max_consecutive_hits)
        return self

    def reset_step_cache(self, *, uncount_last: bool = False):
        """Forget the step cache's reference and zero its counters: the next step is a full step (the pipeline calls this at the
        start of a clip).  ``uncount_last``: keep the counters but take the last step out of them -- for a caller that runs that
        step again (the pipeline's healed re-run), so that nothing is counted twice.  A no-op while the cache is off."""
        sc = self._step_cache
        if sc is not None:
            if uncount_last:
                sc.uncount_last()
                sc.drop()
            else:
                sc.reset()
        return self

    def step_cache_stats(self):
        """{"steps", "full", "reused", "distances"} since the last ``reset_step_cache()``: the cached steps run, how many ran
        every block, how many re-used the residual, and each step's distance d (inf for a step without a reference).  None while
        the cache is off."""
        return None if self._step_cache is None else self._step_cache.stats()

    def invalidate_engine(self):
        """Drop packed weights / workspaces / captured graphs (call after changing parameters in place)."""
        self._engine = None
        self._graphs = {}
        if getattr(self, "_step_cache", None) is not None:
            self._step_cache.drop()            # (its residuals came out of the old weights; the counters stay)

    def load_state_dict(self, *a, **kw):
        out = super().load_state_dict(*a, **kw)
        self.invalidate_engine()
        return out

    def _apply(self, fn, *a, **kw):
        self.invalidate_engine()          # packed weights, workspaces AND captured graphs point at the old storage
        return super()._apply(fn, *a, **kw)

    def init_synthetic(self, seed: int = 0, fast: bool = False):
        """Fill parameters with the deterministic name-keyed synthetic weights (no checkpoints offline).

        ``fast``: draw on the parameter's device (bench-size models); otherwise use the CPU generator so the
        values are identical in every process (golden-fixture tests)."""
        from .synth import synth_tensor

        def fill(item):
            name, t = item
            dev = t.device if (fast and t.is_cuda) else "cpu"
            v = synth_tensor(name, t.shape, seed, device=dev)
            if name.endswith("pos_embedding"):
                v[:, :self.config.max_text_seq_length] = 0
            return t, v.to(t.dtype)

        with torch.no_grad():
            items = [(n, t) for n, t in self.state_dict().items() if n != "router.pos_emb"]
            if fast or len(items) < 64:
                for it in items:
                    t, v = fill(it)
                    t.copy_(v)
            else:
                # every tensor has a generator of its own (keyed by name): the CPU draws -- 8.6 G normal deviates for the
                # 42-layer model, over a minute on one core -- run on a few threads (torch.randn releases the GIL), the values
                # are the same whichever thread drew them; copies to the device stay on this thread
                import os
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(max_workers=max(1, min(12, (os.cpu_count() or 2) // 2))) as pool:
                    for t, v in pool.map(fill, items):
                        t.copy_(v)
        self.invalidate_engine()
        return self

    # ---- the hot path -------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(
        self,
        hidden_states: torch.Tensor,
        encoder_hidden_states: torch.Tensor,
        timestep: Union[int, float, torch.LongTensor],
        timestep_cond: Optional[torch.Tensor] = None,
        image_rotary_emb: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
        attention_kwargs: Optional[Dict[str, Any]] = None,
        id_cond: Optional[torch.Tensor] = None,
        id_vit_hidden: Optional[torch.Tensor] = None,
        index_mask: Optional[torch.Tensor] = None,
        return_dict: bool = True,
        audio_embeds: Optional[torch.Tensor] = None,
        af_matrix: Optional[torch.Tensor] = None,
        denoise_step: Optional[int] = None,
        index_mask_drop_prob: Optional[float] = 0.0,
        routing_logits_zeros_flag: Optional[bool] = False,
        routing_logits_forcing: Optional[torch.Tensor] = None,
    ):
        if self.is_train_face:
            assert id_cond is not None and id_vit_hidden is not None      # reference :636
        if index_mask is not None:
            raise NotImplementedError("index_mask (teacher forcing / routing losses) is a training-only branch")
        if timestep_cond is not None:
            raise NotImplementedError("timestep_cond is never passed by the reference pipeline")
        if self._engine is None:
            from .engine import DenoiseEngine
            self._engine = DenoiseEngine(self)
        args = (hidden_states, encoder_hidden_states, timestep, image_rotary_emb, id_cond, id_vit_hidden,
                audio_embeds, af_matrix, routing_logits_forcing)
        cfg = getattr(self, "_cfg", None)
        if cfg is not None and hidden_states.shape[0] == 2:
            # CFG batch split: this rank computes one sample, the pair exchange restores the [uncond, cond] batch
            return (cfg.join(self._engine.step(*cfg.take(args))), None, None, None, None)
        cached = self._step_cache is not None and self._step_cache.enabled       # (the host decides mid-step: eager)
        if self.use_hip_graph and not cached and torch.is_tensor(timestep) and self._graph_capturable():
            out = self._graphed_step(args)
        else:
            out = self._engine.step(*args)
        return (out, None, None, None, None)

    def _graph_capturable(self):
        """The unsharded step, and the sharded step on the P2P transport (its exchanges are ordinary kernels with device-
        resident sequence numbers: bya_p2p_push / bya_p2p_wait), replay from a hipGraph.  With the ``torch`` transport the
        sharded step stays eager: capturing it needs RCCL collectives inside a stream capture, and on this stack (PyTorch
        2.10-ROCm 7.0, RCCL of ROCm 7.2) even a lone ``all_to_all_single`` under ``torch.cuda.graph`` never returns
        (tools/rccl_graph_probe.py, profiles/history/r3_rccl_graph_probe.txt)."""
        group = getattr(self, "_seq_group", None)
        if getattr(self, "_seq_world", 1) == 1 and group is None:
            return True
        return getattr(self, "_seq_p2p", None) is not None

    def set_mute_audio_embeds(self, ae_mute):
        """The "mute" wav2vec embedding [>= 4 * latent_frames + 1, 12, 768] that completes a single-stream (4-D)
        ``audio_embeds`` call: the reference reads it from ``tests/input/ae_mute.pt`` on first use
        (models/audio_model.py:203), which its repository does not ship.  Not part of the state dict."""
        self.audio_model.mute_audio_embeds = ae_mute
        if self._engine is not None:
            self._engine.release()
        return self

    # ---- explicit step-invariant conditioning cache ---------------------------------
    def precompute_conditioning(self, id_cond=None, id_vit_hidden=None, audio_embeds=None, latent_frames=13):
        """Compute everything that depends only on the identities / audio (not on the timestep or the latents) once;
        later ``forward`` calls given the SAME tensors reuse it.  Call ``release_conditioning()`` to go back to the
        reference behaviour (recompute every step)."""
        if self._engine is None:
            from .engine import DenoiseEngine
            self._engine = DenoiseEngine(self)
        self._engine.precompute(id_cond, id_vit_hidden, audio_embeds, latent_frames)
        return self

    def release_conditioning(self):
        if self._engine is not None:
            self._engine.release()

    # ---- hipGraph replay of the step ---------------------------------------------------------------------------
    @staticmethod
    def _flatten(obj, out):
        if torch.is_tensor(obj):
            out.append(obj)
        elif isinstance(obj, (list, tuple)):
            for o in obj:
                BindyouravatarTransformer3DModel._flatten(o, out)
        return out

    @staticmethod
    def _rebuild(obj, it):
        if torch.is_tensor(obj):
            return next(it)
        if isinstance(obj, (list, tuple)):
            return type(obj)(BindyouravatarTransformer3DModel._rebuild(o, it) for o in obj)
        return obj

    def _graphed_step(self, args):
        """Capture ``engine.step`` once per input signature (shapes / dtypes / which optionals are present) into a HIP
        graph and replay it: the launches are identical, only the host-side launch cost disappears.  Inputs are copied
        into the graph's static buffers before every replay; the returned tensor is a fresh copy of the static output."""
        self._engine.refresh_if_stale()                # in-place parameter edits drop the captured graphs too
        # A precomputed conditioning that serves exactly these identity / audio tensors (precompute_conditioning) is READ IN PLACE
        # by the graph: the capture runs with the cache on and every lookup a hit, so it holds no conditioning launch and writes
        # nothing into the cache.  The three conditioning arguments are then not graph inputs at all (positions 4, 5, 6 of `args`:
        # the engine keys its cache by the caller's own tensors); the cache's identity -- generation and keys -- is part of the
        # graph key, the entry keeps the cached tensors alive, and the engine drops such entries with the cache.
        hit = self._engine.cache_identity(args[4], args[5], args[6])
        live = args if hit is None else tuple(None if i in (4, 5, 6) else a for i, a in enumerate(args))
        flat = self._flatten(live, [])
        key = (tuple((tuple(t.shape), t.dtype) for t in flat) + tuple(a is None for a in args), None if hit is None else hit[0])
        entry = self._graphs.get(key)
        if entry is None:
            # a captured graph bakes in raw pointers of the engine's workspace: give every graph a workspace of its
            # own and keep it alive in the graph's entry (the engine drops its workspace dict whenever the geometry
            # or batch of an eager call changes)
            self._engine._ws_key, self._engine._ws = None, None
            static = [t.detach().clone().to(self.device) for t in flat]
            static_args = self._rebuild(live, iter(static))
            if hit is not None:
                static_args = tuple(args[i] if i in (4, 5, 6) else a for i, a in enumerate(static_args))
            cache = self._engine.cache_invariants
            self._engine.cache_invariants = hit is not None   # no matching cache: recomputed inside the graph each replay
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                   # warm-up outside capture (workspaces, function attributes)
                self._engine.step(*static_args)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = self._engine.step(*static_args)
            self._engine.cache_invariants = cache
            entry = self._graphs[key] = GraphEntry(graph, static, static_out, self._engine._ws, self._engine,
                                                   None if hit is None else hit[1])
            self._engine._ws_key, self._engine._ws = None, None      # eager calls never write into a graph's buffers
        graph, static, static_out = entry.graph, entry.static, entry.static_out
        for dst, src in zip(static, flat):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
        graph.replay()
        return static_out.clone()
