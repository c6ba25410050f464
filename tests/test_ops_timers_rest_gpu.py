"""The per-entry-point timers of the non-GEMM half of ops.py (the counterpart of tests/test_ops_timers_gpu.py): one launch of
every wrapper from ``quantize_rows_fp8`` to ``vae_upsample_pad`` at the smallest shape its kernel takes -- ``attention`` once
per tag the engine uses and once with ``mx_out``, the ``attn_kv_mix`` MX launch once accepted and once declined (more than 32
keys).  The bucket names, the launches per bucket, the FLOPs per bucket (0.0 for the memory-side kernels, the formulas written
out for the others) and -- ``by_shape=True`` -- the attention labels are written out here; the declined launch returns False,
leaves no bucket and counts nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
R = 64                                            # router rows: 16 groups of 4
H, S = 8, 64                                      # joint attention: heads, rows (= keys)
MIX = dict(D=64, H=2, n_id=2, grp=2, Sq=48, Skv=20)
MIX_DECLINED_SKV = 40                             # more than 32 keys: the MX epilogue declines
VAE = dict(T=2, Hh=4, W=6, C=128, Cout=128)

ATTN_FLOPS = 4.0 * 1 * 1 * H * S * S * 64
MIX_FLOPS = 4.0 * MIX["n_id"] * MIX["grp"] * MIX["H"] * MIX["Sq"] * MIX["Skv"] * MIX["D"]
WANT_FLOPS = {
    "bya_rowgemm512": 2.0 * R * 512 * 512,
    "bya_router_group_attn": 2.0 * R * 1536 * 512 + 4.0 * R * 4 * 512,
    "bya_router_mlp_fused": 4.0 * R * 512 * 512,
    "bya_router_group_attn_out": 2.0 * R * 2048 * 512 + 4.0 * R * 4 * 512,
    "bya_router_scores": 2.0 * 2 * R * 32 * 2048,
    "bya_vae_conv3d": 2.0 * VAE["T"] * VAE["Hh"] * VAE["W"] * VAE["Cout"] * 9 * 3 * VAE["C"],
    "bya_attn_fwd:other": ATTN_FLOPS, "bya_attn_fwd:joint": ATTN_FLOPS, "bya_attn_fwd_mx:joint": ATTN_FLOPS,
    "bya_attn_kv_mix": MIX_FLOPS, "bya_attn_kv_mix_mx": MIX_FLOPS,
}
MEMORY_SIDE = ["bya_quantize_rows_fp8", "bya_quantize_mx", "bya_linear_small_m", "bya_timestep_features", "bya_layernorm",
               "bya_layernorm_fp8", "bya_layernorm_mx", "bya_qknorm_rope", "bya_attn_tiny", "bya_router_head",
               "bya_forcing_max_over_frames", "bya_masked_combine", "bya_routed_mix", "bya_patchify", "bya_unpatchify", "bya_act_add",
               "bya_cfg_scheduler_step", "bya_masks_to_routing_logits", "bya_vae_patches", "bya_vae_groupnorm_stats", "bya_vae_norm_act",
               "bya_vae_groupnorm_moments", "bya_vae_norm_act_moments",
               "bya_vae_upsample_pad"]
ATTN_SHAPE = f"1x1x{H}h_q{S}_kv{S}_d64"


@pytest.fixture(scope="module")
def operands(dev):
    """Everything the launches read, built before any timer runs."""
    from bind_your_avatar_implementation_amd import ops
    g = torch.Generator().manual_seed(12)
    rnd = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(BF).to(dev)
    o = dict(rnd=rnd)
    w512 = lambda n: rnd(n, 512, std=512 ** -0.5)
    ln = (rnd(512) + 1, rnd(512))
    o["pack_qkv"] = ops.pack_rowgemm512(w512(1536), rnd(1536), *ln)
    o["pack_ln"] = ops.pack_rowgemm512(w512(512), rnd(512), *ln)
    o["pack"] = ops.pack_rowgemm512(w512(512), rnd(512))
    torch.cuda.synchronize()
    return o


def mix_operands(rnd, Skv):
    D, Hm, n_id, grp, Sq = (MIX[k] for k in ("D", "H", "n_id", "grp", "Sq"))
    E = Hm * D
    kw = dict(head_dim=D, heads=Hm, n_id=n_id, n_grp=grp, Sq=Sq, Skv=Skv, q_strides=(Sq * E, E), k_strides=(grp * Skv * E, Skv * E, E),
              v_strides=(grp * Skv * E, Skv * E, E), scale=D ** -0.5)
    return [rnd(grp, Sq, E), rnd(n_id, grp, Skv, E), rnd(n_id, grp, Skv, E), torch.sigmoid(rnd(grp * Sq, n_id).float()).to(BF)], kw, E


def launch_everything(o, dev):
    """One accepted launch per wrapper (three of ``attention``, two of ``attn_kv_mix``), then the declined one.  -> what it returned."""
    from bind_your_avatar_implementation_amd import ops
    rnd = o["rnd"]
    bf = lambda *s: torch.empty(*s, dtype=BF, device=dev)
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)

    # the quantisers, the small step kernels
    x = rnd(R, 256)
    ops.quantize_rows_fp8(x)
    ops.quantize_mx(x, "mxfp8")
    ops.linear_small_m(rnd(2, 512), rnd(64, 512, std=512 ** -0.5), rnd(64), bf(2, 64))
    ops.timestep_features(torch.tensor([1, 500, 999], dtype=torch.int64, device=dev), bf(3, 256))
    ops.act_add(rnd(1024), bf(1024), act="silu", res=rnd(1024))
    coef = dict(guidance=6.0, sqrt_alpha=0.8, sqrt_beta=0.6, k_sample=1.25, k_denoised=-0.5, k_noise=0.0, k_cur=1.5, k_old=-0.5)
    assert ops.cfg_scheduler_step(rnd(2, 1024), rnd(1, 1024), coef).shape == (1, 1024)
    ops.patchify(rnd(1, 2, 4, 8, 8), bf(1, 2 * 4 * 4, 16))
    ops.unpatchify(rnd(1, 2 * 4 * 4, 16), bf(1, 2, 4, 8, 8))
    masks = (torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(3)) > 0.5).to(torch.uint8).to(dev)
    assert ops.masks_to_routing_logits(masks, frames=2, h=4, w=4).shape == (1, 2 * 4 * 4, 2)

    # the norms (the quantising LayerNorms exist at the DiT width)
    xn = rnd(R, 3072)
    ops.layernorm(xn, bf(R, 3072))
    ops.layernorm_fp8(xn, u8(R, 3072), f32(R))
    ops.layernorm_mx(xn, u8(R, 3072), u8(R, 96), "mxfp8")
    W = H * 64
    q, k, v = rnd(1, S, W, std=0.25), rnd(1, S, W, std=0.25), rnd(1, S, W)
    n64 = [rnd(64) + 1, rnd(64), rnd(64) + 1, rnd(64)]
    ops.qknorm_rope(rnd(1, S, W), rnd(1, S, W), *n64, torch.rand(S - 8, 64, device=dev), torch.rand(S - 8, 64, device=dev), H, 8)

    # attention: the engine's two tags, and the MX-output launch
    out = bf(1, S, W)
    assert ops.self_attention(q, k, v, out, H) is out
    assert ops.self_attention(q, k, v, out, H, scale=1.0, tag="joint", prescaled=True, score_bound=48.0) is out
    pair = (u8(S, W), u8(S, H * 2), "mxfp8")
    got = ops.self_attention(q, k, v, None, H, scale=1.0, tag="joint", prescaled=True, score_bound=48.0, mx_out=pair)
    assert got[0] is pair[0] and got[1] is pair[1]
    qkv = rnd(R, 1536)
    ops.attn_tiny(qkv, qkv[:, 512:], qkv[:, 1024:], bf(R, 512), 4, 8, 16, 1, 4, 1, 1536, 512, 0.125)

    # the cross-attention with the router's mix in its epilogue: bf16 out, MX out
    (mq, mk, mv, mr), kw, E = mix_operands(rnd, MIX["Skv"])
    rows = MIX["grp"] * MIX["Sq"]
    z = bf(MIX["grp"], MIX["Sq"], E)
    assert ops.attn_kv_mix(mq, mk, mv, mr, None, z, f32(rows), z_strides=(MIX["Sq"] * E, E), **kw) is z
    mpair = (u8(rows, E), u8(rows, E // 32), "mxfp8")
    got = ops.attn_kv_mix(mq, mk, mv, mr, None, None, f32(rows), mx_out=mpair, **kw)
    assert got is not False and got[0] is mpair[0] and got[1] is mpair[1]

    # the router: scores, head, combines, row kernels
    ops.router_scores(rnd(R, 2048, std=0.1), rnd(2, 32, 2048, std=0.1), rnd(512) + 1, rnd(512), rnd(R, 512), bf(2, R, 512), 2, R)
    ops.router_head(rnd(2, R, 512), rnd(512, std=0.05), rnd(1), bf(R, 2), 2, R)
    ops.forcing_max_over_frames(rnd(4, 30, 2), bf(4, 30, 2), 4, 30, 2)
    feat, r = rnd(1, 2, R, 64), torch.sigmoid(rnd(1, R, 2).float()).to(BF)
    ops.masked_combine(rnd(1, R, 64), feat, r, None, "face")
    ops.routed_mix(feat, r, torch.eye(2, device=dev, dtype=BF)[None].contiguous(), "audio", bf(1, R, 64), f32(1, R))
    xr = rnd(R, 512)
    geo = (4, 16, 1, 4, 1)                        # L, n_outer, n_inner, outer_stride, seq_stride: 16 groups of 4 rows
    ops.rowgemm512(xr, o["pack_ln"], bf(R, 512), act="gelu_erf")
    ops.router_group_attn(xr, o["pack_qkv"], bf(R, 512), *geo)
    ops.router_mlp_fused(xr.clone(), o["pack_ln"], o["pack"])
    ops.router_group_attn_out(xr.clone(), o["pack_qkv"], o["pack"], *geo)

    # the video VAE
    T, Hh, Wv, C, Cout = (VAE[k] for k in ("T", "Hh", "W", "C", "Cout"))
    xv = rnd(T, Hh, Wv, C)
    ops.vae_patches(xv, None, bf(T * Hh * Wv, 27 * C), 3, 1, 1, False, 0, Hh, Wv, 0, T)
    sums = f32(64)
    ops.vae_groupnorm_stats(xv.view(-1, C), sums, 32)
    ops.vae_norm_act(xv, bf(T, Hh, Wv, C), sums, rnd(C) + 1, rnd(C), 32)
    ops.vae_groupnorm_stats(xv.view(-1, C), sums, 32, moments=True)
    ops.vae_norm_act(xv, bf(T, Hh, Wv, C), sums, rnd(C) + 1, rnd(C), 32, moments=True)
    xpad = torch.zeros(T + 2, Hh + 2, Wv + 2, C, dtype=BF, device=dev)
    ops.vae_conv3d(xpad, rnd(Cout, 27 * C, std=(27 * C) ** -0.5), rnd(Cout), bf(T, Hh, Wv, Cout))
    ops.vae_upsample_pad(xv, torch.zeros(2 * T, 2 * Hh + 2, 2 * Wv + 2, C, dtype=BF, device=dev), 1)

    # declined: 40 keys (the matching plan query answers None)
    (mq, mk, mv, mr), kw, E = mix_operands(rnd, MIX_DECLINED_SKV)
    assert ops.attn_kv_mix_plan(None, None, mx_out=mpair, **kw) is None
    declined = ops.attn_kv_mix(mq, mk, mv, mr, None, None, f32(rows), mx_out=mpair, **kw)
    torch.cuda.synchronize()
    return declined


def run(o, dev, by_shape):
    from bind_your_avatar_implementation_amd import ops
    ops.enable_kernel_timers(by_shape=by_shape)
    try:
        declined = launch_everything(o, dev)
        flops = ops.kernel_timer_flops()
        timers = ops.collect_kernel_timers()
    finally:
        ops.enable_kernel_timers()                                       # (shape labels off again)
        ops.collect_kernel_timers()                                      # ... and the timers
    assert declined is False
    assert all(t >= 0.0 for v in timers.values() for t in v)
    return {k: len(v) for k, v in timers.items()}, flops


def test_buckets_launches_and_flops_per_entry_point(dev, operands):
    launches, flops = run(operands, dev, by_shape=False)
    want = dict(WANT_FLOPS, **{k: 0.0 for k in MEMORY_SIDE})
    assert launches == {k: 1 for k in want}
    assert launches["bya_attn_kv_mix_mx"] == 1                          # the accepted MX mix alone: the declined one left nothing
    assert flops == want


def test_attention_shape_labels(dev, operands):
    launches, flops = run(operands, dev, by_shape=True)
    labelled = {"bya_attn_fwd:other:" + ATTN_SHAPE: ATTN_FLOPS, "bya_attn_fwd:joint:" + ATTN_SHAPE: ATTN_FLOPS,
                "bya_attn_fwd_mx:joint:" + ATTN_SHAPE + ">mxfp8": ATTN_FLOPS}
    want = {k: v for k, v in WANT_FLOPS.items() if not k.startswith("bya_attn_fwd")}         # the other buckets take no shape label
    want.update(labelled, **{k: 0.0 for k in MEMORY_SIDE})
    assert launches == {k: 1 for k in want}
    assert flops == want
