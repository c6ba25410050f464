"""CPU: what the non-GEMM half of ops.py hands to the library -- entry point, pointers, dimensions, strides, descriptor bytes,
and in which order -- for every wrapper from ``quantize_rows_fp8`` to ``vae_upsample_pad``: the LAUNCH wrappers and their
``*_plan`` twins, against a recording taken before the pairs were folded onto shared bodies
(tests/golden/ops_launch_args.json).  The library is the recording stub of tests/test_ops_descriptors_cpu.py.  Launch
wrappers refuse meta tensors, so they are given ``FakeDevice`` tensors: meta tensors that say they are device tensors and
whose address is ``ops._META_BASE`` + the view's offset, the same in every process; ``ops._stream`` is a constant and the
timers are off.  What a wrapper returns is recorded too: for launches which argument came back, for queries the dict built
from the stub's zero-filled struct.

Outputs that a wrapper would allocate itself (``quantize_*`` codes and scales, ``vae_groupnorm_stats``' partial sums, the
routing logits) are always passed: there is no device here to allocate them on.

``python tests/test_ops_launch_args_cpu.py`` rewrites the recording from the ``ops`` module on the path.  It pins a refactor to
the code before it: regenerate it only when a call is MEANT to change, from the commit that is meant to be matched."""
import json
import os

import pytest
import torch

from test_ops_descriptors_cpu import StubLibrary, bf, f32, u8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_launch_args.json")
STREAM = 0x5EED
B, M, K, DW = 2, 40, 64, 96                      # batches, rows, a quantised width, the LayerNorm width (3 MX blocks)
MX_BYTES = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}


class FakeDevice(torch.Tensor):
    """A meta tensor that passes for a device tensor (views keep the subclass)."""
    is_cuda = property(lambda s: True)
    is_meta = property(lambda s: False)

    def data_ptr(self):
        from bind_your_avatar_implementation_amd import ops
        return ops._META_BASE + self.storage_offset() * self.element_size()


def D(t):
    return t.as_subclass(FakeDevice)


def i32(*s):
    return torch.empty(*s, dtype=torch.int32, device="meta")


def i64(*s):
    return torch.empty(*s, dtype=torch.int64, device="meta")


def ident(t):
    return t


def norm_cases(add):
    """The LayerNorm family (four output kinds, launch and query) and the q/k norm."""
    affine = lambda dev: dict(weight=dev(bf(DW)), bias=dev(bf(DW)))
    mod = lambda dev: dict(shift0=dev(bf(B, DW)), scale0=dev(bf(B, DW)), shift1=dev(bf(B, 2 * DW))[:, DW:], scale1=dev(bf(B, DW)),
                           split=7, mod_batch_stride=DW)
    xs = lambda dev: {"2d": dev(bf(M, DW)), "3d": dev(bf(B, M, DW)), "view": dev(bf(M, 2 * DW + 8))[:, 8:8 + DW],
                      "view_3d": dev(bf(B, M + 3, 2 * DW))[:, 1:M + 1, DW:]}

    def codes(dev, shape, rb):
        """A code matrix of ``rb`` bytes per row for an x of this layout: contiguous for the plain ones, padded rows for views."""
        if shape == "2d":
            return dev(u8(M, rb))
        if shape == "3d":
            return dev(u8(B, M, rb))
        if shape == "view":
            return dev(u8(M, rb + 32))[:, 16:16 + rb]
        return dev(u8(B, M + 1, rb + 16))[:, 1:, :rb]

    for shape in ("2d", "3d", "view", "view_3d"):
        lead = (B, M) if shape.endswith("3d") else (M,)
        for mname, kw in (("plain", lambda dev: {}), ("affine", affine), ("mod", lambda dev: dict(affine(dev), **mod(dev), eps=1e-6))):
            if (shape, mname) in (("view", "affine"), ("view_3d", "plain")):
                continue                                                  # (keep the table short: the views with and without)
            x = xs(D)[shape]
            add(f"ln/bf16/{shape}/{mname}", "layernorm", [x, xs(D)[shape]], kw(D))
            add(f"ln/fp8/{shape}/{mname}", "layernorm_fp8", [x, codes(D, shape, DW), D(f32(*lead))], kw(D))
            for fmt in ("mxfp8", "mxfp6"):
                rb = DW * MX_BYTES[fmt] // 8
                add(f"ln/{fmt}/{shape}/{mname}", "layernorm_mx", [x, codes(D, shape, rb), D(u8(*lead, DW // 32)), fmt], kw(D))
            pkw = {k: v for k, v in kw(ident).items() if k != "eps"}      # (the query takes no eps)
            xm = xs(ident)[shape]
            add(f"ln_plan/bf16/{shape}/{mname}", "layernorm_plan", [xm, xs(ident)[shape]], pkw)
            for kind, rb in (("fp8", DW), ("mxfp8", DW), ("mxfp6", DW * 6 // 8)):
                add(f"ln_plan/{kind}/{shape}/{mname}", "layernorm_plan", [xm, codes(ident, shape, rb)], dict(pkw, out_kind=kind))
    add("ln/fp8/flat_codes", "layernorm_fp8", [D(bf(B, M, DW)), D(u8(B * M * DW)), D(f32(B * M))], {})
    add("ln/mxfp6/flat_codes", "layernorm_mx", [D(bf(B, M, DW)), D(u8(B * M, DW * 6 // 8)), D(u8(B * M * 3)), "mxfp6"], {})
    add("ln_plan/bf16/some_vectors", "layernorm_plan", [bf(M, DW), bf(M, DW), True, True], dict(shift1=True, scale1=True))
    add("ln_plan/fp8/device", "layernorm_plan", [D(bf(B, M, DW)), D(u8(B, M, DW))], dict(weight=D(bf(DW)), out_kind="fp8"))
    add("ln_plan/mxfp6/wide_rows", "layernorm_plan", [bf(M, DW), u8(M, DW)], dict(out_kind="mxfp6"))
    for fn, name, o in (("layernorm", "ln", D), ("layernorm_plan", "ln_plan", ident)):
        add(f"{name}/x_dtype!", fn, [o(f32(M, DW)), o(bf(M, DW))], {})
        add(f"{name}/x_4d!", fn, [o(bf(1, 1, M, DW)), o(bf(M, DW))], {})
        add(f"{name}/out_shape!", fn, [o(bf(M, DW)), o(bf(M + 1, DW))], {})
        add(f"{name}/x_inner_stride!", fn, [o(bf(M, 2 * DW))[:, ::2], o(bf(M, DW))], {})
    add("ln/fp8/codes_dtype!", "layernorm_fp8", [D(bf(M, DW)), D(bf(M, DW)), D(f32(M))], {})
    add("ln_plan/fp8/codes_dtype!", "layernorm_plan", [bf(M, DW), bf(M, DW)], dict(out_kind="fp8"))
    add("ln/fp8/codes_rows!", "layernorm_fp8", [D(bf(M, DW)), D(u8(M + 2, DW + 16))[:, :DW], D(f32(M))], {})
    add("ln_plan/fp8/codes_rows!", "layernorm_plan", [bf(M, DW), u8(M + 2, DW + 16)[:, :DW]], dict(out_kind="fp8"))

    H, S, T = 2, 12, 5
    W = H * 64
    p = lambda dev: [dev(bf(64)) for _ in range(4)]
    qkv = lambda dev: dev(bf(B, S, 3 * W))
    tables = lambda dev, rows: [dev(f32(rows, 64)), dev(f32(rows, 64))]
    t = qkv(D)
    add("qkn/both", "qknorm_rope", [t[..., :W], t[..., W:2 * W], *p(D), *tables(D, S - T), H, T], {})
    add("qkn/q_only_scaled", "qknorm_rope", [t[..., :W], None, *p(D), *tables(D, S - T), H, T], dict(eps=1e-5, k_scale=0.125))
    add("qkn/k_only_no_rope", "qknorm_rope", [None, t[..., W:2 * W], *p(D), None, None, H, S], {})
    add("qkn/stats", "qknorm_rope", [t[..., :W], t[..., W:2 * W], *p(D), *tables(D, S - T), H, T], dict(stats=D(f32(3, 2, B * H))))
    add("qkn/2d", "qknorm_rope", [D(bf(S, W)), D(bf(S, W)), *p(D), *tables(D, S), H, 0], {})
    m = qkv(ident)
    add("qkn_plan/both", "qknorm_rope_plan", [m[..., :W], m[..., W:2 * W], H, T], {})
    add("qkn_plan/q_only_tables", "qknorm_rope_plan", [m[..., :W], None, H, T], dict(cos=f32(S - T, 64)))
    add("qkn_plan/k_only_no_rope", "qknorm_rope_plan", [None, m[..., W:2 * W], H, S], dict(cos=None))
    add("qkn_plan/stats_slots", "qknorm_rope_plan", [m[..., :W], m[..., W:2 * W], H, T], dict(stats=3))
    add("qkn_plan/stats_tensor", "qknorm_rope_plan", [m[..., :W], m[..., W:2 * W], H, T], dict(stats=f32(3, 2, B * H)))
    add("qkn_plan/2d_device", "qknorm_rope_plan", [D(bf(S, W)), D(bf(S, W)), H, 0], {})
    add("qkn/k_layout!", "qknorm_rope", [t[..., :W], D(bf(B, S, W)), *p(D), *tables(D, S - T), H, T], {})
    add("qkn_plan/k_layout!", "qknorm_rope_plan", [m[..., :W], bf(B, S, W), H, T], {})
    add("qkn/q_dtype!", "qknorm_rope", [D(f32(B, S, W)), None, *p(D), None, None, H, S], {})
    add("qkn_plan/q_dtype!", "qknorm_rope_plan", [f32(B, S, W), None, H, S], dict(cos=None))
    add("qkn/cos_shape!", "qknorm_rope", [t[..., :W], None, *p(D), *tables(D, S), H, T], {})


def attn_cases(add):
    H, Sq, Skv, nb = 2, 40, 48, 2
    W = H * 64
    geo = dict(head_dim=64, heads=H, nb1=nb, nb2=1, Sq=Sq, Skv=Skv, q_strides=(Sq * W, 0, W), k_strides=(Skv * 3 * W, 0, 3 * W),
               v_strides=(Skv * 3 * W, 0, 3 * W), scale=0.125)
    o_strides = (Sq * W, 0, W)

    def qkv(dev):
        kv = dev(bf(nb, Skv, 3 * W))
        return [dev(bf(nb, Sq, W)), kv[..., W:2 * W], kv[..., 2 * W:]]

    def pair(dev, fmt):
        return (dev(u8(nb * Sq, W * MX_BYTES[fmt] // 8)), dev(u8(nb, Sq, H * 2)), fmt)

    bound = lambda dev: (dev(f32(3, 2, 8)), 4, dev(i32(nb * H)))
    variants = (("plain", {}), ("prescaled", dict(prescaled=True)), ("static_bound", dict(prescaled=True, score_bound=48.0)),
                ("device_bound", dict(prescaled=True, bound=None)))
    for name, kw in variants:
        for dev, fn, pre in ((D, "attention", "attn"), (ident, "attention_plan", "attn_plan")):
            kw = dict(kw, bound=bound(dev)) if "bound" in kw else kw
            lead = qkv(dev) if dev is D else []
            tag = dict(tag="self") if dev is D and name == "static_bound" else {}
            add(f"{pre}/bf16/{name}", fn, [*lead, dev(bf(nb, Sq, W))], dict(geo, o_strides=o_strides, **kw, **tag))
            for fmt in ("mxfp8", "mxfp6"):
                add(f"{pre}/{fmt}/{name}", fn, [*lead, None], dict(geo, mx_out=pair(dev, fmt), **kw, **tag))
    add("attn/bf16/d128_two_levels", "attention", [D(bf(2, 3, Sq, 128)), D(bf(2, 3, Skv, 128)), D(bf(2, 3, Skv, 128)), D(bf(2, 3, Sq, 128))],
        dict(head_dim=128, heads=1, nb1=2, nb2=3, Sq=Sq, Skv=Skv, q_strides=(3 * Sq * 128, Sq * 128, 128),
             k_strides=(3 * Skv * 128, Skv * 128, 128), v_strides=(3 * Skv * 128, Skv * 128, 128), o_strides=(3 * Sq * 128, Sq * 128, 128),
             scale=128 ** -0.5, tag="cross"))
    add("attn/mxfp8/zero_o_strides", "attention", [*qkv(D), None], dict(geo, o_strides=(0, 0, 0), mx_out=pair(D, "mxfp8")))
    for ws in (True, False):
        add(f"attn_plan/bf16/workspace_{ws}", "attention_plan", [bf(nb, Sq, W)],
            dict(geo, o_strides=o_strides, prescaled=True, score_bound=48.0, workspace=ws))
        add(f"attn_plan/mxfp6/workspace_{ws}", "attention_plan", [None], dict(geo, prescaled=True, score_bound=48.0, workspace=ws,
                                                                            mx_out=pair(ident, "mxfp6")))
    add("attn_plan/bf16/device_out", "attention_plan", [D(bf(nb, Sq, W))], dict(geo, o_strides=o_strides, prescaled=True, bound=bound(D)))
    add("attn_plan/mxfp8/device_out", "attention_plan", [None], dict(geo, prescaled=True, score_bound=48.0, mx_out=pair(D, "mxfp8")))
    for dev, fn, pre in ((D, "attention", "attn"), (ident, "attention_plan", "attn_plan")):
        lead = qkv(dev) if dev is D else []
        add(f"{pre}/out_and_mx_out!", fn, [*lead, dev(bf(nb, Sq, W))], dict(geo, o_strides=o_strides, mx_out=pair(dev, "mxfp8")))
        add(f"{pre}/mx_o_strides!", fn, [*lead, None], dict(geo, o_strides=o_strides, mx_out=pair(dev, "mxfp8")))
        add(f"{pre}/mx_e2m1!", fn, [*lead, None], dict(geo, mx_out=(dev(u8(nb * Sq, W // 2)), dev(u8(nb * Sq, H * 2)), "mxfp4")))
        add(f"{pre}/mx_head_dim!", fn, [*lead, None], dict(geo, head_dim=128, mx_out=pair(dev, "mxfp8")))
        add(f"{pre}/mx_codes_size!", fn, [*lead, None], dict(geo, mx_out=(dev(u8(nb * Sq, W)), dev(u8(nb * Sq, H * 2)), "mxfp6")))
        add(f"{pre}/mx_codes_dtype!", fn, [*lead, None], dict(geo, mx_out=(dev(bf(nb * Sq, W)), dev(u8(nb * Sq, H * 2)), "mxfp8")))
        add(f"{pre}/bound_stats_dtype!", fn, [*lead, dev(bf(nb, Sq, W))],
            dict(geo, o_strides=o_strides, prescaled=True, bound=(dev(bf(3, 2, 8)), 0, dev(i32(nb * H)))))
        add(f"{pre}/bound_flags_short!", fn, [*lead, dev(bf(nb, Sq, W))],
            dict(geo, o_strides=o_strides, prescaled=True, bound=(dev(f32(3, 2, 8)), 0, dev(i32(nb * H - 1)))))
    add("attn/q_dtype!", "attention", [D(f32(nb, Sq, W)), *qkv(D)[1:], D(bf(nb, Sq, W))], dict(geo, o_strides=o_strides))
    add("attn/meta_out!", "attention", [*qkv(D), bf(nb, Sq, W)], dict(geo, o_strides=o_strides))

    # self_attention: [B, S, heads * head_dim] views, the strides read off the tensors
    packed = D(bf(nb, Sq, 3 * W))
    add("self/contiguous", "self_attention", [D(bf(nb, Sq, W)), D(bf(nb, Skv, W)), D(bf(nb, Skv, W)), D(bf(nb, Sq, W)), H], {})
    add("self/packed_views", "self_attention", [packed[..., :W], packed[..., W:2 * W], packed[..., 2 * W:], D(bf(nb, Sq + 2, W))[:, 2:], H],
        dict(scale=1.0, tag="self", prescaled=True, score_bound=48.0))
    add("self/2d_d128", "self_attention", [D(bf(Sq, 128)), D(bf(Skv, 128)), D(bf(Skv, 128)), D(bf(Sq, 128)), 1], dict(head_dim=128))
    add("self/mx", "self_attention", [packed[..., :W], packed[..., W:2 * W], packed[..., 2 * W:], None, H],
        dict(scale=1.0, prescaled=True, bound=bound(D), mx_out=pair(D, "mxfp6")))
    add("self/q_4d!", "self_attention", [D(bf(1, nb, Sq, W)), D(bf(nb, Skv, W)), D(bf(nb, Skv, W)), D(bf(nb, Sq, W)), H], {})

    # attn_kv_mix: both output forms, the 2-D and 3-D code layouts
    n_id, grp, Sq, Skv, H, Dh = 2, 3, 24, 20, 2, 64
    E = H * Dh
    mix = dict(head_dim=Dh, heads=H, n_id=n_id, n_grp=grp, Sq=Sq, Skv=Skv, q_strides=(Sq * E, E), k_strides=(grp * Skv * 2 * E, Skv * 2 * E, 2 * E),
               v_strides=(grp * Skv * 2 * E, Skv * 2 * E, 2 * E), scale=0.125)

    def operands(dev):
        kv = dev(bf(n_id, grp, Skv, 2 * E))
        return [dev(bf(grp, Sq, E)), kv[..., :E], kv[..., E:], dev(bf(grp * Sq, n_id))]

    def mix_pair(dev, fmt, layout):
        cb, sb = E * MX_BYTES[fmt] // 8, E // 32
        if layout == "2d":
            return (dev(u8(grp * Sq, cb)), dev(u8(grp * Sq, sb)), fmt)
        if layout == "3d":
            return (dev(u8(grp, Sq, cb)), dev(u8(grp, Sq, sb)), fmt)
        return (dev(u8(grp, Sq + 4, cb + 64))[:, 2:2 + Sq, 32:], dev(u8(grp * Sq + 8, sb + 4))[8:], fmt)      # views of larger buffers

    zs = (Sq * E, E)
    for name, af, wsum in (("face", False, False), ("audio", True, False), ("audio_wsum", True, True)):
        a = lambda dev: dev(bf(n_id, n_id)) if af else None
        w = D(f32(grp * Sq + 8)) if wsum else None
        add(f"mix/bf16/{name}", "attn_kv_mix", [*operands(D), a(D), D(bf(grp, Sq, E)), w], dict(mix, z_strides=zs))
        add(f"mix_plan/bf16/{name}", "attn_kv_mix_plan", [bf(grp, Sq, E), a(ident)], dict(mix, z_strides=zs))
        for fmt, layout in (("mxfp8", "2d"), ("mxfp6", "3d"), ("mxfp8", "views")):
            add(f"mix/{fmt}/{layout}/{name}", "attn_kv_mix", [*operands(D), a(D), None, w], dict(mix, mx_out=mix_pair(D, fmt, layout)))
            add(f"mix_plan/{fmt}/{layout}/{name}", "attn_kv_mix_plan", [None, a(ident)], dict(mix, mx_out=mix_pair(ident, fmt, layout)))
    add("mix/bf16/z_view", "attn_kv_mix", [*operands(D), None, D(bf(grp, Sq, 2 * E))[..., E:]], dict(mix, z_strides=(Sq * 2 * E, 2 * E)))
    add("mix_plan/bf16/z_view_device", "attn_kv_mix_plan", [D(bf(grp, Sq, 2 * E))[..., E:]], dict(mix, z_strides=(Sq * 2 * E, 2 * E)))
    add("mix_plan/mxfp8/device", "attn_kv_mix_plan", [None, D(bf(n_id, n_id))], dict(mix, mx_out=mix_pair(D, "mxfp8", "3d")))
    for dev, fn, pre in ((D, "attn_kv_mix", "mix"), (ident, "attn_kv_mix_plan", "mix_plan")):
        lead = [*operands(dev), None] if dev is D else []
        z = lambda *a: [*lead, *a] if dev is D else [*a, None]
        add(f"{pre}/z_and_mx_out!", fn, z(dev(bf(grp, Sq, E))), dict(mix, mx_out=mix_pair(dev, "mxfp8", "2d")))
        add(f"{pre}/mx_z_strides!", fn, z(None), dict(mix, z_strides=zs, mx_out=mix_pair(dev, "mxfp8", "2d")))
        add(f"{pre}/mx_e2m1!", fn, z(None), dict(mix, mx_out=(dev(u8(grp * Sq, E // 2)), dev(u8(grp * Sq, E // 32)), "mxfp4")))
        add(f"{pre}/mx_codes_narrow!", fn, z(None), dict(mix, mx_out=(dev(u8(grp * Sq, E - 8)), dev(u8(grp * Sq, E // 32)), "mxfp8")))
        add(f"{pre}/mx_scales_rows!", fn, z(None), dict(mix, mx_out=(dev(u8(grp * Sq, E)), dev(u8(grp * Sq - 1, E // 32)), "mxfp8")))
        add(f"{pre}/mx_codes_dtype!", fn, z(None), dict(mix, mx_out=(dev(bf(grp * Sq, E)), dev(u8(grp * Sq, E // 32)), "mxfp8")))
        add(f"{pre}/bf16_no_z_strides!", fn, z(dev(bf(grp, Sq, E))), dict(mix))
    add("mix/r_size!", "attn_kv_mix", [*operands(D)[:3], D(bf(grp * Sq, n_id + 1)), None, D(bf(grp, Sq, E))], dict(mix, z_strides=zs))

    # attn_tiny: the caller gives every dimension
    t = lambda dev: dev(bf(50, 3 * 128))
    for dev, pre in ((D, "tiny"), (ident, "tiny_plan")):
        x, o = t(dev), dev(bf(50, 128))
        if dev is D:
            add("tiny/packed", "attn_tiny", [x[:, :128], x[:, 128:256], x[:, 256:], o, 2, 2, 5, 5, 10, 5, 384, 128, 0.125], {})
            add("tiny/plain", "attn_tiny", [o, dev(bf(50, 128)), dev(bf(50, 128)), dev(bf(50, 128)), 25, 2, 2, 1, 25, 1, 128, 128, 1.0], {})
        else:
            add("tiny_plan/packed", "attn_tiny_plan", [x[:, :128], x[:, 128:256], x[:, 256:], o, 2, 2, 5, 5, 384, 128], {})
            add("tiny_plan/device", "attn_tiny_plan", [D(o), D(bf(50, 128)), D(bf(50, 128)), D(bf(50, 128)), 25, 2, 2, 1, 128, 128], {})
    add("tiny/meta_q!", "attn_tiny", [bf(50, 128), D(bf(50, 128)), D(bf(50, 128)), D(bf(50, 128)), 25, 2, 2, 1, 25, 1, 128, 128, 1.0], {})


def step_cases(add):
    """The small step kernels, the router's scores / head / combine, patchify, the scheduler step, the quantisers."""
    N = 48
    for name, x, q, s in (("2d", D(bf(M, K)), D(u8(M, K)), D(f32(M))), ("3d", D(bf(B, M, K)), D(u8(B, M, K)), D(f32(B, M))),
                          ("view", D(bf(M, 2 * K + 8))[:, 8:8 + K], D(u8(M * K)), D(f32(M))),
                          ("view_3d", D(bf(B, M, 2 * K))[..., K:], D(u8(B, M, K)), D(f32(B * M)))):
        add(f"quant/fp8/{name}", "quantize_rows_fp8", [x, q, s], {})
        for fmt in ("mxfp8", "mxfp6", "mxfp4"):
            add(f"quant/{fmt}/{name}", "quantize_mx", [x, fmt, D(u8(*x.shape[:-1], K * MX_BYTES[fmt] // 8)), D(u8(*x.shape[:-1], K // 32))], {})
    add("quant/fp8/uneven_batches!", "quantize_rows_fp8", [D(bf(B, M + 1, K))[:, :M], D(u8(B, M, K)), D(f32(B, M))], {})
    add("quant/fp8/x_dtype!", "quantize_rows_fp8", [D(f32(M, K)), D(u8(M, K)), D(f32(M))], {})
    add("quant/fp8/q_size!", "quantize_rows_fp8", [D(bf(M, K)), D(u8(M, K + 1)), D(f32(M))], {})
    add("quant/mx/uneven_batches!", "quantize_mx", [D(bf(B, M + 1, K))[:, :M], "mxfp8", D(u8(B, M, K)), D(u8(B, M, K // 32))], {})
    add("quant/mx/fmt!", "quantize_mx", [D(bf(M, K)), "mxfp3", D(u8(M, K)), D(u8(M, K // 32))], {})
    add("quant/mx/scales_size!", "quantize_mx", [D(bf(M, K)), "mxfp8", D(u8(M, K)), D(u8(M, K // 32 + 1))], {})

    add("lin/bias", "linear_small_m", [D(bf(2, K)), D(bf(N, K)), D(bf(N)), D(bf(2, N))], {})
    add("lin/silu_in_out", "linear_small_m", [D(bf(8, K)), D(bf(N, K)), None, D(bf(8, N))], dict(silu_in=True, act_out="silu"))
    add("lin_plan/plain", "linear_small_m_plan", [bf(2, K), bf(N, K), bf(2, N)], {})
    add("lin_plan/silu_device", "linear_small_m_plan", [D(bf(8, K)), D(bf(N, K)), D(bf(8, N))], dict(act_out="silu"))
    add("lin/x_3d!", "linear_small_m", [D(bf(1, 2, K)), D(bf(N, K)), None, D(bf(2, N))], {})
    add("lin_plan/x_3d!", "linear_small_m_plan", [bf(1, 2, K), bf(N, K), bf(2, N)], {})
    add("lin/act!", "linear_small_m", [D(bf(2, K)), D(bf(N, K)), None, D(bf(2, N))], dict(act_out="swish"))
    add("lin_plan/act!", "linear_small_m_plan", [bf(2, K), bf(N, K), bf(2, N)], dict(act_out="swish"))
    add("lin/out_shape!", "linear_small_m", [D(bf(2, K)), D(bf(N, K)), None, D(bf(2, N + 1))], {})

    add("tsf/default", "timestep_features", [D(i64(B)), D(bf(B, 256))], {})
    add("tsf/shifted", "timestep_features", [D(i64(B)), D(bf(B, 256))], dict(flip_sin_to_cos=False, freq_shift=1.0))
    add("tsf/dtype!", "timestep_features", [D(i32(B)), D(bf(B, 256))], {})

    n_id, T = 3, 64
    sc = lambda dev: [dev(bf(n_id, T, 512)), dev(bf(n_id, 32, 512)), dev(bf(512)), dev(bf(512)), dev(bf(32, 512)), dev(bf(n_id, T, 32))]
    add("scores/launch", "router_scores", [*sc(D), n_id, T], {})
    add("scores/eps", "router_scores", [*sc(D), n_id, T], dict(eps=1e-6))
    add("scores_plan/meta", "router_scores_plan", [*sc(ident), n_id, T], {})
    add("scores_plan/device", "router_scores_plan", [*sc(D), n_id, T], {})
    add("scores/strided!", "router_scores", [D(bf(n_id, T, 1024))[..., :512], *sc(D)[1:], n_id, T], {})
    add("scores/dtype!", "router_scores", [*sc(D)[:5], D(f32(n_id, T, 32)), n_id, T], {})
    add("head/launch", "router_head", [D(bf(T, n_id, 32)), D(bf(32)), D(bf(1)), D(bf(T, n_id)), n_id, T], {})
    add("head/strided!", "router_head", [D(bf(T, n_id, 64))[..., :32], D(bf(32)), D(bf(1)), D(bf(T, n_id)), n_id, T], {})
    add("forcing/launch", "forcing_max_over_frames", [D(bf(1, 4 * 30, n_id)), D(bf(1, 30, n_id)), 4, 30, n_id], {})
    add("forcing/dtype!", "forcing_max_over_frames", [D(f32(1, 4 * 30, n_id)), D(bf(1, 30, n_id)), 4, 30, n_id], {})

    Dm = 64
    feat, r1, rB = (lambda: D(bf(B, n_id, T, Dm))), (lambda: D(bf(1, T, n_id))), (lambda: D(bf(B, T, n_id)))
    add("combine/face", "masked_combine", [D(bf(B, T, Dm)), feat(), r1(), None, "face"], {})
    add("combine/audio_view", "masked_combine", [D(bf(B, T + 4, 2 * Dm))[:, 4:, Dm:], feat(), rB(), D(bf(B, n_id, n_id)), "audio"], dict(alpha=0.5))
    add("combine/mode!", "masked_combine", [D(bf(B, T, Dm)), feat(), r1(), None, "video"], {})
    add("combine/r_shape!", "masked_combine", [D(bf(B, T, Dm)), feat(), D(bf(1, T + 1, n_id)), None, "face"], {})
    add("combine/x_dtype!", "masked_combine", [D(f32(B, T, Dm)), feat(), r1(), None, "face"], {})
    add("mixrows/face", "routed_mix", [feat(), r1(), None, "face", D(bf(B, T, Dm))], {})
    add("mixrows/audio_wsum", "routed_mix", [feat(), rB(), D(bf(B, n_id, n_id)), "audio", D(bf(B, T, Dm))], dict(wsum=D(f32(B, T))))
    add("mixrows/mode!", "routed_mix", [feat(), r1(), None, "video", D(bf(B, T, Dm))], {})
    add("mixrows/wsum_dtype!", "routed_mix", [feat(), r1(), None, "face", D(bf(B, T, Dm))], dict(wsum=D(bf(B, T))))

    add("patchify/launch", "patchify", [D(bf(1, 3, 16, 8, 12)), D(bf(1, 3 * 4 * 6, 64))], {})
    add("patchify/strided!", "patchify", [D(bf(1, 3, 16, 8, 24))[..., :12], D(bf(1, 3 * 4 * 6, 64))], {})
    add("unpatchify/launch", "unpatchify", [D(bf(1, 3 * 4 * 6, 64)), D(bf(1, 3, 16, 8, 12))], {})
    add("unpatchify/dtype!", "unpatchify", [D(f32(1, 3 * 4 * 6, 64)), D(bf(1, 3, 16, 8, 12))], {})

    n = 1000
    add("act/plain", "act_add", [D(bf(n)), D(bf(n))], {})
    add("act/silu_res", "act_add", [D(bf(4, 250)), D(bf(4, 250))], dict(act="silu", res=D(bf(2 * n))[n:]))
    add("act_plan/plain", "act_add_plan", [bf(n), bf(n)], {})
    add("act_plan/silu_res_device", "act_add_plan", [D(bf(4, 250)), D(bf(4, 250))], dict(act="silu", res=D(bf(2 * n))[n:]))
    add("act/act!", "act_add", [D(bf(n)), D(bf(n))], dict(act="swish"))
    add("act_plan/act!", "act_add_plan", [bf(n), bf(n)], dict(act="swish"))
    add("act/strided!", "act_add", [D(bf(n, 2))[:, 0], D(bf(n))], {})

    coef = dict(guidance=6.0, sqrt_alpha=0.8, sqrt_beta=0.6, k_sample=1.25, k_denoised=-0.5, k_noise=0.0, k_cur=1.5, k_old=-0.5)
    shape = (4, 6, 8)
    n = 4 * 6 * 8
    preds = lambda dev: {"one": dev(bf(1, *shape)), "two": dev(bf(2, *shape)), "one_of_wider": dev(bf(3, n + 64))[1:2, :n],
                         "two_of_wider": dev(bf(2, n + 64))[:, :n]}
    for name in preds(D):
        add(f"sched/{name}", "cfg_scheduler_step", [preds(D)[name], D(bf(1, *shape)), coef], dict(out=D(bf(1, *shape))))
        add(f"sched_plan/{name}", "cfg_scheduler_step_plan", [preds(ident)[name], bf(1, *shape), coef], {})
    add("sched/all_buffers", "cfg_scheduler_step", [D(bf(2, *shape)), D(bf(1, *shape)), coef],
        dict(old_x0=D(f32(1, *shape)), noise=D(bf(n)), x0_out=D(f32(n)), out=D(bf(n))))
    add("sched/out_allocated", "cfg_scheduler_step", [D(bf(2, *shape)), D(bf(1, *shape)), coef], {})
    add("sched_plan/out_device", "cfg_scheduler_step_plan", [D(bf(2, *shape)), D(bf(1, *shape)), coef], dict(out=D(bf(2, n))[1]))
    for fn, pre, dev in (("cfg_scheduler_step", "sched", D), ("cfg_scheduler_step_plan", "sched_plan", ident)):
        add(f"{pre}/three_predictions!", fn, [dev(bf(3, *shape)), dev(bf(1, *shape)), coef], {})
        add(f"{pre}/pred_dtype!", fn, [dev(f32(2, *shape)), dev(bf(1, *shape)), coef], {})
        add(f"{pre}/pred_rows_strided!", fn, [dev(bf(2, n, 2))[:, :, 0], dev(bf(1, *shape)), coef], {})
    add("sched/noise_dtype!", "cfg_scheduler_step", [D(bf(2, *shape)), D(bf(1, *shape)), coef], dict(noise=D(f32(n))))

    add("masks/launch", "masks_to_routing_logits", [D(u8(n_id, 5, 60, 90))], dict(out=D(bf(1, 13 * 30 * 45, n_id))))
    add("masks/small_grid", "masks_to_routing_logits", [D(u8(n_id, 5, 60, 90))], dict(frames=2, h=6, w=9, out=D(bf(1, 2 * 6 * 9, n_id))))
    add("masks/dtype!", "masks_to_routing_logits", [D(bf(n_id, 5, 60, 90))], dict(out=D(bf(1, 13 * 30 * 45, n_id))))


def rowk_cases(add):
    """The router's row kernels: the launches read packs, the queries a row count or the tensors."""
    R = 100

    def pack(dev, n, ln):
        return dict(w=dev(bf(n, 512)), colsum=dev(f32(n)) if ln else None, cvec=dev(f32(n)), ln=ln)

    rows = lambda dev: dev(bf(R, 512))
    view = lambda dev: dev(bf(R + 2, 1024))[2:, 512:]
    add("rowgemm/plain", "rowgemm512", [rows(D), pack(D, 64, False), D(bf(R, 64))], {})
    add("rowgemm/ln_res_gelu", "rowgemm512", [rows(D), pack(D, 512, True), D(bf(R, 512))], dict(res=D(bf(R, 512)), act="gelu_erf", eps=1e-6))
    add("rowgemm/views_nsplit", "rowgemm512", [view(D), pack(D, 1536, True), D(bf(R, 2048))[:, 512:]], dict(nsplit=512))
    add("rowgemm/res_view", "rowgemm512", [view(D), pack(D, 512, False), view(D)], dict(res=view(D)))
    add("rowgemm_plan/int_rows", "rowgemm512_plan", [R, 64], {})
    add("rowgemm_plan/int_rows_ln_res_gelu", "rowgemm512_plan", [R, 512], dict(ln=True, res=True, act="gelu_erf"))
    add("rowgemm_plan/tensors", "rowgemm512_plan", [rows(ident), 64], dict(out=bf(R, 64)))
    add("rowgemm_plan/views", "rowgemm512_plan", [view(ident), 512], dict(out=view(ident), res=view(ident), ln=True))
    add("rowgemm_plan/device", "rowgemm512_plan", [view(D), 512], dict(out=D(bf(R, 512)), res=True, act="silu"))
    add("rowgemm/k!", "rowgemm512", [D(bf(R, 256)), pack(D, 64, False), D(bf(R, 64))], {})
    add("rowgemm_plan/k!", "rowgemm512_plan", [bf(R, 256), 64], dict(out=bf(R, 64)))
    add("rowgemm/out_shape!", "rowgemm512", [rows(D), pack(D, 64, False), D(bf(R + 1, 64))], {})
    add("rowgemm_plan/out_shape!", "rowgemm512_plan", [rows(ident), 64], dict(out=bf(R + 1, 64)))
    add("rowgemm/res_shape!", "rowgemm512", [rows(D), pack(D, 64, False), D(bf(R, 64))], dict(res=D(bf(R, 128))))
    add("rowgemm_plan/res_shape!", "rowgemm512_plan", [rows(ident), 64], dict(out=bf(R, 64), res=bf(R, 128)))
    add("rowgemm/x_inner_stride!", "rowgemm512", [D(bf(R, 1024))[:, ::2], pack(D, 64, False), D(bf(R, 64))], {})
    add("rowgemm_plan/x_inner_stride!", "rowgemm512_plan", [bf(R, 1024)[:, ::2], 64], dict(out=bf(R, 64)))
    add("rowgemm/act!", "rowgemm512", [rows(D), pack(D, 64, False), D(bf(R, 64))], dict(act="swish"))
    add("rowgemm_plan/act!", "rowgemm512_plan", [R, 64], dict(act="swish"))

    geo = [4, 5, 5, 20, 1]                           # L, n_outer, n_inner, outer_stride, seq_stride: 25 groups of 4 rows
    add("group_attn/plain", "router_group_attn", [rows(D), pack(D, 1536, True), D(bf(R + 1, 512))[1:], *geo], {})
    add("group_attn/views", "router_group_attn", [view(D), pack(D, 1536, True), D(bf(R, 1024))[:, :512], *geo], dict(eps=1e-6, scale=0.25))
    add("group_attn_plan/int_rows", "router_group_attn_plan", [R, *geo], {})
    add("group_attn_plan/views", "router_group_attn_plan", [view(ident), *geo], dict(out=bf(R, 1024)[:, :512]))
    add("group_attn_plan/device", "router_group_attn_plan", [rows(D), *geo], dict(out=D(bf(R, 512))))
    add("group_attn/k!", "router_group_attn", [D(bf(R, 256)), pack(D, 1536, True), D(bf(R, 512)), *geo], {})
    add("group_attn_plan/k!", "router_group_attn_plan", [bf(R, 256), *geo], {})
    add("group_attn/out_shape!", "router_group_attn", [rows(D), pack(D, 1536, True), D(bf(R, 256)), *geo], {})
    add("group_attn_plan/out_shape!", "router_group_attn_plan", [rows(ident), *geo], dict(out=bf(R, 256)))
    add("group_attn/pack!", "router_group_attn", [rows(D), pack(D, 512, True), D(bf(R, 512)), *geo], {})
    add("group_attn/in_place!", "router_group_attn", [D(bf(R, 1024))[:, :512], pack(D, 1536, True), D(bf(R, 1024))[:, :512], *geo], {})

    add("mlp/in_place", "router_mlp_fused", [rows(D), pack(D, 512, True), pack(D, 512, False)], {})
    add("mlp/out_view_tp0", "router_mlp_fused", [view(D), pack(D, 512, True), pack(D, 512, False)], dict(eps=1e-6, out=D(bf(R, 512)), tiles_pass0=3))
    add("mlp_plan/int_rows", "router_mlp_fused_plan", [R], {})
    add("mlp_plan/in_place_view_tp0", "router_mlp_fused_plan", [view(ident)], dict(tiles_pass0=3))
    add("mlp_plan/out_device", "router_mlp_fused_plan", [view(D)], dict(out=D(bf(R, 512))))
    add("mlp/k!", "router_mlp_fused", [D(bf(R, 256)), pack(D, 512, True), pack(D, 512, False)], {})
    add("mlp_plan/k!", "router_mlp_fused_plan", [bf(R, 256)], {})
    add("mlp/out_shape!", "router_mlp_fused", [rows(D), pack(D, 512, True), pack(D, 512, False)], dict(out=D(bf(R + 1, 512))))
    add("mlp_plan/out_shape!", "router_mlp_fused_plan", [rows(ident)], dict(out=bf(R + 1, 512)))
    add("mlp/packs_swapped!", "router_mlp_fused", [rows(D), pack(D, 512, False), pack(D, 512, True)], {})

    add("attn_out/in_place", "router_group_attn_out", [rows(D), pack(D, 1536, True), pack(D, 512, False), *geo], {})
    add("attn_out/out_view_tp0", "router_group_attn_out", [view(D), pack(D, 1536, True), pack(D, 512, False), *geo],
        dict(eps=1e-6, scale=0.25, out=D(bf(R, 512)), tiles_pass0=2))
    add("attn_out_plan/int_rows", "router_group_attn_out_plan", [R, *geo], {})
    add("attn_out_plan/in_place_view_tp0", "router_group_attn_out_plan", [view(ident), *geo], dict(tiles_pass0=2))
    add("attn_out_plan/out_device", "router_group_attn_out_plan", [view(D), *geo], dict(out=D(bf(R, 512))))
    add("attn_out/k!", "router_group_attn_out", [D(bf(R, 256)), pack(D, 1536, True), pack(D, 512, False), *geo], {})
    add("attn_out_plan/k!", "router_group_attn_out_plan", [bf(R, 256), *geo], {})
    add("attn_out/out_shape!", "router_group_attn_out", [rows(D), pack(D, 1536, True), pack(D, 512, False), *geo], dict(out=D(bf(R, 256))))
    add("attn_out_plan/out_shape!", "router_group_attn_out_plan", [rows(ident), *geo], dict(out=bf(R, 256)))
    add("attn_out/pack_out_ln!", "router_group_attn_out", [rows(D), pack(D, 1536, True), pack(D, 512, True), *geo], {})


def vae_cases(add):
    Ts, Hs, Ws, C = 3, 6, 8, 32
    x = lambda: D(bf(Ts, Hs, Ws, C))
    add("vae/patches", "vae_patches", [x(), None, D(bf(Ts * Hs * Ws, 9 * 3 * C)), 3, 1, 1, False, 0, Hs, Ws, 0, Ts], {})
    add("vae/patches_cache_up", "vae_patches", [x(), D(bf(2, Hs, Ws, C)), D(bf(2 * 2 * Hs * 2 * Ws, 9 * 3 * C + 32)), 3, 1, 1, True, 1, 2 * Hs, 2 * Ws,
                                                1, 2], {})
    add("vae/patches_cache_shape!", "vae_patches", [x(), D(bf(1, Hs, Ws, C)), D(bf(Ts * Hs * Ws, 9 * 3 * C)), 3, 1, 1, False, 0, Hs, Ws, 0, Ts], {})
    add("vae/patches_rows!", "vae_patches", [x(), None, D(bf(Ts * Hs * Ws + 1, 9 * 3 * C)), 3, 1, 1, False, 0, Hs, Ws, 0, Ts], {})
    rows = Ts * Hs * Ws
    add("vae/gn_stats", "vae_groupnorm_stats", [D(bf(rows, C)), D(f32(2 * 8)), 8], dict(partial=D(f32(16))))
    add("vae/gn_stats_many_rows", "vae_groupnorm_stats", [D(bf(1100, C)), D(f32(2, 4)), 4], dict(partial=D(f32(64))))
    add("vae/gn_stats_sums!", "vae_groupnorm_stats", [D(bf(rows, C)), D(f32(8)), 8], dict(partial=D(f32(16))))
    add("vae/gn_stats_partial_short!", "vae_groupnorm_stats", [D(bf(1100, C)), D(f32(2, 4)), 4], dict(partial=D(f32(16))))
    na = lambda: [D(f32(16)), D(bf(C)), D(bf(C)), 8]
    add("vae/norm_act", "vae_norm_act", [x(), x(), *na()], {})
    add("vae/norm_act_pad_none", "vae_norm_act", [x(), D(bf(Ts + 2, Hs + 2, Ws + 2, C)), *na()], dict(act=None, eps=1e-5, out_pad=True))
    add("vae/norm_act_spatial", "vae_norm_act", [x(), x(), *na()],
        dict(zy=D(bf(2 * 3 * 4, 2 * C))[:, :C], zb=D(bf(2 * 3 * 4, 2 * C))[:, C:], latent_shape=(2, 3, 4), tmode=2))
    add("vae/norm_act_y_shape!", "vae_norm_act", [x(), D(bf(Ts, Hs, Ws + 2, C)), *na()], {})
    add("vae/norm_act_act!", "vae_norm_act", [x(), x(), *na()], dict(act="gelu"))
    Co = 16
    xpad = lambda kt: D(bf(Ts + kt - 1, Hs + 2, Ws + 2, C))
    add("vae/conv3d", "vae_conv3d", [xpad(3), D(bf(Co, 27 * C)), D(bf(Co)), D(bf(Ts, Hs, Ws, Co))], {})
    add("vae/conv3d_kt1_res_views", "vae_conv3d", [xpad(1), D(bf(Co + 16, 9 * C + 32)), None, D(bf(Ts, Hs, Ws, 2 * Co))[..., Co:]],
        dict(res=D(bf(Ts, Hs, Ws, 3 * Co))[..., :Co], KT=1))
    add("vae/conv3d_pad!", "vae_conv3d", [xpad(1), D(bf(Co, 27 * C)), None, D(bf(Ts, Hs, Ws, Co))], {})
    add("vae/conv3d_res_shape!", "vae_conv3d", [xpad(3), D(bf(Co, 27 * C)), None, D(bf(Ts, Hs, Ws, Co))], dict(res=D(bf(Ts, Hs, Ws, 2 * Co))))
    add("vae/conv3d_out_rows!", "vae_conv3d", [xpad(3), D(bf(Co, 27 * C)), None, D(bf(Ts, Hs + 1, Ws, Co))[:, :Hs]], {})
    for tmode, To in ((0, Ts), (1, 2 * Ts), (2, 2 * Ts - 1)):
        add(f"vae/upsample_pad_t{tmode}", "vae_upsample_pad", [x(), D(bf(To, 2 * Hs + 2, 2 * Ws + 2, C)), tmode], {})
    add("vae/upsample_pad_shape!", "vae_upsample_pad", [x(), D(bf(2 * Ts, 2 * Hs + 2, 2 * Ws + 2, C)), 2], {})


def cases():
    """-> [(case id, name of the ops function, positional arguments, keyword arguments)]; an id ending in "!" is refused."""
    out = []
    add = lambda cid, fn, args, kw: out.append((cid, fn, args, kw))
    norm_cases(add)
    attn_cases(add)
    step_cases(add)
    rowk_cases(add)
    vae_cases(add)
    assert len({c[0] for c in out}) == len(out)
    return out


def _returned(ret, args, kw):
    """What came back, by the argument it is: "arg2", "kw:out", "kw:mx_out[0]"; a dict (a query's answer), True / False / None;
    a tuple of these; or, for a tensor the wrapper allocated, its shape."""
    if ret is None or isinstance(ret, (bool, dict)):
        return ret
    if isinstance(ret, tuple):
        return [_returned(r, args, kw) for r in ret]
    named = [(f"arg{i}", a) for i, a in enumerate(args)] + [(f"kw:{k}", v) for k, v in kw.items()]
    for name, a in named:
        if a is ret:
            return name
        if isinstance(a, tuple):
            for j, e in enumerate(a):
                if e is ret:
                    return f"{name}[{j}]"
    return f"new {type(ret).__name__} {list(ret.shape)} {ret.dtype}"


def record(monkeypatch_setattr):
    """Run the table against the stub -> {case id: {"calls": [[entry point, arguments]], "returns", "raises": type name or None}}."""
    from bind_your_avatar_implementation_amd import _hip, ops
    monkeypatch_setattr(ops, "_stream", lambda: STREAM)
    monkeypatch_setattr(ops, "_ATTN_WS", {None: "registered"})            # (a FakeDevice tensor's device has no index)
    monkeypatch_setattr(ops, "_TIMERS", None)
    monkeypatch_setattr(ops, "ATTN_VARIANTS", {})
    seen = {}
    for cid, fn, args, kw in cases():
        stub = StubLibrary()
        monkeypatch_setattr(_hip, "load", lambda stub=stub: stub)
        raised, ret = None, None
        try:
            ret = _returned(getattr(ops, fn)(*args, **kw), args, kw)
        except Exception as e:                                           # (the type is what is pinned)
            raised = type(e).__name__
        seen[cid] = {"calls": stub.calls, "returns": ret, "raises": raised}
    return seen, dict(ops.ATTN_VARIANTS)


@pytest.fixture(scope="module")
def recorded():
    with pytest.MonkeyPatch.context() as mp:
        return record(mp.setattr)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(recorded, golden):
    assert sorted(recorded[0]) == sorted(golden)
    assert 150 <= len(golden) <= 500


def test_refused_cases_raise_before_the_library_is_asked(recorded):
    for cid, got in recorded[0].items():
        if cid.endswith("!"):
            assert got["raises"] in ("ValueError", "TypeError", "AssertionError", "KeyError"), (cid, got["raises"])
            assert got["calls"] == [], cid
        else:
            assert got["raises"] is None and got["calls"], (cid, got["raises"])


GROUPS = ["ln", "ln_plan", "qkn", "qkn_plan", "attn", "attn_plan", "self", "mix", "mix_plan", "tiny", "tiny_plan", "quant", "lin", "lin_plan",
          "tsf", "scores", "scores_plan", "head", "forcing", "combine", "mixrows", "patchify", "unpatchify", "act", "act_plan", "sched",
          "sched_plan", "masks", "rowgemm", "rowgemm_plan", "group_attn", "group_attn_plan", "mlp", "mlp_plan", "attn_out", "attn_out_plan",
          "vae"]


@pytest.mark.parametrize("group", GROUPS)
def test_call_sequence_arguments_and_return(recorded, golden, group):
    ids = [c for c in golden if c.split("/")[0] == group]
    assert ids
    for cid in ids:
        assert json.loads(json.dumps(recorded[0][cid])) == golden[cid], cid


def test_every_group_is_compared(golden):
    assert {c.split("/")[0] for c in golden} == set(GROUPS)


def test_attention_launches_are_counted_by_tag_and_variant(recorded):
    """The stub's ``bya_attn_variant`` answers 0: every launch counts under its tag and variant 0's name; queries count nothing."""
    launches = {}
    for cid, fn, _, kw in cases():
        if fn in ("attention", "self_attention") and not cid.endswith("!"):
            key = (kw.get("tag", "other"), "d64_running_max")
            launches[key] = launches.get(key, 0) + 1
    assert recorded[1] == launches and set(k[0] for k in launches) == {"other", "self", "cross"}


def test_the_recording_covers_what_it_should(golden):
    entries = {c[0] for g in golden.values() for c in g["calls"]}
    launches = {"bya_quantize_rows_fp8", "bya_quantize_mx", "bya_linear_small_m", "bya_timestep_features", "bya_layernorm", "bya_layernorm_fp8",
                "bya_layernorm_mx", "bya_qknorm_rope", "bya_attn_fwd", "bya_attn_fwd_mx", "bya_attn_kv_mix", "bya_attn_kv_mix_mx",
                "bya_attn_tiny", "bya_router_scores", "bya_router_head", "bya_forcing_max_over_frames", "bya_masked_combine",
                "bya_routed_mix", "bya_patchify", "bya_unpatchify", "bya_act_add", "bya_cfg_scheduler_step", "bya_masks_to_routing_logits",
                "bya_rowgemm512", "bya_router_group_attn", "bya_router_mlp_fused", "bya_router_group_attn_out", "bya_vae_patches",
                "bya_vae_groupnorm_stats", "bya_vae_norm_act", "bya_vae_conv3d", "bya_vae_upsample_pad"}
    plans = {"bya_linear_small_m_plan", "bya_layernorm_plan", "bya_qknorm_rope_plan", "bya_attn_plan", "bya_attn_mx_plan",
             "bya_attn_kv_mix_plan", "bya_attn_kv_mix_mx_plan", "bya_attn_tiny_plan", "bya_router_scores_plan", "bya_act_add_plan",
             "bya_cfg_scheduler_step_plan", "bya_rowgemm512_plan", "bya_router_group_attn_plan", "bya_router_mlp_fused_plan",
             "bya_router_group_attn_out_plan"}
    assert entries == launches | plans | {"bya_attn_variant"}
    for cid, g in golden.items():
        names = [c[0] for c in g["calls"]]
        if names and names[-1] in launches:                              # every launch ends with the stream
            assert g["calls"][-1][1][-1] == STREAM, cid
        if names and names[-1] in ("bya_attn_fwd", "bya_attn_fwd_mx"):   # the variant query, then the launch
            assert names[:-1] == ["bya_attn_variant"], cid
        elif names and names[0] in ("bya_attn_plan", "bya_attn_mx_plan"):
            assert names[1:] == ["bya_attn_variant"], cid
        else:
            assert len(names) <= 1, cid
    raises = {cid: g["raises"] for cid, g in golden.items() if g["raises"]}
    assert all(cid.endswith("!") for cid in raises)
    # the members of a pair refuse the same inputs with the same exception
    for cid, kind in raises.items():
        group, _, rest = cid.partition("/")
        twin = f"{group}_plan/{rest}"
        if twin in raises:
            assert raises[twin] == kind, cid


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with pytest.MonkeyPatch.context() as mp:
        table, _ = record(mp.setattr)
    with open(GOLDEN, "w") as f:                                         # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(table[cid])}" for cid in sorted(table)) + "\n}\n")
    print(f"{len(table)} cases -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
