"""CPU: the C ABI of the kv-mix whose epilogue writes MX codes (include/bya.h, bya_attn_kv_mix_mx / bya_attn_kv_mix_mx_plan) --
error codes before any launch and the plan against bya_attn_kv_mix_plan's --, the two cross-attention output projections in
enable_mx_weights(linears=...) / enable_fp8_weights, and the byte layout of the codes and scales restated in torch."""
import ctypes
import types

import pytest
import torch

from test_mx_cpu import BITS, quant_mx_ref

OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
E4M3, E2M3, E2M1 = 0, 2, 4
BASE = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    return _hip.load()


def desc(D=64, H=48, n_id=2, n_grp=13, Sq=1350, Skv=32):
    from bind_your_avatar_implementation_amd import _hip
    d = _hip.AttnMixDesc()
    d.head_dim, d.heads, d.n_id, d.n_grp, d.Sq, d.Skv = D, H, n_id, n_grp, Sq, Skv
    d.q_row = d.k_row = d.v_row = H * D
    d.q_grp, d.k_grp, d.v_grp, d.k_id, d.v_id = Sq * H * D, Skv * H * D, Skv * H * D, n_grp * Skv * H * D, n_grp * Skv * H * D
    d.scale = D ** -0.5
    return d


def strides(d, fmt):
    cb = d.heads * d.head_dim * (8 if fmt == E4M3 else 6) // 8
    sb = d.heads * d.head_dim // 32
    return [d.Sq * cb, cb, d.Sq * sb, sb]


def plan_fields(p):
    return (p.form, p.head_dim, p.grid, p.row_chunks, p.lds_bytes, p.big_lds)


def test_binding_table_has_the_two_entry_points(lib):
    from bind_your_avatar_implementation_amd import _hip
    for name, nargs in (("bya_attn_kv_mix_mx", 15), ("bya_attn_kv_mix_mx_plan", 10)):
        assert len(_hip.SIGNATURES[name]) == nargs and hasattr(lib, name)


def test_error_codes_before_any_launch(lib):
    from bind_your_avatar_implementation_amd import _hip

    def launch(d, fmt, st, q=BASE, codes=BASE, scales=BASE, af=None):
        return lib.bya_attn_kv_mix_mx(q, BASE, BASE, BASE, af, codes, scales, None, ctypes.byref(d), fmt, *st, None)

    def plan(d, fmt, st, codes=BASE, scales=BASE, af=None, out=None):
        out = _hip.AttnMixPlan(-9) if out is None else out
        return lib.bya_attn_kv_mix_mx_plan(codes, scales, af, ctypes.byref(d), fmt, *st, ctypes.byref(out)), out

    for fn in (lambda *a, **k: launch(*a, **k), lambda *a, **k: plan(*a, **k)[0]):
        d = desc()
        st = strides(d, E2M3)
        assert fn(d, E2M1, st) == ERR_UNSUPPORTED                       # e2m1 is never an activation format
        assert fn(d, 1, st) == ERR_UNSUPPORTED
        assert fn(d, E2M3, st, codes=None) == ERR_SHAPE and fn(d, E2M3, st, scales=None) == ERR_SHAPE
        d40 = desc(Skv=40)
        assert fn(d40, E2M3, st) == ERR_UNSUPPORTED                     # the MX epilogue exists on the <= 32-key form alone
        assert fn(desc(Skv=65), E2M3, st) == ERR_SHAPE                  # ... and what bya_attn_kv_mix refuses stays refused
        assert fn(desc(D=96), E2M3, st) == ERR_UNSUPPORTED
        dz = desc()
        dz.z_row = 3072
        assert fn(dz, E2M3, st) == ERR_SHAPE                            # there is no bf16 output
        dz.z_row, dz.z_grp = 0, 8
        assert fn(dz, E2M3, st) == ERR_SHAPE
        assert fn(d, E2M3, st, codes=BASE + 2) == ERR_ALIGN
        assert fn(d, E2M3, [st[0], st[1] + 2, st[2], st[3]]) == ERR_ALIGN
        assert fn(d, E2M3, [st[0] + 2, st[1], st[2], st[3]]) == ERR_ALIGN
        assert fn(d, E2M3, [st[0], st[1] - 4, st[2], st[3]]) == ERR_SHAPE                     # c_row too short for the heads
        assert fn(d, E4M3, st) == ERR_SHAPE                                                   # ... e2m3's row under e4m3
        assert fn(d, E2M3, [st[0], st[1], st[2], st[3] - 1]) == ERR_SHAPE                     # sc_row too short
        assert fn(d, E2M3, [-4, st[1], st[2], st[3]]) == ERR_SHAPE
        one = desc(n_id=1)
        assert fn(one, E2M3, st, af=BASE) == ERR_SHAPE                  # audio weights need >= 2 streams
        dq = desc()
        dq.q_row = 3076
        assert fn(dq, E2M3, st) == ERR_ALIGN
    d = desc()
    assert launch(d, E2M3, strides(d, E2M3), q=None) == ERR_SHAPE
    assert launch(d, E2M3, strides(d, E2M3), q=BASE + 8) == ERR_ALIGN
    assert lib.bya_attn_kv_mix_mx_plan(BASE, BASE, None, ctypes.byref(d), E2M3, *strides(d, E2M3), None) == ERR_SHAPE
    assert lib.bya_attn_kv_mix_mx_plan(BASE, BASE, None, None, E2M3, *strides(d, E2M3), ctypes.byref(_hip.AttnMixPlan())) == ERR_SHAPE
    rc, p = plan(desc(Skv=40), E2M3, strides(d, E2M3))
    assert rc == ERR_UNSUPPORTED and p.form == -9                       # untouched on rejection
    # the generic-form reference option: refused as well (the caller then issues the two launches)
    _hip.set_option("reference_forms", _hip.REFERENCE_FORMS["kv_mix_generic"])
    try:
        assert plan(d, E2M3, strides(d, E2M3))[0] == ERR_UNSUPPORTED
        assert launch(d, E2M3, strides(d, E2M3)) == ERR_UNSUPPORTED
    finally:
        _hip.set_option("reference_forms", 0)
    assert plan(d, E2M3, strides(d, E2M3))[0] == OK
    assert plan(d, E2M3, strides(d, E2M3), codes=BASE + 4, scales=BASE + 1)[0] == OK          # 4-byte codes, any scale address


@pytest.mark.parametrize("D,H,n_id,n_grp,Sq,Skv", [(64, 48, 2, 13, 1350, 32), (128, 16, 2, 1, 17550, 32), (128, 2, 4, 2, 420, 20),
                                                   (64, 3, 3, 1, 45, 32), (64, 48, 2, 1, 29, 32)])
@pytest.mark.parametrize("fmt", [E4M3, E2M3])
def test_plan_equals_the_bf16_launch_plan(lib, D, H, n_id, n_grp, Sq, Skv, fmt):
    from bind_your_avatar_implementation_amd import _hip
    d = desc(D, H, n_id, n_grp, Sq, Skv)
    mp, bp = _hip.AttnMixPlan(-9), _hip.AttnMixPlan(-8)
    assert lib.bya_attn_kv_mix_mx_plan(BASE + 4, BASE + 3, None, ctypes.byref(d), fmt, *strides(d, fmt), ctypes.byref(mp)) == OK
    d.z_grp, d.z_row = Sq * H * D, H * D
    assert lib.bya_attn_kv_mix_plan(BASE, None, ctypes.byref(d), ctypes.byref(bp)) == OK
    assert plan_fields(mp) == plan_fields(bp) and mp.form == 0
    assert mp.big_lds == (1 if (D, n_id) == (128, 4) else 0)


def test_ops_front_end_refuses_a_bf16_output_next_to_mx_out():
    from bind_your_avatar_implementation_amd import ops
    kw = dict(head_dim=64, heads=3, n_id=2, n_grp=1, Sq=45, Skv=32, q_strides=(0, 192), k_strides=(32 * 192, 0, 192),
              v_strides=(32 * 192, 0, 192))
    c = torch.empty(45, 144, dtype=torch.uint8, device="meta")
    s = torch.empty(45, 6, dtype=torch.uint8, device="meta")
    z = torch.empty(45, 192, dtype=torch.bfloat16, device="meta")
    with pytest.raises(ValueError, match="no bf16 output"):
        ops.attn_kv_mix_plan(z, None, mx_out=(c, s, "mxfp6"), **kw)
    with pytest.raises(ValueError, match="no bf16 output"):
        ops.attn_kv_mix_plan(None, None, z_strides=(0, 192), mx_out=(c, s, "mxfp6"), **kw)
    with pytest.raises(ValueError):
        ops.attn_kv_mix_plan(None, None, mx_out=(c, s, "mxfp4"), **kw)                       # never an activation format
    with pytest.raises(ValueError):
        ops.attn_kv_mix_plan(None, None, mx_out=(c[:, :140], s, "mxfp6"), **kw)             # too narrow for the heads
    p = ops.attn_kv_mix_plan(None, None, mx_out=(c, s, "mxfp6"), **kw)
    assert p["form"] == "mix32" and p["mx_out"] == "mxfp6"
    assert p == dict(ops.attn_kv_mix_plan(z, None, z_strides=(0, 192), **kw), mx_out="mxfp6")
    assert ops.attn_kv_mix_plan(None, None, mx_out=(c, s, "mxfp6"), **dict(kw, Skv=40)) is None


def test_linear_selection_admits_the_cross_attention_out_projections():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel as Model
    from bind_your_avatar_implementation_amd import engine
    assert engine.MX_CROSS_OUT == ("po", "ao")
    assert engine.FP8_LINEARS == ("qkv", "out", "ff1", "ff2", "pq", "aq") and engine.FP8_DEFAULT == ("qkv", "out", "ff1", "ff2")
    fake = types.SimpleNamespace(invalidate_engine=lambda: None)
    Model.enable_mx_weights(fake, "mxfp8", linears=("ff1", "ao"))
    assert fake._mx_linears == ("ff1", "ao") and engine.mx_linears_of(fake) == {"ff1", "ao"}
    assert not hasattr(fake, "_mx_fuse_cross_attention_quant")                                # absent = the default, on
    Model.enable_mx_weights(fake, "mxfp8", linears="qkv,po", fuse_cross_attention_quant=False)
    assert engine.mx_linears_of(fake) == {"qkv", "po"} and fake._mx_fuse_cross_attention_quant is False
    Model.enable_mx_weights(fake, "mxfp8", linears="all")
    assert fake._mx_linears == "all" and engine.mx_linears_of(fake) == set(engine.FP8_LINEARS)   # "all": the six existing kinds
    assert not hasattr(fake, "_mx_fuse_cross_attention_quant")
    Model.enable_mx_weights(fake, "mxfp8")
    assert engine.mx_linears_of(fake) == set(engine.FP8_DEFAULT)
    Model.enable_mx_weights(fake, "mxfp8", linears=("po", "nope"))
    with pytest.raises(ValueError, match="MX linears"):
        engine.mx_linears_of(fake)
    with pytest.raises(TypeError):
        Model.enable_mx_weights(fake, "mxfp8", fuse_cross_attention_quant=1)
    # per-row fp8 needs the whole row's amax, which no attention epilogue has: the fp8 mode keeps refusing the two names
    Model.enable_fp8_weights(fake, linears=("po",))
    with pytest.raises(ValueError, match="fp8 linears"):
        engine.fp8_linears_of(fake)
    Model.enable_fp8_weights(fake, linears="ff1,ao")
    with pytest.raises(ValueError, match="fp8 linears"):
        engine.fp8_linears_of(fake)
    Model.enable_fp8_weights(fake, linears="all")
    assert engine.fp8_linears_of(fake) == set(engine.FP8_LINEARS)


@pytest.mark.parametrize("D,H", [(64, 3), (128, 2)])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp6"])
def test_byte_offsets_of_a_head_block(D, H, fmt):
    """include/bya.h: block j of head h of a row sits at byte (h * D + 32 j) * bits / 8 of the row's codes and its scale at
    byte h * D / 32 + j -- on the restatement of bya_quantize_mx for the [rows, H * D] matrix: changing one block's values
    changes exactly those bytes."""
    g = torch.Generator().manual_seed(D + H)
    x = torch.randn(4, H * D, generator=g).to(torch.bfloat16)
    c0, s0 = quant_mx_ref(x, fmt)
    bb = 32 * BITS[fmt] // 8
    assert c0.shape == (4, H * D * BITS[fmt] // 8) and s0.shape == (4, H * D // 32)
    for h in range(H):
        for j in range(D // 32):
            y = x.clone()
            col = h * D + 32 * j
            y[2, col:col + 32] = (x[2, col:col + 32].float() * -37.0).to(torch.bfloat16)
            c1, s1 = quant_mx_ref(y, fmt)
            off = (h * D + 32 * j) * BITS[fmt] // 8
            dc, ds = (c1 != c0).nonzero(), (s1 != s0).nonzero()
            assert dc.numel() and bool((dc[:, 0] == 2).all()) and off <= int(dc[:, 1].min()) and int(dc[:, 1].max()) < off + bb
            assert ds.tolist() == [[2, h * D // 32 + j]]
            # the lane of chunk ch (8 columns) owns bytes off + ch' * bits of the block, ch' = ch % 4: its 8 codes alone
            lane = y.clone()
            lane[2, col + 8:col + 16] = 0
            c2, _ = quant_mx_ref(lane, fmt)
            d2 = (c2 != c1).nonzero()[:, 1]
            if int(y[2, col:col + 32].abs().argmax()) // 8 != 1:                              # (the block's scale did not move)
                assert off + BITS[fmt] <= int(d2.min()) and int(d2.max()) < off + 2 * BITS[fmt]
