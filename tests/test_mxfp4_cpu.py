"""CPU: the e2m1 (MXFP4) weight format of include/bya.h ("MX weights") restated in torch on top of tests/test_mx_cpu.py -- the
8 magnitudes, the rounding, the nibble packing, the block rule -- plus the argument checks of bya_gemm_mx_mixed and of
enable_mx_weights(weight_format=...) (nothing is launched).  tests/test_mxfp4_gpu.py compares the kernels with this
restatement, byte for byte."""
import ctypes
import types

import numpy as np
import pytest
import torch

from mx_ref import (dequant, dequant_mx, e2m1_decode, e2m1_encode, e2m1_encode_nearest, e2m1_values, pack4,  # noqa: F401
                    quant_mx_ref, quant_ref, unpack4)

E4M3, E2M3, E2M1 = 0, 2, 4
T128X128, T256X256 = 1, 3


def test_e2m1_codes_are_fixed_points_ties_go_to_even_and_nibbles_round_trip():
    codes = torch.arange(16)
    assert torch.equal(e2m1_encode_nearest(e2m1_decode(codes)), codes)
    assert torch.equal(e2m1_encode(e2m1_decode(codes)), codes)
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], dtype=torch.float64)
    for enc in (e2m1_encode_nearest, e2m1_encode):
        assert e2m1_decode(enc(ties)).tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
        assert e2m1_decode(enc(-ties)).tolist() == [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
        above = torch.tensor([6.0001, 7.0, 7.99, 100.0, -6.5, -1e30], dtype=torch.float64)
        assert e2m1_decode(enc(above)).tolist() == [6.0, 6.0, 6.0, 6.0, -6.0, -6.0]
    g = torch.Generator().manual_seed(0)
    c = torch.randint(0, 16, (7, 128), generator=g)
    b = pack4(c)
    assert b.shape == (7, 64) and torch.equal(unpack4(b), c)
    assert torch.equal(pack4(unpack4(b)), b)
    assert pack4(torch.tensor([0x3, 0xA])).tolist() == [0xA3]                         # element 0 = the low nibble


def test_binade_rint_form_of_e2m1_rounding_equals_the_nearest_code_definition():
    """The arithmetic of f32_to_e2m1 (rint of the value counted in steps of its binade, after the clamp at 6), in numpy on
    fp32 as the kernel does it, against the nearest-code definition: 400k random values in (-8, 8), every code plus and minus
    a quarter step, and +-0."""
    g = torch.Generator().manual_seed(0)
    vals = e2m1_values().float()
    step = torch.tensor([0.5, 0.5, 0.5, 0.5, 1.0, 1.0, 2.0, 2.0])
    near = torch.cat([vals + step / 4, vals - step / 4])
    v = torch.cat([torch.rand(400_000, generator=g) * 16 - 8, near, -near, torch.tensor([0.0, -0.0])]).float()
    a = np.minimum(np.abs(v.numpy()), np.float32(6.0))
    c = np.where(a < 2, np.rint(a * 2), np.where(a < 4, np.rint(a) + 2, np.rint(a * np.float32(0.5)) + 4)).astype(np.int64)
    c |= (v.numpy().view(np.uint32) >> 28).astype(np.int64) & 8
    nearest = e2m1_encode_nearest(v.double())
    assert np.array_equal(c, nearest.numpy())
    assert torch.equal(e2m1_encode(v.double()), nearest)


def test_block_rule_zero_blocks_subnormals_outliers_and_round_trip():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(3, 256, generator=g) * 5).to(torch.bfloat16)
    x[0, :32] = 0                                     # all-zero block: byte 127, zero codes
    x[0, 32:64] = -0.0                                # (-0 too)
    x[1, 64:96] = torch.tensor([2.0 ** -130] * 32).to(torch.bfloat16)       # subnormal block maximum: E clamps at -127
    x[2, :32] = 0.5
    x[2, 3] = 3e38                                    # an outlier sets its block's scale and nothing else
    codes, scales = quant_ref(x, "mxfp4")
    assert codes.shape == (3, 128) and scales.shape == (3, 8)
    assert scales[0, 0] == 127 and scales[0, 1] == 127 and (codes[0, :32] == 0).all()
    assert scales[1, 2] == 0
    assert scales[2, 0] == 127 + 127 - 2
    calm = x.clone()
    calm[2, 3] = 0.5
    _, s_calm = quant_ref(calm, "mxfp4")
    assert torch.equal(s_calm[2, 1:], scales[2, 1:]) and torch.equal(s_calm[:2], scales[:2]) and s_calm[2, 0] != scales[2, 0]
    back = dequant(codes, scales, "mxfp4")
    # block-relative error: amax * 2^-E lies in [4, 8).  Half an element step of the top binade is 1 of at least 4; the
    # saturation of a block maximum in (6, 8) loses less than 2 of at most 8: 1/4 either way (derived, not measured)
    blk = x.double().reshape(3, 8, 32)
    err = (back.reshape(3, 8, 32) - blk).abs().amax(-1) / blk.abs().amax(-1).clamp_min(1e-300)
    assert float(err[2:, 1:].max()) <= 2.0 ** -2 and float(err[0, 2:].max()) <= 2.0 ** -2
    assert torch.equal(pack4(unpack4(codes)), codes)


def test_mixed_entry_points_reject_bad_arguments_without_launching():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    lib = _hip.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    d = _hip.GemmDesc()
    d.M, d.N, d.K, d.batch, d.lda, d.ldw, d.ldc = 16, 16, 128, 1, 96, 64, 16

    def mixed(a_fmt, w_fmt, ptr=p):
        return lib.bya_gemm_mx_mixed(ptr, ptr, ptr, ptr, None, ptr, None, None, None, ctypes.byref(d), a_fmt, w_fmt, None)

    assert mixed(E2M3, E2M1, ptr=None) == -1
    assert mixed(E2M1, E2M1) < 0 and mixed(E2M1, E2M3) < 0              # e2m1 activations are not offered
    assert mixed(E2M3, 1) < 0 and mixed(E4M3, 1) < 0                    # no format 1
    d.lda = d.ldw = 128
    assert mixed(E4M3, E2M3) < 0 and mixed(E2M3, E4M3) < 0              # no other mixed pair
    d.K, d.lda, d.ldw = 192, 144, 96
    assert mixed(E2M3, E2M1) < 0                                         # K % 128
    d.K, d.lda, d.ldw = 256, 192, 112
    assert mixed(E2M3, E2M1) < 0                                         # ldw below K / 2
    d.lda, d.ldw = 176, 128
    assert mixed(E2M3, E2M1) < 0                                         # lda below the e2m3 row bytes
    assert lib.bya_quantize_mx(None, None, None, 4, 128, 128, E2M1, None) == -1
    assert lib.bya_layernorm_mx(p, p, p, None, None, None, None, None, None, 4, 1, 3072, 3072, 1536, 0, 0, 0, 0,
                                1e-5, E2M1, None) == -1                  # activations are never e2m1
    assert lib.bya_gemm_mx(p, p, p, p, None, p, None, None, None, ctypes.byref(d), E2M1, None) == -1

    # plan queries (host side; the pointers are never read): the path follows the activation format
    base = 1 << 40
    pl = _hip.GemmPlan(-9, -9, -9, -9, -9)

    def plan(a_fmt, w_fmt, M, N, K=256):
        d.M, d.N, d.K, d.batch, d.ldc = M, N, K, 1, N
        d.lda, d.ldw = K * (8 if a_fmt == E4M3 else 6) // 8, K * {E4M3: 8, E2M3: 6, E2M1: 4}[w_fmt] // 8
        rc = lib.bya_gemm_mx_mixed_plan(base, base, base, base, None, base, None, None, None, ctypes.byref(d), a_fmt, w_fmt,
                                        ctypes.byref(pl))
        return rc, pl.path

    assert plan(E2M1, E2M1, 200, 144) [0] < 0 and pl.path == -9          # untouched on rejection
    assert plan(E2M3, E2M1, 3500, 3700) == (0, T256X256)
    assert plan(E2M3, E2M1, 200, 144) == (0, T128X128)
    assert plan(E4M3, E2M1, 3500, 3700) == (0, T128X128)
    assert plan(E2M3, E2M3, 3500, 3700) == (0, T256X256) and plan(E4M3, E4M3, 3500, 3700) == (0, T128X128)
    assert (pl.m0, pl.tail, pl.split_k, pl.row_chunks) == (0, -1, 0, 1)
    assert lib.bya_gemm_mx_mixed_plan(base, base, base, base, None, base, None, None, None, ctypes.byref(d), E2M3, E2M1,
                                      None) == -1


def test_python_surface_of_the_weight_format():
    from bind_your_avatar_implementation_amd import ops
    assert ops.MX_FORMATS == {"mxfp8": 0, "mxfp6": 2}                     # the activation vocabulary is unchanged
    assert ops.MX_WEIGHT_FORMATS == {"mxfp8": 0, "mxfp6": 2, "mxfp4": 4}
    assert ops.mx_code_bytes(3072, "mxfp4") == 1536 and ops.mx_code_bytes(3072, "mxfp6") == 2304
    with pytest.raises(ValueError):
        ops.mx_fmt_code("mxfp4")
    meta = lambda *s: torch.empty(*s, dtype=torch.uint8, device="meta")
    out = torch.empty(3500, 3700, dtype=torch.bfloat16, device="meta")
    for fmt, expect in (("mxfp6", "t256x256"), ("mxfp8", "t128x128")):
        args = (meta(3500, ops.mx_code_bytes(256, fmt)), meta(3500, 8), meta(3700, 128), meta(3700, 8), out, fmt)
        assert ops.gemm_mx_plan(*args, w_fmt="mxfp4")["path"] == expect
    with pytest.raises(ValueError):
        ops.gemm_mx_plan(meta(3500, 256), meta(3500, 8), meta(3700, 192), meta(3700, 8), out, "mxfp8", w_fmt="mxfp6")
    with pytest.raises(ValueError):
        ops.gemm_mx_plan(meta(3500, 128), meta(3500, 8), meta(3700, 128), meta(3700, 8), out, "mxfp4", w_fmt="mxfp4")


def test_enable_mx_weights_validates_the_weight_format_before_touching_the_engine():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    enable = BindyouravatarTransformer3DModel.enable_mx_weights
    calls = []
    fake = types.SimpleNamespace(invalidate_engine=lambda: calls.append(1))
    with pytest.raises(ValueError):
        enable(fake, "mxfp6", weight_format="fp4")
    with pytest.raises(ValueError):
        enable(fake, "mxfp8", weight_format="mxfp6")
    with pytest.raises(ValueError):
        enable(fake, "mxfp4")
    with pytest.raises(ValueError):
        enable(fake, "mxfp4", weight_format="mxfp4")
    assert not calls and not hasattr(fake, "_mx_weights") and not hasattr(fake, "_mx_weight_format")
    assert enable(fake, "mxfp8", weight_format="mxfp4") is fake
    assert fake._mx_weights == "mxfp8" and fake._mx_weight_format == "mxfp4" and fake._mx_linears is None and calls == [1]
    enable(fake, weight_format="mxfp4", linears=("ff1",))
    assert fake._mx_weights == "mxfp6" and fake._mx_weight_format == "mxfp4" and fake._mx_linears == ("ff1",)
    enable(fake, "mxfp6", weight_format="mxfp6")
    assert fake._mx_weight_format == "mxfp6"
    enable(fake, "mxfp6")
    assert fake._mx_weights == "mxfp6" and fake._mx_weight_format is None and len(calls) == 4
    enable(fake, weight_format="mxfp4", enabled=False)
    assert fake._mx_weights is None and fake._mx_weight_format is None
