"""CPU: the OCP MX format of include/bya.h ("MX weights") restated in torch -- block scales, e2m3 / e4m3 element codes, the
e2m3 bit packing -- plus the argument checks of the MX entry points and of enable_mx_weights (nothing is launched).  The
restatement here is what tests/test_mx_gpu.py compares the kernels with, byte for byte."""
import ctypes
import types

import numpy as np
import pytest
import torch

from mx_ref import (BITS, EMAX, FMT_CODE, dequant_mx, e2m3_decode, e2m3_encode, e2m3_encode_nearest, e2m3_values,  # noqa: F401
                    pack6, quant_mx_ref, unpack6)

def test_e2m3_codes_are_fixed_points_and_ties_go_to_even():
    codes = torch.arange(64)
    assert torch.equal(e2m3_encode_nearest(e2m3_decode(codes)), codes)
    assert torch.equal(e2m3_encode(e2m3_decode(codes)), codes)
    # midpoints: 0.0625 (0 | 0.125) -> 0, 0.1875 -> 0.25, 1.0625 -> 1.0, 2.125 -> 2.0, 3.875 -> 4.0, 7.25 -> 7.0, above -> 7.5
    v = torch.tensor([0.0625, 0.1875, 1.0625, 2.125, 3.875, 7.25, 7.75, 100.0, -0.01], dtype=torch.float64)
    assert e2m3_decode(e2m3_encode_nearest(v)).tolist() == [0.0, 0.25, 1.0, 2.0, 4.0, 7.0, 7.5, 7.5, -0.0]


def test_binade_rint_form_of_e2m3_rounding_equals_the_nearest_code_definition():
    """The arithmetic csrc/mx_common.h's f32_to_e2m3 uses (rint of the value counted in steps of its binade), written out in
    numpy -- a check of the formula, not of the kernel, which tests/test_mx_gpu.py compares byte for byte --, against the
    nearest-code definition above on every fp32 product a block can produce (|v| < 8 plus saturating values); the torch
    form the GPU tests use (e2m3_encode) as well."""
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.rand(400_000, generator=g) * 16 - 8, torch.randn(100_000, generator=g) * 0.2,
                   e2m3_values().float() + 0.0625, e2m3_values().float() * 0.5, torch.tensor([0.0, -0.0])]).float()
    a = np.minimum(np.abs(v.numpy()), np.float32(7.5))
    c = np.where(a < 2, np.rint(a * 8), np.where(a < 4, np.rint(a * 4) + 8, np.rint(a * 2) + 16)).astype(np.int64)
    c |= (v.numpy().view(np.uint32) >> 26).astype(np.int64) & 32
    nearest = e2m3_encode_nearest(v.double())
    assert np.array_equal(c, nearest.numpy())
    assert torch.equal(e2m3_encode(v.double()), nearest)


@pytest.mark.parametrize("fmt", ["mxfp6", "mxfp8"])
def test_restatement_scales_zero_blocks_and_round_trip(fmt):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(3, 256, generator=g) * 5).to(torch.bfloat16)
    x[0, :32] = 0                                     # all-zero block: byte 127, zero codes
    x[0, 32:64] = -0.0                                # (-0 too)
    x[1, 64:96] = torch.tensor([2.0 ** -130] * 32).to(torch.bfloat16)       # subnormal block maximum: E clamps at -127
    x[2, :32] = 0.5
    x[2, 3] = 3e38                                    # an outlier sets its block's scale and nothing else
    codes, scales = quant_mx_ref(x, fmt)
    assert codes.shape == (3, 256 * BITS[fmt] // 8) and scales.shape == (3, 8)
    assert scales[0, 0] == 127 and scales[0, 1] == 127 and (codes[0, :2 * 32 * BITS[fmt] // 8] == 0).all()
    assert scales[1, 2] == 0
    assert scales[2, 0] == 127 + 127 - EMAX[fmt] and scales[2, 1] != scales[2, 0]
    back = dequant_mx(codes, scales, fmt)
    # block-relative error: half an element step, or the saturation of a block maximum in (largest finite, 2^(emax+1)) * 2^E
    # (448 of up to 512 for e4m3, 7.5 of up to 8 for e2m3): at most 1/8 either way
    blk = x.double().reshape(3, 8, 32)
    err = (back.reshape(3, 8, 32) - blk).abs().amax(-1) / blk.abs().amax(-1).clamp_min(1e-300)
    assert float(err[2:, 1:].max()) <= 2.0 ** -3
    if fmt == "mxfp6":
        assert torch.equal(pack6(unpack6(codes)), codes)


def test_mx_entry_points_reject_bad_arguments_without_launching():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    lib = _hip.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    assert lib.bya_quantize_mx(None, None, None, 4, 128, 128, 2, None) == -1
    assert lib.bya_quantize_mx(p, p, p, 4, 96, 96, 2, None) == -1                  # K % 128
    assert lib.bya_quantize_mx(p, p, p, 4, 128, 128, 1, None) == -1                # no format 1 (e5m2 is not offered)
    d = _hip.GemmDesc()
    d.M, d.N, d.K, d.batch, d.lda, d.ldw, d.ldc = 16, 16, 128, 1, 96, 96, 16
    assert lib.bya_gemm_mx(None, None, None, None, None, None, None, None, None, ctypes.byref(d), 2, None) == -1
    assert lib.bya_gemm_mx(p, p, p, p, None, p, None, None, None, ctypes.byref(d), 4, None) == -1       # fp4: out of scope
    d.K = 192
    assert lib.bya_gemm_mx(p, p, p, p, None, p, None, None, None, ctypes.byref(d), 2, None) == -1
    assert lib.bya_layernorm_mx(p, p, p, None, None, None, None, None, None, 4, 1, 3072, 3072, 2304, 0, 0, 0, 0,
                                1e-5, 3, None) == -1


def test_enable_mx_weights_validates_before_touching_the_engine():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    calls = []
    fake = types.SimpleNamespace(invalidate_engine=lambda: calls.append(1))
    for bad in ("mxfp4", "fp6", "e2m3", None):
        with pytest.raises(ValueError):
            BindyouravatarTransformer3DModel.enable_mx_weights(fake, bad)
    assert not calls and not hasattr(fake, "_mx_weights")
    assert BindyouravatarTransformer3DModel.enable_mx_weights(fake, "mxfp8", linears="all") is fake
    assert fake._mx_weights == "mxfp8" and fake._mx_linears == "all" and calls == [1]
    BindyouravatarTransformer3DModel.enable_mx_weights(fake, linears=("ff1", "aq"))
    assert fake._mx_weights == "mxfp6" and fake._mx_linears == ("ff1", "aq")
    BindyouravatarTransformer3DModel.enable_mx_weights(fake, enabled=False)
    assert fake._mx_weights is None
