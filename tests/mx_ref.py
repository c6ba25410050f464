"""The OCP MX formats of include/bya.h ("MX weights") restated in torch (a plain helper module: no tests, no fixtures): block
scales, the e2m3 / e4m3 / e2m1 element codes, the 6-bit and 4-bit packings, the quantiser and the dequantiser, and the random
and hard bf16 inputs the MX tests share.  tests/test_mx_cpu.py and tests/test_mxfp4_cpu.py test these restatements; the GPU
tests compare the kernels with them byte for byte."""
import torch

FMT_CODE = {"mxfp8": 0, "mxfp6": 2}
EMAX = {"mxfp8": 8, "mxfp6": 2}
BITS = {"mxfp8": 8, "mxfp6": 6}


def e2m3_values():
    """Magnitudes of the 32 non-negative e2m3 codes (code = exponent << 3 | mantissa, exponent bias 1, no inf / NaN)."""
    c = torch.arange(32)
    e, m = c >> 3, (c & 7).double()
    return torch.where(e == 0, m / 8, (1 + m / 8) * torch.pow(2.0, (e - 1).double()))


def e2m3_encode_nearest(v):
    """The definition: RNE of float64 values to e2m3 codes, saturating at 7.5 -- the nearest of the 32 magnitudes, ties to
    the even code."""
    vals = e2m3_values()
    a = v.abs().clamp(max=7.5)
    d = (a[..., None] - vals).abs()
    best = d.min(dim=-1, keepdim=True).values
    cand = (d == best) & ((torch.arange(32) & 1) == 0)          # a tie sits between an odd and an even code
    code = torch.where(cand.any(-1), cand.int().argmax(-1), (d == best).int().argmax(-1))
    return code | (torch.signbit(v).long() << 5)


def e2m3_encode(v):
    """The same codes by counting steps of the value's binade (1/8 below 2, 1/4 in [2, 4), 1/2 from 4) and rounding the
    count half-to-even (torch.round): the form that scales to whole activation matrices."""
    a = v.abs().clamp(max=7.5)
    c = torch.where(a < 2, torch.round(a * 8), torch.where(a < 4, torch.round(a * 4) + 8, torch.round(a * 2) + 16))
    return c.long() | (torch.signbit(v).long() << 5)


def e2m3_decode(c):
    c = c.long()
    mag = e2m3_values().to(c.device)[c & 31]
    return torch.where((c & 32) != 0, -mag, mag)


def pack6(codes):
    """[.., K] e2m3 codes -> [.., K * 3 / 4] bytes: element i of a 32-block at bits 6i .. 6i+5, LSB first."""
    c = codes.long().reshape(*codes.shape[:-1], -1, 4)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)        # 24 bits = 3 bytes per 4 elements
    return torch.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], -1).reshape(*codes.shape[:-1], -1).to(torch.uint8)


def unpack6(b):
    t = b.long().reshape(*b.shape[:-1], -1, 3)
    w = t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)
    return torch.stack([(w >> (6 * i)) & 63 for i in range(4)], -1).reshape(*b.shape[:-1], -1)


def quant_mx_ref(x, fmt):
    """include/bya.h, bya_quantize_mx, on the CPU: x bf16 [.., K] -> (codes uint8 [.., K * bits / 8], scales uint8 [.., K / 32])."""
    xf = x.float().double()
    blk = xf.reshape(*xf.shape[:-1], -1, 32)
    amax = blk.abs().amax(-1, keepdim=True)
    _, ex = torch.frexp(amax)                                        # amax = mant * 2^ex, mant in [0.5, 1)
    E = (ex.long() - 1 - EMAX[fmt]).clamp(-127, 127)
    zero = amax == 0
    E = torch.where(zero, torch.zeros_like(E), E)
    v = torch.ldexp(blk, -E.double())                                # exact: a power-of-two product
    if fmt == "mxfp8":
        q = v.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn).view(torch.uint8).long()
    else:
        q = e2m3_encode(v)
    q = torch.where(zero, torch.zeros_like(q), q).reshape(*x.shape)
    codes = q.to(torch.uint8) if fmt == "mxfp8" else pack6(q)
    return codes, (E + 127).squeeze(-1).to(torch.uint8)


def dequant_mx(codes, scales, fmt):
    """MX bytes -> float64 [.., K]."""
    if fmt == "mxfp8":
        el = codes.view(torch.float8_e4m3fn).double()
    else:
        el = e2m3_decode(unpack6(codes))
    el = el.reshape(*scales.shape, 32)
    return torch.ldexp(el, (scales.long() - 127)[..., None].double()).reshape(*scales.shape[:-1], -1)


def e2m1_values():
    """Magnitudes of the 8 non-negative e2m1 codes (code = exponent << 1 | mantissa, exponent bias 1, no inf / NaN)."""
    return torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def e2m1_encode_nearest(v):
    """The definition: RNE of float64 values to e2m1 codes, saturating at 6 -- the nearest of the 8 magnitudes, ties to the
    even code."""
    vals = e2m1_values()
    a = v.abs().clamp(max=6.0)
    d = (a[..., None] - vals).abs()
    best = d.min(dim=-1, keepdim=True).values
    cand = (d == best) & ((torch.arange(8) & 1) == 0)           # a tie sits between an odd and an even code
    code = torch.where(cand.any(-1), cand.int().argmax(-1), (d == best).int().argmax(-1))
    return code | (torch.signbit(v).long() << 3)


def e2m1_encode(v):
    """The same codes by counting steps of the value's binade (1/2 below 2, 1 in [2, 4), 2 from 4) and rounding the count
    half-to-even: the form csrc/mx_common.h's f32_to_e2m1 uses."""
    a = v.abs().clamp(max=6.0)
    c = torch.where(a < 2, torch.round(a * 2), torch.where(a < 4, torch.round(a) + 2, torch.round(a / 2) + 4))
    return c.long() | (torch.signbit(v).long() << 3)


def e2m1_decode(c):
    c = c.long()
    mag = e2m1_values().to(c.device)[c & 7]
    return torch.where((c & 8) != 0, -mag, mag)


def pack4(codes):
    """[.., K] e2m1 codes -> [.., K / 2] bytes: element i in bits 4 (i % 2) .. +3 of byte i / 2, low nibble first."""
    c = codes.long().reshape(*codes.shape[:-1], -1, 2)
    return (c[..., 0] | (c[..., 1] << 4)).to(torch.uint8)


def unpack4(b):
    b = b.long()
    return torch.stack([b & 15, b >> 4], -1).reshape(*b.shape[:-1], -1)


def quant_ref(x, fmt):
    """include/bya.h, bya_quantize_mx, on the CPU for "mxfp4" (codes uint8 [.., K / 2], scales uint8 [.., K / 32]); the other
    two formats go to tests/test_mx_cpu.py."""
    if fmt != "mxfp4":
        return quant_mx_ref(x, fmt)
    xf = x.float().double()
    blk = xf.reshape(*xf.shape[:-1], -1, 32)
    amax = blk.abs().amax(-1, keepdim=True)
    _, ex = torch.frexp(amax)                                        # amax = mant * 2^ex, mant in [0.5, 1)
    E = (ex.long() - 1 - 2).clamp(-127, 127)                         # emax_elem = 2
    zero = amax == 0
    E = torch.where(zero, torch.zeros_like(E), E)
    q = e2m1_encode(torch.ldexp(blk, -E.double()))                   # exact: a power-of-two product
    q = torch.where(zero, torch.zeros_like(q), q).reshape(*x.shape)
    return pack4(q), (E + 127).squeeze(-1).to(torch.uint8)


def dequant(codes, scales, fmt):
    """MX bytes -> float64 [.., K]."""
    if fmt != "mxfp4":
        return dequant_mx(codes, scales, fmt)
    el = e2m1_decode(unpack4(codes)).reshape(*scales.shape, 32)
    return torch.ldexp(el, (scales.long() - 127)[..., None].double()).reshape(*scales.shape[:-1], -1)


def rnd(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16)


def hard_inputs(M, K, seed):
    """Gaussian rows with per-channel outliers, all-zero and -0 blocks, saturating blocks and tiny (subnormal-range) blocks."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 2.0
    x[:, torch.randperm(K, generator=g)[:max(1, K // 64)]] *= 300.0                   # outlier channels
    x = x.to(torch.bfloat16)
    x[0, :64] = 0
    x[1 % M, 32:64] = -0.0
    if M > 2:
        # a block whose maximum is just below the next power of two: x * 2^-E rounds past the largest finite value
        x[2, :32] = torch.tensor([7.9, -7.95, 3.0] + [0.01] * 29).to(torch.bfloat16)
        x[2, 32:64] = torch.tensor([511.0, -500.0, 470.0] + [1.0] * 29).to(torch.bfloat16)
    if M > 3:
        x[3, :32] = (torch.randn(32, generator=g) * 1e-39).to(torch.bfloat16)          # bf16 subnormals: E clamps at -127
        x[3, 32:64] = (torch.randn(32, generator=g) * 1e30).to(torch.bfloat16)
    return x
