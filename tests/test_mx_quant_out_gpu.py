"""The MX GEMM whose epilogue writes MX codes (include/bya.h, bya_gemm_mx_quant; ops.gemm_mx_quant): byte for byte
bya_gemm_mx(_mixed) followed by bya_quantize_mx -- on random data over every operand / output format pair and both tiles, on
exact data built to hit the edge blocks of the format (against the torch restatement of tests/test_mx_cpu.py too), with
canaries around and inside the output buffers, with batched operands, as the operand of the next GEMM, and in the engine
(enable_mx_weights(fuse_activation_quant=...)).  No tolerance anywhere: every comparison is torch.equal.

Measured on the first run: see DESIGN.md section 11."""
import ctypes

import pytest
import torch

from test_mx_cpu import BITS, EMAX, dequant_mx, e2m3_decode, e2m3_encode, pack6, quant_mx_ref, unpack6

pytestmark = pytest.mark.gpu

FORMATS = ("mxfp8", "mxfp6")
CODE = {"mxfp8": 0, "mxfp6": 2, "mxfp4": 4}
ALL_BITS = {**BITS, "mxfp4": 4}


def rnd(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16)


_OPERANDS = {}


def operands(dev, M, N, K, fmt, w_fmt):
    """Random MX operands of one shape and format pair, built once: (a codes, a scales, w codes, w scales, bias)."""
    from bind_your_avatar_implementation_amd import ops
    key = (M, N, K, fmt, w_fmt)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(M + N)
        a = torch.randn(M, K, generator=g) * 2.0
        a[:, torch.randperm(K, generator=g)[:max(1, K // 64)]] *= 100.0                  # outlier channels
        a = a.to(torch.bfloat16)
        a[min(5, M - 1)] = 0                                                              # a zero row: zero blocks where no bias
        w = rnd((N, K), N + 1, std=K ** -0.5)
        w[:, 7] *= 50.0                                                                  # output blocks of very different size
        bias = rnd((N,), 4, std=3.0).to(dev)
        _OPERANDS[key] = (*ops.quantize_mx(a.to(dev), fmt), *ops.quantize_mx(w.to(dev), w_fmt), bias)
    return _OPERANDS[key]


def two_launches(ac, asc, wc, wsc, fmt, w_fmt, out_fmt, bias, act):
    from bind_your_avatar_implementation_amd import ops
    M, N = asc.shape[-2], wc.shape[0]
    out = torch.empty(*asc.shape[:-1], N, dtype=torch.bfloat16, device=ac.device)
    ops.gemm_mx(ac, asc, wc, wsc, out, fmt, bias=bias, act=act, w_fmt=w_fmt)
    return (*ops.quantize_mx(out, out_fmt), out)


def fused(ac, asc, wc, wsc, fmt, w_fmt, out_fmt, bias, act, expect_path=None):
    from bind_your_avatar_implementation_amd import ops
    N = wc.shape[0]
    lead = tuple(asc.shape[:-1])
    oc = torch.full((*lead, ops.mx_code_bytes(N, out_fmt)), 0xA5, dtype=torch.uint8, device=ac.device)
    osc = torch.full((*lead, N // 32), 0xA5, dtype=torch.uint8, device=ac.device)
    if expect_path is not None:
        plan = ops.gemm_mx_quant_plan(ac, asc, wc, wsc, oc, osc, fmt, w_fmt=w_fmt, out_fmt=out_fmt, bias=bias, act=act)
        assert plan["path"] == expect_path, plan
    got = ops.gemm_mx_quant(ac, asc, wc, wsc, oc, osc, fmt, w_fmt=w_fmt, out_fmt=out_fmt, bias=bias, act=act)
    assert got[0] is oc and got[1] is osc
    return oc, osc


# 300 x 256: a partial row tile of the 128 x 128 path; 17 x 128: fewer rows than one fragment; 3500 x 3712: 14 x 15 = 210 tiles
# of 256 x 256 (>= 200: e2m3 activations run on 256 x 256 tiles), a partial row tile and 14.5 column tiles
SHAPES = [(300, 256, 256), (17, 128, 128), (3500, 3712, 256)]


@pytest.mark.parametrize("out_fmt", FORMATS)
@pytest.mark.parametrize("w_kind", ["same", "mxfp4"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fused_launch_equals_gemm_then_quantiser_byte_for_byte(dev, M, N, K, fmt, w_kind, out_fmt):
    w_fmt = fmt if w_kind == "same" else "mxfp4"
    ac, asc, wc, wsc, bias = operands(dev, M, N, K, fmt, w_fmt)
    big = fmt == "mxfp6" and -(-M // 256) * -(-N // 256) >= 200
    path = "t256x256" if big else "t128x128"
    assert big == ((M, N, K) == SHAPES[2] and fmt == "mxfp6")
    for act in (None, "gelu_tanh"):
        for b in (None, bias):
            c_ref, s_ref, _ = two_launches(ac, asc, wc, wsc, fmt, w_fmt, out_fmt, b, act)
            oc, osc = fused(ac, asc, wc, wsc, fmt, w_fmt, out_fmt, b, act, expect_path=path)
            bad_s, bad_c = int((osc != s_ref).sum()), int((oc != c_ref).sum())
            print(f"{fmt}*{w_fmt}>{out_fmt} {M}x{N}x{K} act={act} bias={b is not None} {path}: "
                  f"{bad_s} of {s_ref.numel()} scale bytes, {bad_c} of {c_ref.numel()} code bytes differ")
            assert torch.equal(osc, s_ref)
            assert torch.equal(oc, c_ref)


# ------------------------------------------------------------------------------------------ edge blocks on exact data
def e2m3_grid():
    c = torch.arange(32)
    return e2m3_decode(c)                                                                 # the 32 magnitudes, float64


def exact_case(fmt):
    """A [40, 256] whose dequantised values are the wanted outputs, for W = the identity: the GEMM's fp32 sums are A's values
    exactly, and a bias of a few columns adds what a block of A cannot hold.  Blocks of 32 columns:
      0, 7  random elements and scales          1  zeros                        2  480 (e4m3 saturates) / 7.5 (+ 0.25: e2m3 does)
      3     one outlier column, zeros around    4  amax 4 next to -2^-5, -2^-17  5  amax exactly 8      6  amax exactly 2^-3
    Rows 0 and 1 of A are all zero.  Elements are e2m3 magnitudes (a subset of e4m3's), so both formats hold A exactly.
    -> (A codes, A scales, the values [40, 256] float64, bias [256] float64)"""
    M, K = 40, 256
    g = torch.Generator().manual_seed(11)
    grid = e2m3_grid()
    el = grid[torch.randint(0, 32, (M, K), generator=g)] * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1).double()
    sc = torch.randint(-3, 4, (M, K // 32), generator=g)
    el[:, 32:64] = 0
    el[:, 64:96] = grid[torch.randint(0, 16, (M, 32), generator=g)]                       # < 2: small next to the maximum
    el[0::2, 64 + 3], sc[0::2, 2] = 7.5, 6                                               # 480
    el[1::2, 64 + 9], sc[1::2, 2] = 7.5, 0                                               # 7.5 (+ 0.25 of bias = 7.75)
    el[:, 96:128], sc[:, 3] = 0, 10
    el[:, 96 + 5] = -7.5                                                                  # the outlier column: -7680
    el[:, 128:160], sc[:, 4] = 0, 0
    el[:, 128 + 1], el[:, 128 + 30] = 4.0, -3.0
    el[:, 160:192] = grid[torch.randint(0, 24, (M, 32), generator=g)]                     # < 4
    el[:, 160 + 31], sc[:, 5] = 4.0, 1                                                    # 8.0
    el[:, 192:224] = grid[torch.randint(0, 8, (M, 32), generator=g)]                      # < 1
    el[:, 192 + 16], sc[:, 6] = -1.0, -3                                                  # -2^-3
    el[:2] = 0
    el = torch.where(el == 0, torch.zeros_like(el), el)                                   # no -0 operands
    scales = (127 + sc).to(torch.uint8)
    target = torch.ldexp(el.reshape(M, -1, 32), sc[..., None].double()).reshape(M, K)
    codes = el.float().to(torch.float8_e4m3fn).view(torch.uint8) if fmt == "mxfp8" else pack6(e2m3_encode(el))
    assert torch.equal(dequant_mx(codes, scales, fmt), target)
    bias = torch.zeros(K, dtype=torch.float64)
    bias[64 + 9] = 0.25
    bias[128 + 7], bias[128 + 20] = -2.0 ** -5, -2.0 ** -17
    bias[5], bias[230] = 1.5, -0.375                                                      # (and two ordinary columns)
    return codes, scales, target, bias


def check_edge_blocks(sb, cb, out_fmt, with_bias):
    """What the blocks of exact_case were built for, spelled out on the scale bytes ``sb`` and code bytes ``cb`` (CPU)."""
    sb = sb.long()
    el = cb.long() if out_fmt == "mxfp8" else unpack6(cb)                                 # one code per element
    sign, top = (0x80, 0x7e) if out_fmt == "mxfp8" else (0x20, 0x1f)                      # sign bit; largest finite magnitude
    emax = EMAX[out_fmt]
    assert (sb[:, 1] == 127).all() and (el[:, 32:64] == 0).all()                          # zero block: byte 127, zero codes
    if not with_bias:
        assert (sb[:2] == 127).all() and (cb[:2] == 0).all()                              # all-zero A rows
    if out_fmt == "mxfp8":
        assert (sb[2::2, 2] == 127 + 8 - emax).all() and (el[2::2, 64 + 3] == top).all()  # 480 -> 448
    elif with_bias:
        assert (sb[3::2, 2] == 127 + 2 - emax).all() and (el[3::2, 64 + 9] == top).all()  # 7.75 -> 7.5
    # the outlier -7680: its block's scale, and itself saturated (e4m3: -480 -> -448) or on the largest code (e2m3: -7.5)
    assert (sb[2:, 3] == 127 + 12 - emax).all() and (el[2:, 96 + 5] == (sign | top)).all()
    assert (sb[2:, 5] == 127 + 3 - emax).all() and (sb[2:, 6] == 127 - 3 - emax).all()    # amax on a power of two
    assert (sb[2:, 4] == 127 + 2 - emax).all()
    if with_bias:
        assert (el[2:, 128 + 20] == sign).all()                                           # -2^-17 next to 4: -0, sign kept
        if out_fmt == "mxfp6":
            assert (el[2:, 128 + 7] == sign).all()                                        # -2^-5: a quarter step of e2m3, -0


@pytest.mark.parametrize("out_fmt", FORMATS)
@pytest.mark.parametrize("fmt,w_fmt", [("mxfp8", "mxfp8"), ("mxfp6", "mxfp6"), ("mxfp6", "mxfp4"), ("mxfp8", "mxfp4")])
def test_edge_blocks_on_exact_outputs(dev, fmt, w_fmt, out_fmt):
    from bind_your_avatar_implementation_amd import ops
    codes, scales, target, bias = exact_case(fmt)
    d = lambda t: t.to(dev)
    M, N = target.shape
    wc, wsc = ops.quantize_mx(torch.eye(N).to(torch.bfloat16).to(dev), w_fmt)             # 1.0 is a code of every format
    assert (target.to(torch.bfloat16).double() == target).all()                          # every value of A is an exact bf16
    bias16 = bias.to(torch.bfloat16)
    assert (bias16.double() == bias).all()
    for with_bias in (False, True):
        # acc is exact; acc + bias is one fp32 rounding of the exact sum, then the one rounding to bf16
        want = (target + bias).float().to(torch.bfloat16) if with_bias else target.to(torch.bfloat16)
        b = d(bias16) if with_bias else None
        c_two, s_two, out = two_launches(d(codes), d(scales), wc, wsc, fmt, w_fmt, out_fmt, b, None)
        oc, osc = fused(d(codes), d(scales), wc, wsc, fmt, w_fmt, out_fmt, b, None, expect_path="t128x128")
        assert torch.equal(out.cpu(), want)                                               # the GEMM output is what was built
        c_def, s_def = quant_mx_ref(want, out_fmt)                                        # the torch restatement of the format
        check_edge_blocks(s_def, c_def, out_fmt, with_bias)                               # (the case hits what it was built for)
        assert torch.equal(osc, s_two) and torch.equal(oc, c_two)
        assert torch.equal(osc.cpu(), s_def) and torch.equal(oc.cpu(), c_def)
        check_edge_blocks(osc.cpu(), oc.cpu(), out_fmt, with_bias)
    # the outlier column moves its own block's scale and nothing else
    quiet = codes.clone()
    if fmt == "mxfp8":
        quiet[:, 96 + 5] = 0
    else:
        e = unpack6(quiet)
        e[:, 96 + 5] = 0
        quiet = pack6(e)
    qc, qsc = fused(d(quiet), d(scales), wc, wsc, fmt, w_fmt, out_fmt, d(bias16), None)
    rb = 32 * BITS[out_fmt] // 8
    keep = [c for c in range(oc.shape[1]) if not 3 * rb <= c < 4 * rb]
    others = [0, 1, 2, 4, 5, 6, 7]
    assert torch.equal(qc[:, keep], oc[:, keep]) and torch.equal(qsc[:, others], osc[:, others])
    assert (qsc[:, 3] == 127).all() and (osc[2:, 3] != 127).all()                         # (rows 0, 1 of A are zero)


# ------------------------------------------------------------------------------------------ raw descriptor: strides, canaries
def raw_quant(a, asc, w, wsc, bias, codes_ptr, scales_ptr, M, N, K, fmt, w_fmt, out_fmt, ldc, batch=1, a_bs=0, c_bs=0,
              act=None):
    from bind_your_avatar_implementation_amd import _hip, ops
    d = ops.GemmDesc()
    d.M, d.N, d.K, d.batch = M, N, K, batch
    d.lda, d.ldw, d.ldc = K * ALL_BITS[fmt] // 8, K * ALL_BITS[w_fmt] // 8, ldc
    d.a_batch_stride, d.c_batch_stride = a_bs, c_bs
    d.act, d.alpha = ops.ACT[act], 1.0
    rc = _hip.load().bya_gemm_mx_quant(a.data_ptr(), asc.data_ptr(), w.data_ptr(), wsc.data_ptr(),
                                       None if bias is None else bias.data_ptr(), codes_ptr, scales_ptr, ctypes.byref(d),
                                       CODE[fmt], CODE[w_fmt], CODE[out_fmt], ops._stream())
    assert rc == 0, rc


@pytest.mark.parametrize("out_fmt", FORMATS)
@pytest.mark.parametrize("fmt,M,N,K", [("mxfp8", 300, 256, 256), ("mxfp6", 300, 256, 256), ("mxfp6", 3500, 3712, 256)])
def test_no_stray_writes_around_or_between_the_rows(dev, fmt, M, N, K, out_fmt):
    """Canary bytes before and after both output buffers and in the padding of a row stride larger than the row, on shapes
    with a partial row tile (and, at 3712 columns, half a column tile of the 256 x 256 path)."""
    ac, asc, wc, wsc, bias = operands(dev, M, N, K, fmt, fmt)
    c_ref, s_ref, _ = two_launches(ac, asc, wc, wsc, fmt, fmt, out_fmt, bias, "gelu_tanh")
    rb, pad, guard = N * BITS[out_fmt] // 8, 48, 4096
    ldc = rb + pad
    cbuf = torch.full((guard + M * ldc + guard,), 0xC3, dtype=torch.uint8, device=dev)
    sbuf = torch.full((guard + M * (N // 32) + guard,), 0xC3, dtype=torch.uint8, device=dev)
    assert (cbuf.data_ptr() + guard) % 16 == 0 and (sbuf.data_ptr() + guard) % 4 == 0
    raw_quant(ac, asc, wc, wsc, bias, cbuf.data_ptr() + guard, sbuf.data_ptr() + guard, M, N, K, fmt, fmt, out_fmt, ldc,
              act="gelu_tanh")
    rows = cbuf[guard:guard + M * ldc].view(M, ldc)
    assert torch.equal(rows[:, :rb], c_ref)
    assert (rows[:, rb:] == 0xC3).all()                                                   # the padding of every row
    assert (cbuf[:guard] == 0xC3).all() and (cbuf[guard + M * ldc:] == 0xC3).all()
    assert torch.equal(sbuf[guard:guard + M * (N // 32)].view(M, N // 32), s_ref)
    assert (sbuf[:guard] == 0xC3).all() and (sbuf[guard + M * (N // 32):] == 0xC3).all()


@pytest.mark.parametrize("fmt,w_fmt,out_fmt", [("mxfp6", "mxfp6", "mxfp8"), ("mxfp8", "mxfp4", "mxfp6")])
def test_batched_operands(dev, fmt, w_fmt, out_fmt):
    """batch = 2 as grid.z with batch strides larger than the matrices: A codes advance by a_batch_stride, the codes by
    c_batch_stride, and the scale rows of entry z are z * M + m (dense)."""
    from bind_your_avatar_implementation_amd import ops
    M, N, K = 300, 256, 256
    ac0, asc0, wc, wsc, bias = operands(dev, M, N, K, fmt, w_fmt)
    a1 = (rnd((M, K), 77, std=3.0)).to(dev)
    ac1, asc1 = ops.quantize_mx(a1, fmt)
    lda, rb = ac0.shape[1], N * BITS[out_fmt] // 8
    a_bs, c_bs = M * lda + 160, M * rb + 320
    abuf = torch.zeros(2 * a_bs, dtype=torch.uint8, device=dev)
    abuf[:M * lda] = ac0.reshape(-1)
    abuf[a_bs:a_bs + M * lda] = ac1.reshape(-1)
    sa = torch.cat([asc0, asc1]).contiguous()
    cbuf = torch.full((2 * c_bs,), 0xC3, dtype=torch.uint8, device=dev)
    sbuf = torch.full((2 * M, N // 32), 0xC3, dtype=torch.uint8, device=dev)
    raw_quant(abuf, sa, wc, wsc, bias, cbuf.data_ptr(), sbuf.data_ptr(), M, N, K, fmt, w_fmt, out_fmt, rb, batch=2, a_bs=a_bs,
              c_bs=c_bs)
    for z, (a_c, a_s) in enumerate(((ac0, asc0), (ac1, asc1))):
        c_ref, s_ref, _ = two_launches(a_c, a_s, wc, wsc, fmt, w_fmt, out_fmt, bias, None)
        assert torch.equal(cbuf[z * c_bs:z * c_bs + M * rb].view(M, rb), c_ref)
        assert torch.equal(sbuf[z * M:(z + 1) * M], s_ref)
        assert (cbuf[z * c_bs + M * rb:(z + 1) * c_bs] == 0xC3).all()
    # and the front end's own batch form (evenly stacked entries)
    oc, osc = fused(torch.stack([ac0, ac1]), torch.stack([asc0, asc1]), wc, wsc, fmt, w_fmt, out_fmt, bias, None)
    assert torch.equal(oc[1], cbuf[c_bs:c_bs + M * rb].view(M, rb)) and torch.equal(osc.view(2 * M, -1), sbuf)


@pytest.mark.parametrize("fmt,w_fmt", [("mxfp6", "mxfp6"), ("mxfp8", "mxfp4")])
def test_fused_pair_is_a_legal_operand_of_the_next_gemm(dev, fmt, w_fmt):
    from bind_your_avatar_implementation_amd import ops
    M, N, K = 300, 256, 256
    ac, asc, wc, wsc, bias = operands(dev, M, N, K, fmt, w_fmt)
    c_ref, s_ref, _ = two_launches(ac, asc, wc, wsc, fmt, w_fmt, fmt, bias, "gelu_tanh")
    oc, osc = fused(ac, asc, wc, wsc, fmt, w_fmt, fmt, bias, "gelu_tanh")
    w2c, w2s = ops.quantize_mx(rnd((384, N), 21, std=N ** -0.5).to(dev), w_fmt)
    res = rnd((M, 384), 22).to(dev)
    y_ref, y = torch.empty(M, 384, dtype=torch.bfloat16, device=dev), torch.empty(M, 384, dtype=torch.bfloat16, device=dev)
    ops.gemm_mx(c_ref, s_ref, w2c, w2s, y_ref, fmt, res=res, w_fmt=w_fmt)
    ops.gemm_mx(oc, osc, w2c, w2s, y, fmt, res=res, w_fmt=w_fmt)
    assert torch.equal(y, y_ref) and bool(y.float().abs().sum() > 0)


# ------------------------------------------------------------------------------------------ engine
class Counter:
    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *a, **kw):
        self.n += 1
        return self.fn(*a, **kw)


def counted_forward(model, gi, monkeypatch):
    from bind_your_avatar_implementation_amd import ops
    model(**gi)                                                                           # builds the engine (packs weights)
    with monkeypatch.context() as mp:
        q, f = Counter(ops.quantize_mx), Counter(ops.gemm_mx_quant)
        mp.setattr(ops, "quantize_mx", q)
        mp.setattr(ops, "gemm_mx_quant", f)
        out = model(**gi)[0].clone()
    return out, q.n, f.n


@pytest.mark.parametrize("fmt,weight_format", [("mxfp6", None), ("mxfp8", "mxfp4")])
def test_engine_ff1_feeds_ff2_directly(dev, monkeypatch, fmt, weight_format):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    model.enable_mx_weights(fmt, weight_format=weight_format, fuse_activation_quant=False)
    off, q_off, f_off = counted_forward(model, gi, monkeypatch)
    assert not model._engine.mx_fuse_quant and f_off == 0
    model.enable_mx_weights(fmt, weight_format=weight_format, fuse_activation_quant=True)
    assert model._engine is None                                                          # the switch invalidates the engine
    on, q_on, f_on = counted_forward(model, gi, monkeypatch)
    assert model._engine.mx_fuse_quant
    print(f"{fmt}/{weight_format}: quantize_mx calls {q_off} -> {q_on}, gemm_mx_quant calls {f_off} -> {f_on}, {blocks} blocks")
    assert torch.equal(on, off)
    assert q_off - q_on == blocks and f_on == blocks
    model.enable_mx_weights(fmt, weight_format=weight_format)                             # the default is on
    assert counted_forward(model, gi, monkeypatch)[2] == blocks
    # graph replay of the fused step: bit for bit the eager result
    model.use_hip_graph = True
    try:
        model(**gi)                                                                       # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], on)
    finally:
        model.use_hip_graph = False
        model._graphs = {}
    # ff.net.2 in bf16: nothing to feed, the two launches stay and the output does not depend on the switch
    sel = ("qkv", "out", "ff1")
    model.enable_mx_weights(fmt, weight_format=weight_format, linears=sel, fuse_activation_quant=False)
    ref, _, f0 = counted_forward(model, gi, monkeypatch)
    model.enable_mx_weights(fmt, weight_format=weight_format, linears=sel, fuse_activation_quant=True)
    got, _, f1 = counted_forward(model, gi, monkeypatch)
    assert set(model._engine.wmx) == set(sel) and f0 == 0 and f1 == 0
    assert torch.equal(got, ref)
