"""The persistent one-wave-per-SIMD 256 x 256 MX GEMM with mxfp4 (e2m1) weights under mxfp8 activations
(csrc/gemm_mx_v4.hip, gemm256p_mx_kernel<.., MX_E2M1>; bya_gemm_mx_call, ops.gemm_mx_call(..., kernel=)): the operand and scale
map on exact data against the closed form, then bit for bit against the 128 x 128 kernel of csrc/gemm_mx.hip on the same bytes
(kernel = 0 of the same call) under the bf16, the quantising and the q/k-norm + RoPE epilogue, the fallbacks, and the engine's
step with enable_mx_weights("mxfp8", weight_format="mxfp4", persistent_gemm=...).  No tolerance anywhere: every comparison is
torch.equal on bit patterns, and the plan is asserted before every launch.  The smallest exact-data case comes first."""
import ctypes

import pytest
import torch

from exact_gemm import GuardedOut, assert_exact, exact_epilogue
from test_mx_gpu import exact_operand
from test_mx_p256_gpu import spread
from test_mx_qkn_gpu import (EPS, K_SCALE, PAD, Counter, bits, check_equal_and_canaries, nan_buffer, norm_params, operands,
                             pair_and_fused)
from test_mxfp4_cpu import dequant, e2m1_encode, pack4

pytestmark = pytest.mark.gpu
FMT, WFMT = "mxfp8", "mxfp4"


def call(kernel, want, ac, asc, wc, wsc, out, fmt=FMT, w_fmt=WFMT, **kw):
    """ops.gemm_mx_call under ``kernel`` with the plan asserted first."""
    from bind_your_avatar_implementation_amd import ops
    plan = ops.gemm_mx_call_plan(ac, asc, wc, wsc, out, kernel, fmt, w_fmt, **kw)
    assert plan is not None and plan["path"] == want, (kernel, plan)
    got = ops.gemm_mx_call(ac, asc, wc, wsc, out, kernel, fmt, w_fmt, **kw)
    torch.cuda.synchronize()
    return got, plan


def w_scales_distinct(rows, K):
    """Block scales 2^-2 .. 2^2 that differ between neighbouring blocks of a row (so between the blocks of a K-tile and
    between K-tiles) and between neighbouring rows."""
    r, b = torch.arange(rows)[:, None], torch.arange(K // 32)[None]
    return (127 + (r + b) % 5 - 2).to(torch.uint8)


def exact_w4(rows, K, seed, one_hot=False):
    """e2m1 weights on exact data: elements in {0, +-0.5 .. +-3}, or one non-zero element per row (every k of the K-tile and
    every sign and magnitude is met over the rows).  -> (codes, scales, fp64 values) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0], dtype=torch.float64)
    if one_hot:
        el = torch.zeros(rows, K, dtype=torch.float64)
        n = torch.arange(rows)
        el[n, (n * 37 + 5) % K] = vals[1 + n % 10]
    else:
        el = vals[torch.randint(0, len(vals), (rows, K), generator=g)]
    codes, scales = pack4(e2m1_encode(el)), w_scales_distinct(rows, K)
    v = dequant(codes, scales, WFMT)
    assert torch.equal(v, torch.ldexp(el.reshape(rows, -1, 32), (scales.long() - 127)[..., None].double()).reshape(rows, K))
    return codes, scales, v


def exact_a8(rows, K, dev, seed, batch=1):
    c, s = exact_operand(batch * rows, K, FMT, seed)
    v = dequant(c, s, FMT)
    lead = (batch, rows) if batch > 1 else (rows,)
    return c.reshape(*lead, -1).to(dev), s.reshape(*lead, -1).to(dev), v.reshape(*lead, -1).to(dev)


@pytest.mark.parametrize("one_hot", [False, True], ids=["grid", "onehot"])
@pytest.mark.parametrize("M,N", [(1, 8), (300, 264)])
def test_w4_operand_and_scale_map_on_exact_data(dev, M, N, one_hot):
    """K = 512 under kernel = 2: every product is a multiple of 2^-6 below 2^8 and every partial sum exact in fp32, so the
    result EQUALS the closed form rounded to bf16.  A wrong nibble order, chunk swizzle, lane -> block map, slot row, stale ring
    stage or scale byte changes the answer; the one-hot rows name the k that went wrong."""
    K = 512
    ac, asc, a = exact_a8(M, K, dev, seed=M)
    wc, wsc, w = exact_w4(N, K, seed=N + 1, one_hot=one_hot)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    _, plan = call(2, "p256", ac, asc, wc.to(dev), wsc.to(dev), out)
    assert_exact(out, a @ w.to(dev).T, plan, f"w4 operand map {M}x{N}x{K}")


@pytest.mark.parametrize("B,M,N,K,kernel", [
    (1, 1, 8, 1024, 2),             # one tile
    (1, 300, 264, 512, 2),          # four tiles: most workgroups have none
    (2, 1811, 3848, 640, 1),        # odd K-tile count, batch
    (1, 3621, 3848, 512, 1),        # 240 tiles, ragged M and N; the shortest K: each K-tile variant A / B / C / D once
])
def test_w4_exact_data_with_the_whole_epilogue(dev, B, M, N, K, kernel):
    """Bias, GELU(tanh), two gates split at a row, the residual in place and n_split = the whole width, on exact operands:
    bit for bit kernel = 0 of the same call, guard bands intact."""
    ac, asc, a = exact_a8(M, K, dev, seed=M + K, batch=B)
    wc, wsc, w = exact_w4(N, K, seed=N + K + 1)
    wc, wsc, w = wc.to(dev), wsc.to(dev), w.to(dev)
    split = M // 3
    epi = exact_epilogue(w, dev, seed=7, bias=True, gates=True, res_rows=M, batch=B)
    res = epi["res"] if B > 1 else epi["res"][0]
    got = {}
    for k, want in ((0, "t128x128"), (kernel, "p256")):
        out = GuardedOut(M, N, dev, batch=B)
        out.fill(res)
        call(k, want, ac, asc, wc, wsc, out.view(), bias=epi["bias"], res=out.view(), gate0=epi["gate0"], gate1=epi["gate1"],
             gate_split=split)
        assert out.guard_intact()
        got[k] = out.gathered()
    assert not bool(torch.isnan(got[0].float()).any())
    assert torch.equal(bits(got[0]), bits(got[kernel]))
    # ... with an activation and a column split (no residual with a split)
    got = {}
    for k, want in ((0, "t128x128"), (kernel, "p256")):
        parts = 2 if N % 16 == 0 else 1
        out = GuardedOut(M, N, dev, batch=B, parts=parts)
        call(k, want, ac, asc, wc, wsc, out.view(), bias=epi["bias"], act="gelu_tanh", split=out.split)
        assert out.guard_intact()
        got[k] = out.gathered()
    assert torch.equal(bits(got[0]), bits(got[kernel])) and not bool(torch.isnan(got[0].float()).any())


_W4 = {}


def spread_w4(rows, K, dev, seed):
    """Quantised gaussian weight rows whose blocks spread over 20 binades, with all-zero blocks, in e2m1 (by the device
    quantiser, which tests/test_mxfp4_gpu.py holds to the definition byte for byte)."""
    from bind_your_avatar_implementation_amd import ops
    key = (rows, K, seed)
    if key not in _W4:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(rows, K // 32, 32, generator=g) * torch.exp2(torch.randint(-10, 11, (rows, K // 32, 1), generator=g).float())
        x[torch.rand(rows, K // 32, generator=g) < 0.02] = 0.0
        _W4[key] = ops.quantize_mx(x.reshape(rows, K).to(torch.bfloat16).to(dev), WFMT)
    return _W4[key]


@pytest.mark.parametrize("case", ["k3072", "k12288", "qkv_split", "batch"])
def test_w4_equals_the_128_tile_kernel_bit_for_bit(dev, case):
    B, M, N, K, parts, kernel = {"k3072": (1, 3621, 3848, 3072, 1, 1), "k12288": (1, 300, 264, 12288, 1, 2),
                                 "qkv_split": (1, 3621, 3840, 3072, 3, 1), "batch": (2, 1811, 3848, 1024, 1, 1)}[case]
    ac, asc = spread(B * M, K, dev, 1)
    wc, wsc = spread_w4(N, K, dev, 2)
    if B > 1:
        ac, asc = ac.view(B, M, -1), asc.view(B, M, -1)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(3)) * 4).to(torch.bfloat16).to(dev)
    got = {}
    for k, want in ((0, "t128x128"), (kernel, "p256")):
        out = GuardedOut(M, N, dev, batch=B, parts=parts)
        call(k, want, ac, asc, wc, wsc, out.view(), bias=bias, split=out.split)
        assert out.guard_intact()
        got[k] = out.gathered()
    assert not bool(torch.isnan(got[0].float()).any()) and float(got[0].float().abs().sum()) > 0
    assert torch.equal(bits(got[0]), bits(got[kernel]))
    if case == "k12288":
        # kernel = 0 of the new call is the old entry point
        from bind_your_avatar_implementation_amd import ops
        old = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac, asc, wc, wsc, old, FMT, bias=bias, w_fmt=WFMT)
        assert torch.equal(bits(old), bits(got[0]))


@pytest.mark.parametrize("M,N,K,kernel", [(300, 256, 512, 2), (3621, 3840, 512, 1)])
@pytest.mark.parametrize("epi", [False, True], ids=["plain", "bias_gelu"])
def test_w4_quantising_epilogue_writes_the_128_tile_kernels_bytes(dev, M, N, K, kernel, epi):
    from bind_your_avatar_implementation_amd import ops
    ac, asc = spread(M, K, dev, 4)
    wc, wsc = spread_w4(N, K, dev, 5)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(6)) * 4).to(torch.bfloat16).to(dev) if epi else None
    act = "gelu_tanh" if epi else None
    PADR = 3                                # canary rows behind the M rows
    got = {}
    for k, want in ((0, "t128x128"), (kernel, "p256")):
        codes = torch.full((M + PADR, N), 0xAA, dtype=torch.uint8, device=dev)
        scales = torch.full((M + PADR, N // 32), 0xAA, dtype=torch.uint8, device=dev)
        call(k, want, ac, asc, wc, wsc, codes[:M], out_scales=scales[:M], out_fmt=FMT, bias=bias, act=act)
        assert bool((codes[M:] == 0xAA).all()) and bool((scales[M:] == 0xAA).all())
        got[k] = (codes[:M].clone(), scales[:M].clone())
    assert torch.equal(got[0][0], got[kernel][0]) and torch.equal(got[0][1], got[kernel][1])
    assert bool((got[0][0] != 0).any())
    # ... and the old entry point's bytes
    oc, osc = torch.empty(M, N, dtype=torch.uint8, device=dev), torch.empty(M, N // 32, dtype=torch.uint8, device=dev)
    ops.gemm_mx_quant(ac, asc, wc, wsc, oc, osc, fmt=FMT, w_fmt=WFMT, out_fmt=FMT, bias=bias, act=act)
    assert torch.equal(oc, got[kernel][0]) and torch.equal(osc, got[kernel][1])


def test_w4_quant_row_stride_padding_is_left_alone(dev):
    """Codes in a buffer whose row stride is wider than N: the padding keeps its canary bytes (through the C ABI)."""
    from bind_your_avatar_implementation_amd import _hip, ops
    M, N, K, LD = 300, 256, 512, 256 + 64
    ac, asc = spread(M, K, dev, 4)
    wc, wsc = spread_w4(N, K, dev, 5)
    d = ops._mx_quant_desc(ac, asc, wc, wsc, torch.empty(M, N, dtype=torch.uint8, device=dev),
                           torch.empty(M, N // 32, dtype=torch.uint8, device=dev), FMT, WFMT, FMT, None, 1.0)
    d.ldc = LD
    lib = _hip.load()
    got = {}
    for k, want in ((0, 1), (2, 4)):
        codes = torch.full((M + 2, LD), 0xAA, dtype=torch.uint8, device=dev)
        scales = torch.full((M + 2, N // 32), 0xAA, dtype=torch.uint8, device=dev)
        c = _hip.MxGemmCall()
        c.A, c.a_scales, c.W, c.w_scales, c.C, c.q_scales = (t.data_ptr() for t in (ac, asc, wc, wsc, codes, scales))
        c.a_fmt, c.w_fmt, c.out_fmt, c.kernel = 0, 4, 0, k
        p = _hip.GemmPlan()
        assert lib.bya_gemm_mx_call_plan(ctypes.byref(c), ctypes.byref(d), ctypes.byref(p)) == 0 and p.path == want
        assert lib.bya_gemm_mx_call(ctypes.byref(c), ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert bool((codes[:, N:] == 0xAA).all()) and bool((codes[M:] == 0xAA).all()) and bool((scales[M:] == 0xAA).all())
        got[k] = (codes, scales)
    assert torch.equal(got[0][0], got[2][0]) and torch.equal(got[0][1], got[2][1])


def fused_call(dev, ac, asc, wc, wsc, bias, M, width, text, kernel, expect, tensors=3, fmt=FMT, w_fmt=WFMT):
    """The q/k-norm launch of the new call into a NaN-filled [tensors + 1, M + PAD, width] buffer (pair_and_fused's layout)."""
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    one = nan_buffer(dev, tensors + 1, M + PAD, width)
    norm = dict(qw=qw, qb=qb, kw=kw, kb=kb, cos=cos, sin=sin, text_rows=text, eps=EPS, k_scale=K_SCALE, tensors=tensors)
    got, plan = call(kernel, expect, ac, asc, wc, wsc, one[0, :M], fmt, w_fmt, bias=bias, split=(width, (M + PAD) * width),
                     norm=norm)
    assert got is True and plan["row_chunks"] == 1
    return one


# (M, width, K, text rows, kernel): a ragged row tile with the text / video boundary inside a 16-row fragment and q | k at
# column 192 inside a wave's 128 columns; all text (cos and sin None); 14 x 15 = 210 tiles with q | k at 1216 and k | v at 2432
# inside waves and a quarter-full last column tile
QKN_SHAPES = [(300, 192, 512, 40, 2), (300, 192, 512, 300, 2), (3500, 1216, 512, 226, 1)]


@pytest.mark.parametrize("M,width,K,text,kernel", QKN_SHAPES)
def test_w4_qkn_epilogue_equals_two_launches_and_the_tiled_kernel(dev, M, width, K, text, kernel):
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, FMT, WFMT)
    two, tiled = pair_and_fused(dev, ac, asc, wc, wsc, bias, FMT, WFMT, M, width, text, expect="t128x128")
    one = fused_call(dev, ac, asc, wc, wsc, bias, M, width, text, kernel, "p256")
    check_equal_and_canaries(two, one, M, 3)
    assert torch.equal(bits(one), bits(tiled))
    assert float(one[:3, :M].float().abs().sum()) > 0
    zero = fused_call(dev, ac, asc, wc, wsc, bias, M, width, text, 0, "t128x128")
    assert torch.equal(bits(zero), bits(one))


def test_w4_qkn_q_and_k_alone(dev):
    M, width, K, text = 300, 192, 512, 40
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, FMT, WFMT)
    wc2, wsc2, bias2 = wc[:2 * width].contiguous(), wsc[:2 * width].contiguous(), bias[:2 * width].contiguous()
    two, _ = pair_and_fused(dev, ac, asc, wc2, wsc2, bias2, FMT, WFMT, M, width, text, tensors=2)
    one = fused_call(dev, ac, asc, wc2, wsc2, bias2, M, width, text, 2, "p256", tensors=2)
    check_equal_and_canaries(two, one, M, 2)


@pytest.mark.parametrize("fmt,M,N,K,kernel", [("mxfp6", 300, 264, 512, 2), ("mxfp8", 300, 264, 384, 2), ("mxfp8", 300, 264, 512, 1)],
                         ids=["mxfp6_x_mxfp4", "three_k_tiles", "four_tiles_under_kernel_1"])
def test_w4_fallbacks_run_the_tiled_kernel(dev, fmt, M, N, K, kernel):
    from bind_your_avatar_implementation_amd import ops
    ac, asc, wc, wsc, bias = operands(dev, M, N, K, fmt, WFMT)
    old = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.gemm_mx(ac, asc, wc, wsc, old, fmt, bias=bias, w_fmt=WFMT)
    new = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    call(kernel, "t128x128", ac, asc, wc, wsc, new, fmt, WFMT, bias=bias)
    assert torch.equal(bits(old), bits(new)) and not bool(torch.isnan(new.float()).any())


# ------------------------------------------------------------------------------------------ engine
class CallRecorder:
    """Wraps ops.gemm_mx_call: keeps (epilogue, kernel argument, plan path) of every launch."""

    def __init__(self, fn, plan_fn):
        self.fn, self.plan_fn, self.calls = fn, plan_fn, []

    def __call__(self, *a, **kw):
        plan = self.plan_fn(*a, **kw)
        epi = "qkn" if kw.get("norm") is not None else "quant" if kw.get("out_scales") is not None else "bf16"
        self.calls.append((epi, a[5], plan and plan["path"]))
        return self.fn(*a, **kw)


def recorded_forward(model, gi, monkeypatch):
    from bind_your_avatar_implementation_amd import ops
    model(**gi)                                                                           # builds the engine (packs weights)
    with monkeypatch.context() as mp:
        c = CallRecorder(ops.gemm_mx_call, ops.gemm_mx_call_plan)
        old = [Counter(ops.gemm_mx), Counter(ops.gemm_mx_quant), Counter(ops.gemm_mx_qkv_norm_rope)]
        mp.setattr(ops, "gemm_mx_call", c)
        for name, o in zip(("gemm_mx", "gemm_mx_quant", "gemm_mx_qkv_norm_rope"), old):
            mp.setattr(ops, name, o)
        out = model(**gi)[0].clone()
    return out, c.calls, sum(o.n for o in old)


def replay_equals(model, gi, want):
    model.use_hip_graph = True
    try:
        model(**gi)                                                                       # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], want)
    finally:
        model.use_hip_graph = False
        model._graphs = {}


def test_engine_step_with_mxfp4_weights_on_the_persistent_kernel_keeps_its_bits(dev, monkeypatch):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    model.enable_mx_weights("mxfp8", weight_format="mxfp4")
    off, c_off, n_off = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_call_kernel == 0 and c_off == [] and n_off == 4 * blocks
    model.enable_mx_weights("mxfp8", weight_format="mxfp4", persistent_gemm="always")
    assert model._engine is None                                                          # the switch invalidates the engine
    on, c_on, n_on = recorded_forward(model, gi, monkeypatch)
    print(f"gemm_mx_call launches {c_on}")
    assert model._engine.mx_call_kernel == 2 and model._engine.mx_kernel == 0 and n_on == 0
    # qkv, out, ff2 per block with the bf16 epilogue, ff1 with the quantising one: kernel 2, all on the persistent kernel
    assert sorted(c_on) == sorted([("bf16", 2, "p256")] * (3 * blocks) + [("quant", 2, "p256")] * blocks)
    assert torch.equal(on, off)
    replay_equals(model, gi, off)
    # with the fused q|k|v launch and the attention writing to_out's operand
    model.enable_mx_weights("mxfp8", weight_format="mxfp4", persistent_gemm="always", fuse_qk_norm=True, fuse_attention_quant=True)
    both, c_both, n_both = recorded_forward(model, gi, monkeypatch)
    assert n_both == 0 and sorted(c_both) == sorted([("bf16", 2, "p256")] * (2 * blocks) + [("quant", 2, "p256")] * blocks +
                                                    [("qkn", 2, "p256")] * blocks)
    model.enable_mx_weights("mxfp8", weight_format="mxfp4", fuse_qk_norm=True, fuse_attention_quant=True)
    ref_both, c_ref, _ = recorded_forward(model, gi, monkeypatch)
    assert c_ref == [] and torch.equal(both, ref_both) and torch.equal(both, off)
    model.enable_mx_weights("mxfp8", weight_format="mxfp4", persistent_gemm="always", fuse_qk_norm=True, fuse_attention_quant=True)
    model(**gi)
    replay_equals(model, gi, off)
    # mxfp6 activations: the switch changes no launch
    model.enable_mx_weights("mxfp6", weight_format="mxfp4")
    ref6, _, n6 = recorded_forward(model, gi, monkeypatch)
    model.enable_mx_weights("mxfp6", weight_format="mxfp4", persistent_gemm="always")
    got6, c6, n6p = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_call_kernel == 0 and c6 == [] and n6p == n6 and torch.equal(got6, ref6)
