"""The persistent one-wave-per-SIMD 256 x 256 MX GEMM on mxfp6 (e2m3) activations with mxfp6 or mxfp4 weights, and its
quantising epilogue for mxfp6 output (csrc/gemm_mx_v4.hip, gemm256p_mx_kernel<.., MX_E2M3>; bya_gemm_mx_call with
BYA_MX_KERNEL_FP6, ops.gemm_mx_call(..., kernel=17 / 18)): the operand and scale map on exact data against the closed form, then
bit for bit against the tiled kernels of csrc/gemm_mx.hip on the same bytes (kernel = 16 of the same call) under the bf16, the
quantising and the q/k-norm + RoPE epilogue, the fallbacks, and the engine's step with
enable_mx_weights("mxfp6", persistent_gemm_mxfp6=...).  No tolerance anywhere: every comparison is torch.equal on bit patterns,
and the plan is asserted before every launch.  The smallest exact-data case comes first."""
import pytest
import torch

from exact_gemm import GuardedOut, assert_exact, exact_epilogue
from test_mx_cpu import dequant_mx, e2m3_encode, pack6
from test_mx_gpu import exact_operand
from test_mx_p256_gpu import spread as spread8
from test_mx_p256_w4_gpu import (call, exact_w4, fused_call, recorded_forward, replay_equals, spread_w4,
                                 w_scales_distinct)
from test_mx_qkn_gpu import bits, check_equal_and_canaries, operands, pair_and_fused

pytestmark = pytest.mark.gpu
FMT = "mxfp6"
PAIRS = ["mxfp6", "mxfp4"]                  # the weights' format under mxfp6 activations


def tiled(M, N, B=1):
    """The tiled kernel of an mxfp6 launch: 256 x 256 tiles from 200 of them."""
    return "t256x256" if -(-M // 256) * -(-N // 256) * B >= 200 else "t128x128"


def exact_a6(rows, K, dev, seed, batch=1):
    c, s = exact_operand(batch * rows, K, FMT, seed)
    v = dequant_mx(c, s, FMT)
    lead = (batch, rows) if batch > 1 else (rows,)
    return c.reshape(*lead, -1).to(dev), s.reshape(*lead, -1).to(dev), v.reshape(*lead, -1).to(dev)


def exact_w6(rows, K, seed, one_hot=False):
    """e2m3 weights on exact data with a distinct scale per block: exact_operand's elements, or one non-zero element per row
    (every k of the K-tile and every sign and magnitude is met over the rows).  -> (codes, scales, fp64 values) on the CPU."""
    scales = w_scales_distinct(rows, K)
    if one_hot:
        vals = torch.tensor([0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0], dtype=torch.float64)
        el = torch.zeros(rows, K, dtype=torch.float64)
        n = torch.arange(rows)
        el[n, (n * 37 + 5) % K] = vals[n % 10]
        codes = pack6(e2m3_encode(el))
    else:
        codes, _ = exact_operand(rows, K, FMT, seed)
    return codes, scales, dequant_mx(codes, scales, FMT)


def exact_w(w_fmt, rows, K, seed, one_hot=False):
    return exact_w6(rows, K, seed, one_hot) if w_fmt == "mxfp6" else exact_w4(rows, K, seed, one_hot)


@pytest.mark.parametrize("one_hot", [False, True], ids=["grid", "onehot"])
@pytest.mark.parametrize("w_fmt", PAIRS)
@pytest.mark.parametrize("M,N", [(1, 8), (300, 264)])
def test_fp6_operand_and_scale_map_on_exact_data(dev, M, N, w_fmt, one_hot):
    """K = 512 under kernel = 18: every product is a multiple of 2^-6 below 2^8 and every partial sum exact in fp32, so the
    result EQUALS the closed form rounded to bf16.  A wrong row rotation, lane -> block map, 6-bit element order, slot row, stale
    ring stage or scale byte changes the answer; the one-hot rows name the k that went wrong."""
    K = 512
    ac, asc, a = exact_a6(M, K, dev, seed=M)
    wc, wsc, w = exact_w(w_fmt, N, K, seed=N + 1, one_hot=one_hot)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    _, plan = call(18, "p256", ac, asc, wc.to(dev), wsc.to(dev), out, FMT, w_fmt)
    assert_exact(out, a @ w.to(dev).T, plan, f"fp6 x {w_fmt} operand map {M}x{N}x{K}")


@pytest.mark.parametrize("w_fmt", PAIRS)
@pytest.mark.parametrize("B,M,N,K,kernel", [
    (1, 1, 8, 1024, 18),            # one tile
    (1, 300, 264, 512, 18),         # four tiles: most workgroups have none
    (2, 1811, 3848, 640, 17),       # odd K-tile count, batch
    (1, 3621, 3848, 512, 17),       # 240 tiles, ragged M and N; the shortest K: each K-tile variant A / B / C / D once
])
def test_fp6_exact_data_with_the_whole_epilogue(dev, B, M, N, K, kernel, w_fmt):
    """Bias, GELU(tanh), two gates split at a row, the residual in place and n_split = the whole width, on exact operands:
    bit for bit kernel = 16 of the same call, guard bands intact."""
    ac, asc, a = exact_a6(M, K, dev, seed=M + K, batch=B)
    wc, wsc, w = exact_w(w_fmt, N, K, seed=N + K + 1)
    wc, wsc, w = wc.to(dev), wsc.to(dev), w.to(dev)
    split = M // 3
    epi = exact_epilogue(w, dev, seed=7, bias=True, gates=True, res_rows=M, batch=B)
    res = epi["res"] if B > 1 else epi["res"][0]
    got = {}
    for k, want in ((16, tiled(M, N, B)), (kernel, "p256")):
        out = GuardedOut(M, N, dev, batch=B)
        out.fill(res)
        call(k, want, ac, asc, wc, wsc, out.view(), FMT, w_fmt, bias=epi["bias"], res=out.view(), gate0=epi["gate0"],
             gate1=epi["gate1"], gate_split=split)
        assert out.guard_intact()
        got[k] = out.gathered()
    assert not bool(torch.isnan(got[16].float()).any())
    assert torch.equal(bits(got[16]), bits(got[kernel]))
    # ... with an activation and a column split (no residual with a split)
    got = {}
    for k, want in ((16, tiled(M, N, B)), (kernel, "p256")):
        parts = 2 if N % 16 == 0 else 1
        out = GuardedOut(M, N, dev, batch=B, parts=parts)
        call(k, want, ac, asc, wc, wsc, out.view(), FMT, w_fmt, bias=epi["bias"], act="gelu_tanh", split=out.split)
        assert out.guard_intact()
        got[k] = out.gathered()
    assert torch.equal(bits(got[16]), bits(got[kernel])) and not bool(torch.isnan(got[16].float()).any())


_SPREAD6 = {}


def spread6(rows, K, dev, seed):
    """Quantised gaussian rows whose blocks spread over 20 binades, with all-zero blocks, in e2m3 (by the device quantiser, which
    tests/test_mx_gpu.py holds to the definition byte for byte)."""
    from bind_your_avatar_implementation_amd import ops
    key = (rows, K, seed)
    if key not in _SPREAD6:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(rows, K // 32, 32, generator=g) * torch.exp2(torch.randint(-10, 11, (rows, K // 32, 1), generator=g).float())
        x[torch.rand(rows, K // 32, generator=g) < 0.02] = 0.0
        _SPREAD6[key] = ops.quantize_mx(x.reshape(rows, K).to(torch.bfloat16).to(dev), FMT)
    return _SPREAD6[key]


def spread_w(w_fmt, rows, K, dev, seed):
    return spread6(rows, K, dev, seed) if w_fmt == "mxfp6" else spread_w4(rows, K, dev, seed)


@pytest.mark.parametrize("w_fmt", PAIRS)
@pytest.mark.parametrize("case", ["k3072", "k12288", "qkv_split", "batch"])
def test_fp6_equals_the_tiled_kernel_bit_for_bit(dev, case, w_fmt):
    B, M, N, K, parts, kernel = {"k3072": (1, 3621, 3848, 3072, 1, 17), "k12288": (1, 300, 264, 12288, 1, 18),
                                 "qkv_split": (1, 3621, 3840, 3072, 3, 17), "batch": (2, 1811, 3848, 1024, 1, 17)}[case]
    ac, asc = spread6(B * M, K, dev, 1)
    wc, wsc = spread_w(w_fmt, N, K, dev, 2)
    if B > 1:
        ac, asc = ac.view(B, M, -1), asc.view(B, M, -1)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(3)) * 4).to(torch.bfloat16).to(dev)
    got = {}
    for k, want in ((16, tiled(M, N, B)), (kernel, "p256")):
        out = GuardedOut(M, N, dev, batch=B, parts=parts)
        call(k, want, ac, asc, wc, wsc, out.view(), FMT, w_fmt, bias=bias, split=out.split)
        assert out.guard_intact()
        got[k] = out.gathered()
    assert not bool(torch.isnan(got[16].float()).any()) and float(got[16].float().abs().sum()) > 0
    assert torch.equal(bits(got[16]), bits(got[kernel]))
    if case == "k12288":
        # kernel = 16 of the call is the old entry point
        from bind_your_avatar_implementation_amd import ops
        old = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac, asc, wc, wsc, old, FMT, bias=bias, w_fmt=w_fmt)
        assert torch.equal(bits(old), bits(got[16]))


# (activations, weights, output): mxfp6 and mxfp8 output from e2m3 operands, mxfp6 output from mxfp8 operands
QUANT_FORMATS = [("mxfp6", "mxfp6", "mxfp6"), ("mxfp6", "mxfp4", "mxfp6"), ("mxfp6", "mxfp6", "mxfp8"), ("mxfp6", "mxfp4", "mxfp8"),
                 ("mxfp8", "mxfp8", "mxfp6"), ("mxfp8", "mxfp4", "mxfp6")]


@pytest.mark.parametrize("M,N,K,kernel", [(300, 256, 512, 18), (3621, 3840, 512, 17)])
@pytest.mark.parametrize("fmt,w_fmt,out_fmt", QUANT_FORMATS, ids=["x".join(f) for f in QUANT_FORMATS])
def test_fp6_quantising_epilogue_writes_the_tiled_kernels_bytes(dev, M, N, K, kernel, fmt, w_fmt, out_fmt):
    """Codes and scale bytes equal kernel = 16's, plain and with bias + GELU(tanh); 0xAA canaries behind the M rows stay (behind
    N and in the row pitch: the next test); the pair is accepted as the next GEMM's operand."""
    from bind_your_avatar_implementation_amd import ops
    ac, asc = spread6(M, K, dev, 4) if fmt == "mxfp6" else spread8(M, K, dev, 4)
    wc, wsc = spread_w(w_fmt, N, K, dev, 5) if w_fmt != "mxfp8" else spread8(N, K, dev, 5)
    row_bytes = N * {"mxfp6": 6, "mxfp8": 8}[out_fmt] // 8
    PADR = 3                                         # canary rows behind the M rows
    want0 = tiled(M, N) if fmt == "mxfp6" else "t128x128"
    for epi in (False, True):
        bias = (torch.randn(N, generator=torch.Generator().manual_seed(6)) * 4).to(torch.bfloat16).to(dev) if epi else None
        act = "gelu_tanh" if epi else None
        got = {}
        for k, want in ((16, want0), (kernel, "p256")):
            codes = torch.full((M + PADR, row_bytes), 0xAA, dtype=torch.uint8, device=dev)
            scales = torch.full((M + PADR, N // 32), 0xAA, dtype=torch.uint8, device=dev)
            call(k, want, ac, asc, wc, wsc, codes[:M], fmt, w_fmt, out_scales=scales[:M], out_fmt=out_fmt, bias=bias, act=act)
            assert bool((codes[M:] == 0xAA).all()) and bool((scales[M:] == 0xAA).all())
            got[k] = (codes[:M].clone(), scales[:M].clone())
        assert torch.equal(got[16][0], got[kernel][0]) and torch.equal(got[16][1], got[kernel][1])
        assert bool((got[16][0] != 0).any())
        # ... and the old entry point's bytes
        oc = torch.empty(M, row_bytes, dtype=torch.uint8, device=dev)
        osc = torch.empty(M, N // 32, dtype=torch.uint8, device=dev)
        ops.gemm_mx_quant(ac, asc, wc, wsc, oc, osc, fmt=fmt, w_fmt=w_fmt, out_fmt=out_fmt, bias=bias, act=act)
        assert torch.equal(oc, got[kernel][0]) and torch.equal(osc, got[kernel][1])
    # the pair is the next GEMM's operand: (M, N) codes in out_fmt against out_fmt weights, on either kernel
    w2c, w2s = (spread6 if out_fmt == "mxfp6" else spread8)(264, N, dev, 8)
    nxt = {}
    for k, want in ((16, "t128x128"), (18, "p256" if N >= 512 else "t128x128")):       # (N is the next K: four K-tiles or more)
        out = torch.full((M, 264), float("nan"), dtype=torch.bfloat16, device=dev)
        call(k, want, got[kernel][0], got[kernel][1], w2c, w2s, out, out_fmt, out_fmt)
        nxt[k] = out
    assert torch.equal(bits(nxt[16]), bits(nxt[18])) and not bool(torch.isnan(nxt[16].float()).any())


@pytest.mark.parametrize("fmt,w_fmt", [("mxfp6", "mxfp6"), ("mxfp6", "mxfp4"), ("mxfp8", "mxfp8")])
def test_fp6_quant_bytes_behind_n_and_the_row_pitch_are_left_alone(dev, fmt, w_fmt):
    """mxfp6 codes in a buffer whose row stride is wider than the row's 3 N / 4 bytes: the bytes behind N -- the padding of the
    pitch -- and the rows behind M keep their canary bytes (through the C ABI), a ragged last row tile included."""
    import ctypes
    from bind_your_avatar_implementation_amd import _hip, ops
    M, N, K = 300, 256, 512
    RB, LD = N * 6 // 8, N * 6 // 8 + 64
    ac, asc = spread6(M, K, dev, 4) if fmt == "mxfp6" else spread8(M, K, dev, 4)
    wc, wsc = spread_w(w_fmt, N, K, dev, 5) if w_fmt != "mxfp8" else spread8(N, K, dev, 5)
    d = ops._mx_quant_desc(ac, asc, wc, wsc, torch.empty(M, RB, dtype=torch.uint8, device=dev),
                           torch.empty(M, N // 32, dtype=torch.uint8, device=dev), fmt, w_fmt, FMT, None, 1.0)
    d.ldc = LD
    lib = _hip.load()
    code = {"mxfp8": 0, "mxfp6": 2, "mxfp4": 4}
    got = {}
    for k, want in ((16, 1), (18, 4)):
        codes = torch.full((M + 2, LD), 0xAA, dtype=torch.uint8, device=dev)
        scales = torch.full((M + 2, N // 32), 0xAA, dtype=torch.uint8, device=dev)
        c = _hip.MxGemmCall()
        c.A, c.a_scales, c.W, c.w_scales, c.C, c.q_scales = (t.data_ptr() for t in (ac, asc, wc, wsc, codes, scales))
        c.a_fmt, c.w_fmt, c.out_fmt, c.kernel = code[fmt], code[w_fmt], code[FMT], k
        p = _hip.GemmPlan()
        assert lib.bya_gemm_mx_call_plan(ctypes.byref(c), ctypes.byref(d), ctypes.byref(p)) == 0 and p.path == want
        assert lib.bya_gemm_mx_call(ctypes.byref(c), ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert bool((codes[:, RB:] == 0xAA).all()) and bool((codes[M:] == 0xAA).all()) and bool((scales[M:] == 0xAA).all())
        assert bool((codes[:M, :RB] != 0xAA).any())
        got[k] = (codes, scales)
    assert torch.equal(got[16][0], got[18][0]) and torch.equal(got[16][1], got[18][1])


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("w_fmt", PAIRS)
@pytest.mark.parametrize("M,width,K,text,kernel", [(300, 192, 512, 40, 18), (3500, 1216, 512, 226, 17)])
def test_fp6_qkn_epilogue_equals_two_launches_and_the_tiled_kernel(dev, M, width, K, text, kernel, w_fmt, with_bias):
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, FMT, w_fmt)
    bias = bias if with_bias else None
    want0 = tiled(M, 3 * width)
    two, tiled_one = pair_and_fused(dev, ac, asc, wc, wsc, bias, FMT, w_fmt, M, width, text, expect=want0)
    one = fused_call(dev, ac, asc, wc, wsc, bias, M, width, text, kernel, "p256", fmt=FMT, w_fmt=w_fmt)
    check_equal_and_canaries(two, one, M, 3)
    assert torch.equal(bits(one), bits(tiled_one))
    assert float(one[:3, :M].float().abs().sum()) > 0
    zero = fused_call(dev, ac, asc, wc, wsc, bias, M, width, text, 16, want0, fmt=FMT, w_fmt=w_fmt)
    assert torch.equal(bits(zero), bits(one))


@pytest.mark.parametrize("w_fmt", PAIRS)
@pytest.mark.parametrize("M,N,K,misalign", [(300, 264, 384, False), (300, 260, 512, False), (300, 264, 512, True)],
                         ids=["three_k_tiles", "n_not_a_multiple_of_8", "misaligned_bias"])
def test_fp6_fallbacks_run_the_tiled_kernel(dev, M, N, K, misalign, w_fmt):
    from bind_your_avatar_implementation_amd import ops
    ac, asc, wc, wsc, bias = operands(dev, M, N, K, FMT, w_fmt)
    if misalign:                                    # 8-byte aligned: legal for the tiled kernel, not for the persistent one
        buf = torch.empty(N + 4, dtype=torch.bfloat16, device=dev)
        buf[4:] = bias
        bias = buf[4:]
        assert bias.data_ptr() % 16 == 8
    old = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.gemm_mx(ac, asc, wc, wsc, old, FMT, bias=bias, w_fmt=w_fmt)
    new = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    call(18, "t128x128", ac, asc, wc, wsc, new, FMT, w_fmt, bias=bias)
    assert torch.equal(bits(old), bits(new)) and not bool(torch.isnan(new.float()).any())


# ------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("w_fmt", PAIRS)
def test_engine_step_with_mxfp6_activations_on_the_persistent_kernel_keeps_its_bits(dev, monkeypatch, w_fmt):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    model.enable_mx_weights(FMT, weight_format=w_fmt)
    off, c_off, n_off = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_call_kernel == 0 and c_off == [] and n_off == 4 * blocks
    model.enable_mx_weights(FMT, weight_format=w_fmt, persistent_gemm_mxfp6="always")
    assert model._engine is None                                                          # the switch invalidates the engine
    on, c_on, n_on = recorded_forward(model, gi, monkeypatch)
    print(f"gemm_mx_call launches {c_on}")
    assert model._engine.mx_call_kernel == 18 and model._engine.mx_kernel == 0 and n_on == 0
    # qkv, out, ff2 per block with the bf16 epilogue, ff1 with the quantising one (to e2m3): kernel 18, all on the persistent kernel
    assert sorted(c_on) == sorted([("bf16", 18, "p256")] * (3 * blocks) + [("quant", 18, "p256")] * blocks)
    assert torch.equal(on, off)
    replay_equals(model, gi, off)
    # with the fused q|k|v launch and the attention writing to_out's operand
    model.enable_mx_weights(FMT, weight_format=w_fmt, persistent_gemm_mxfp6="always", fuse_qk_norm=True, fuse_attention_quant=True)
    both, c_both, n_both = recorded_forward(model, gi, monkeypatch)
    assert n_both == 0 and sorted(c_both) == sorted([("bf16", 18, "p256")] * (2 * blocks) + [("quant", 18, "p256")] * blocks +
                                                    [("qkn", 18, "p256")] * blocks)
    model.enable_mx_weights(FMT, weight_format=w_fmt, fuse_qk_norm=True, fuse_attention_quant=True)
    ref_both, c_ref, _ = recorded_forward(model, gi, monkeypatch)
    assert c_ref == [] and torch.equal(both, ref_both) and torch.equal(both, off)
    model.enable_mx_weights(FMT, weight_format=w_fmt, persistent_gemm_mxfp6="always", fuse_qk_norm=True, fuse_attention_quant=True)
    model(**gi)
    replay_equals(model, gi, off)
    # True: the tile count decides (the small model's launches stay tiled), through the same call
    model.enable_mx_weights(FMT, weight_format=w_fmt, persistent_gemm_mxfp6=True)
    few, c_few, n_few = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_call_kernel == 17 and n_few == 0 and len(c_few) == 4 * blocks and torch.equal(few, off)


def test_engine_with_mxfp8_activations_ignores_the_mxfp6_switch(dev, monkeypatch):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    model.enable_mx_weights("mxfp8")
    ref, c_ref, n_ref = recorded_forward(model, gi, monkeypatch)
    model.enable_mx_weights("mxfp8", persistent_gemm_mxfp6=True)
    got, c_got, n_got = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_call_kernel == 0 and model._engine.mx_kernel == 0
    assert c_ref == [] and c_got == [] and n_got == n_ref and torch.equal(got, ref)
