"""Every GEMM kernel on exact data (tests/exact_gemm.py): each case first asserts, through the plan query of its entry point,
that it reaches the kernel it is written for, then that the result equals the exact product rounded to bf16 BIT FOR BIT, with
the output poisoned before the launch and a guard band around it that must survive.  The case tables are module constants:
test_gemm_exact_cpu.py plans them on meta tensors and checks that together they cover every kernel the planners can return."""
import pytest
import torch
import torch.nn.functional as F

from exact_gemm import (BF, GuardedOut, assert_exact, bad_elements, describe, exact_epilogue, exact_fp8_operand,
                        exact_operands, pow2, reference, strided)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from bind_your_avatar_implementation_amd import ops
    ops.ensure_gemm_workspace(dev)            # (split-K plans depend on it: registered before the first query)
    return ops


# (id, M, N, K, options, expected plan key, case arguments)
#   forced tiles: M one above / below a multiple of the tile height, N % 16 != 0 (N % 256 == 4 where the path admits N % 8 != 0),
#   K of 1..4 K-tiles; epilogue variants spread over them
BF16_CASES = [
    ("t0-k1", 257, 260, 64, dict(gemm_tile=0), "t128x64", {}),
    ("t0-k4-epi", 255, 260, 256, dict(gemm_tile=0), "t128x64", dict(bias=True, gates=True, gate_split=70, res="alias")),
    ("t1-k2", 129, 260, 128, dict(gemm_tile=1), "t128x128", dict(bias=True)),
    ("t1-k3-batch2", 127, 260, 192, dict(gemm_tile=1), "t128x128", dict(batch=2, gates=True, gate_split=64, res="separate")),
    ("t1-split3", 255, 264, 256, dict(gemm_tile=1), "t128x128", dict(parts=3, bias=True, lda_pad=64)),
    ("t2-k3", 257, 260, 192, dict(gemm_tile=2), "t256x128", dict(alpha=0.5, rowscale=True, bias=True)),
    ("t2-k4-batch2", 255, 132, 256, dict(gemm_tile=2), "t256x128", dict(batch=2, res="alias", bias=True)),
    ("t3-k1", 257, 516, 64, dict(gemm_tile=3), "t256x256", dict(bias=True)),
    ("t3-k4-epi", 511, 260, 256, dict(gemm_tile=3), "t256x256", dict(gates=True, gate_split=300, res="separate", alpha=2.0)),
    ("p256-k3", 257, 264, 192, dict(gemm_tile=4), "p256", dict(bias=True)),
    ("p256-k4-split3", 511, 264, 256, dict(gemm_tile=4), "p256", dict(parts=3, bias=True, lda_pad=64)),
    ("p256-batch2", 300, 264, 320, dict(gemm_tile=4), "p256", dict(batch=2, gates=True, gate_split=100, res="alias",
                                                                   rowscale=True, bias=True)),
    ("w8-misaligned-c", 257, 264, 256, dict(gemm_tile=4), "w8_256", dict(col0=4, bias=True, res="separate")),
    ("w8-k2", 255, 264, 128, dict(gemm_tile=4), "w8_256", dict(gates=True, gate_split=128)),
    ("w8-variant1", 513, 264, 256, dict(gemm_tile=4, gemm_variant=1), "w8_256", dict(bias=True, alpha=2.0)),
    ("p128-k4", 129, 264, 256, dict(gemm_tile=5), "p128", dict(bias=True, res="alias")),
    ("p128-k5-batch2", 127, 264, 320, dict(gemm_tile=5), "p128", dict(batch=2, gates=True, gate_split=16)),
    ("p128s-k4", 129, 264, 256, dict(gemm_tile=6), "p128s", dict(bias=True, rowscale=True)),
    ("p128s-split3", 383, 528, 320, dict(gemm_tile=6), "p128s", dict(parts=3, bias=True)),
    ("p128s-batch2", 255, 264, 256, dict(gemm_tile=6), "p128s", dict(batch=2, res="separate", gates=True, gate_split=200)),
    # the library's own choices at the shapes of the DiT step
    ("auto-to_out", 17776, 3072, 3072, {}, "p256|p128s", dict(bias=True, gates=True, gate_split=16384 - 5, res="alias")),
    ("auto-to_out-gate-past-m0", 17776, 3072, 3072, {}, "p256|p128s", dict(gates=True, gate_split=16384 + 5, res="separate")),
    ("auto-ff2-k12288", 17776, 3072, 12288, {}, "p256|p128s", dict(bias=True)),
    ("auto-qkv-rank", 2222, 9216, 3072, {}, "p256|p128s", dict(parts=3, bias=True)),
    ("auto-rank-to_out", 2222, 3072, 3072, {}, "p128s", dict(bias=True, gates=True, gate_split=226, res="alias")),
    ("auto-variant2", 2222, 9216, 3072, dict(gemm_variant=2), "p256", dict(bias=True)),
    ("auto-n64", 300, 64, 512, {}, "t128x64", dict(bias=True)),
    ("forced4-tail-128", 1299, 76544, 192, dict(gemm_tile=4), "p256|t128x128", dict(bias=True, rowscale=True, alpha=0.5)),
    # split-K (K ranges of at least 8 K-tiles); the cost model sends 4000 x 1536 to the 128-row tile, so the 256-row one is forced
    ("splitk1", 4000, 1536, 1024, dict(gemm_splitk=1, gemm_splitk_min=8, gemm_tile=4), "p256+splitk", dict(bias=True, gates=True, gate_split=3000, res="alias")),
    ("splitk2", 2222, 3072, 3072, dict(gemm_splitk=2, gemm_splitk_min=8, gemm_tile=4), "p256+splitk", dict(bias=True)),
]


def meta_case(M, N, K, batch=1, bias=False, gates=False, gate_split=0, res=None, alpha=1.0, rowscale=False, parts=1, col0=8,
              lda_pad=0):
    """The arguments of a BF16_CASES case on the meta device (same shapes, strides and view offsets as ``build_case``'s):
    for the plan queries without a GPU."""
    def m(*shape, dtype=BF):
        return torch.empty(*shape, dtype=dtype, device="meta")
    a = strided(m(batch, M, K) if batch > 1 else m(M, K), lda_pad)
    out = GuardedOut(M, N, "meta", batch=batch, parts=parts, col0=col0)
    res_t = None if not res else (out.view() if res == "alias" else m(*out.view().shape))
    return dict(a=a, w=m(N, K), out=out.view(), bias=m(N) if bias else None, res=res_t, gate0=m(N) if gates else None,
                gate1=m(N) if gates else None, gate_split=gate_split, split=out.split,
                bias_rowscale=m(batch * M, dtype=torch.float32) if rowscale else None, alpha=alpha)


def build_case(ops, dev, M, N, K, batch=1, bias=False, gates=False, gate_split=0, res=None, alpha=1.0, rowscale=False,
               parts=1, col0=8, lda_pad=0, seed=None):
    """-> (args for ops.gemm / gemm_plan as a dict with a, w, out; the GuardedOut; the fp64 reference)."""
    seed = (M * 131 + N * 7 + K) % 100003 if seed is None else seed
    a, w = exact_operands(M, N, K, dev, seed, batch)
    a = strided(a, lda_pad)                                          # A as a strided view (lda = K + lda_pad)
    ep = exact_epilogue(w, dev, seed + 11, bias=bias, gates=gates, alpha=alpha, res_rows=M if res else None, batch=batch)
    rs = pow2((batch * M,), dev, seed + 23) if rowscale else None
    out = GuardedOut(M, N, dev, batch=batch, parts=parts, col0=col0)
    res_t = res_v = None
    if res:
        res_v = ep["res"] if batch > 1 else ep["res"][0]
        if res == "alias":                                           # x += ...: the residual IS the output
            out.fill(res_v)
            res_t = out.view()
        else:
            res_t = res_v.to(BF)
    args = dict(a=a, w=w, out=out.view(), bias=ep["bias"], res=res_t, gate0=ep["gate0"], gate1=ep["gate1"], gate_split=gate_split,
                split=out.split, bias_rowscale=rs, alpha=alpha)
    ref = reference(a, w, ep["bias"], ep["gate0"], ep["gate1"], gate_split, None if res_v is None else res_v.to(BF), rs, alpha)
    return args, out, ref


def _call(fn, args):
    kw = dict(args)
    return fn(kw.pop("a"), kw.pop("w"), kw.pop("out"), **kw)


@pytest.mark.parametrize("cid,M,N,K,opts,expect,kw", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_bf16_exact(ops, dev, cid, M, N, K, opts, expect, kw):
    args, out, ref = build_case(ops, dev, M, N, K, **kw)
    with ops.options(**opts):
        plan = _call(ops.gemm_plan, args)
        assert ops.plan_key(plan) == expect, plan
        _call(ops.gemm, args)
    torch.cuda.synchronize()
    assert_exact(out.gathered(), ref, plan, f"{cid} {M}x{N}x{K}")
    assert out.guard_intact(), f"{cid}: a write outside the output view"
    assert ops.gemm_workspace_status() == 0
    print(f"{cid}: {M}x{N}x{K} on {ops.plan_key(plan)} bit-exact")


SKINNY_CASES = [(1, 1), (1, 15), (1, 17), (1, 64), (2, 15), (2, 64)]


@pytest.mark.parametrize("B,M", SKINNY_CASES)
def test_skinny_exact(ops, dev, B, M):
    """The weight-streaming kernel (ops.weight_streaming): M of 1 / 15 / 17 / 64, batch entries stacked (2 x 15 rows) or not
    (2 x 64)."""
    N, K = 272, 512
    args, out, ref = build_case(ops, dev, M, N, K, batch=B, bias=True, res="separate", alpha=2.0)
    with ops.weight_streaming():
        plan = _call(ops.gemm_plan, args)
        assert plan["path"] == "skinny", plan
        _call(ops.gemm, args)
    torch.cuda.synchronize()
    assert_exact(out.gathered(), ref, plan, f"skinny {B}x{M}x{N}x{K}")
    assert out.guard_intact()


# bya_rowgemm512 takes its W-stationary kernel for N = 512, 2048 <= M <= 65536 and no LayerNorm, unless the reference form
# "rowgemm_chunked" is set; everything else runs the chunk-balanced kernel.  (Its nsplit argument is ignored by the library.)
ROWGEMM_CASES = [
    (2049, 512, False, "w_stationary"),
    (4133, 512, False, "w_stationary"),
    (2049, 512, True, "chunk_balanced"),       # the same shape on the other kernel (reference form)
    (4133, 512, True, "chunk_balanced"),
    (1000, 512, False, "chunk_balanced"),      # M < 2048
    (127, 1536, False, "chunk_balanced"),      # N != 512
]


@pytest.mark.parametrize("M,N,chunked,kernel", ROWGEMM_CASES)
def test_rowgemm512_without_layernorm_exact(ops, dev, M, N, chunked, kernel):
    """bya_rowgemm512 without its LayerNorm prologue (out = res + x @ W.T + b), the residual aliasing the output: both kernels."""
    a, w = exact_operands(M, N, 512, dev, seed=M + N)
    ep = exact_epilogue(w, dev, M, bias=True, res_rows=M)
    res_v = ep["res"][0]
    out = GuardedOut(M, N, dev, col0=8)
    out.fill(res_v)
    pack = ops.pack_rowgemm512(w, ep["bias"])
    with ops.options(reference_forms=["rowgemm_chunked"] if chunked else []):
        ops.rowgemm512(a, pack, out.view(), res=out.view())
    torch.cuda.synchronize()
    assert_exact(out.gathered(), reference(a, w, ep["bias"], res=res_v.to(BF)), kernel, f"rowgemm512 {M}x{N}")
    assert out.guard_intact()


FP8_CASES = [
    (1, 1000, 3072, 512, dict(fp8_kernel=1), "t128x128"),
    (2, 129, 260, 1024, {}, "t128x128"),
    (1, 3621, 3848, 512, {}, "p256"),
    (2, 1811, 3848, 512, {}, "p256"),
]


@pytest.mark.parametrize("B,M,N,K,opts,expect", FP8_CASES)
def test_fp8_exact(ops, dev, B, M, N, K, opts, expect):
    """bya_gemm_fp8 on e4m3 codes of exact values with power-of-two row / channel scales: both kernels."""
    a8, sa, da = exact_fp8_operand(B * M, K, dev, seed=M + K)
    w8, sw, dw = exact_fp8_operand(N, K, dev, seed=N)
    ep = exact_epilogue(w8, dev, N, bias=True, gates=True, res_rows=M, batch=B)
    res_v = ep["res"] if B > 1 else ep["res"][0]
    out = GuardedOut(M, N, dev, batch=B)
    out.fill(res_v)
    a8 = a8.reshape(B, M, K) if B > 1 else a8
    kw = dict(bias=ep["bias"], res=out.view(), gate0=ep["gate0"], gate1=ep["gate1"], gate_split=M // 3)
    with ops.options(**opts):
        plan = ops.gemm_fp8_plan(a8, sa, w8, sw, out.view(), **kw)
        assert plan["path"] == expect, plan
        ops.gemm_fp8(a8, sa, w8, sw, out.view(), **kw)
    torch.cuda.synchronize()
    da = da.reshape(B, M, K) if B > 1 else da
    assert_exact(out.gathered(), reference(da, dw, ep["bias"], ep["gate0"], ep["gate1"], M // 3, res_v.to(BF)), plan,
                 f"fp8 {B}x{M}x{N}x{K}")
    assert out.guard_intact()


MX_CASES = [
    ("mxfp8", 1, 255, 260, 256, "t128x128"),
    ("mxfp8", 2, 3621, 3844, 256, "t128x128"),
    ("mxfp6", 1, 257, 260, 384, "t128x128"),
    ("mxfp6", 2, 3621, 3844, 256, "t256x256"),             # the e2m3 256 x 256 tile: ragged M and N, batch 2
    ("mxfp6", 1, 3621, 3844, 512, "t256x256"),
]


@pytest.mark.parametrize("fmt,B,M,N,K,expect", MX_CASES)
def test_mx_exact(ops, dev, fmt, B, M, N, K, expect):
    from test_mx_cpu import dequant_mx
    from test_mx_gpu import exact_operand
    ac, asc = exact_operand(B * M, K, fmt, seed=M + K)
    wc, wsc = exact_operand(N, K, fmt, seed=N + 1)
    da, dw = dequant_mx(ac, asc, fmt).to(dev), dequant_mx(wc, wsc, fmt).to(dev)
    w_bf = torch.zeros(N, 1, device=dev)
    ep = exact_epilogue(w_bf, dev, N, bias=True, gates=True, res_rows=M, batch=B)
    res_v = ep["res"] if B > 1 else ep["res"][0]
    out = GuardedOut(M, N, dev, batch=B)
    out.fill(res_v)
    asc = asc.reshape(B, M, K // 32) if B > 1 else asc
    args = (ac.reshape(-1).to(dev), asc.to(dev), wc.to(dev), wsc.to(dev), out.view(), fmt)
    kw = dict(bias=ep["bias"], res=out.view(), gate0=ep["gate0"], gate1=ep["gate1"], gate_split=M // 2)
    plan = ops.gemm_mx_plan(*args, **kw)
    assert plan["path"] == expect, plan
    ops.gemm_mx(*args, **kw)
    torch.cuda.synchronize()
    da = da.reshape(B, M, K) if B > 1 else da
    assert_exact(out.gathered(), reference(da, dw, ep["bias"], ep["gate0"], ep["gate1"], M // 2, res_v.to(BF)), plan,
                 f"{fmt} {B}x{M}x{N}x{K}")
    assert out.guard_intact()


QKN_CASES = [
    (1, 300, 1152, 256, 40, {}, "p128"),                    # plan 1
    (2, 826, 9216, 3072, 226, {}, "p128"),
    (1, 2222, 9216, 3072, 226, {}, "p256|p128"),            # plan 2, text rows before m0 = 1792
    (1, 2222, 9216, 3072, 2000, {}, "p256|p128"),           # ... and past it (the second launch starts inside the text rows)
    (1, 1000, 1152, 512, 226, dict(gemm_tile=4), "p256"),   # plan 0
]


@pytest.mark.parametrize("B,M,N,K,text,opts,expect", QKN_CASES)
def test_qkv_norm_rope_plans_bit_identical_to_the_unfused_pair(ops, dev, B, M, N, K, text, opts, expect):
    """bya_gemm_qkv_norm_rope's epilogue has a LayerNorm: not exact, but it must equal bya_gemm_bf16 + bya_qknorm_rope BIT FOR
    BIT on every row plan -- here the shapes the plan query puts on plans 1 and 2 (text_rows on either side of m0)."""
    width = N // 3
    x, w = exact_operands(M, N, K, dev, seed=M, batch=B)
    g = torch.Generator(device=dev).manual_seed(M)
    bias = (torch.randn(N, generator=g, device=dev) * 0.5).to(BF)
    qw, qb, kw, kb = ((torch.randn(64, generator=g, device=dev) * 0.3 + (1 if i % 2 == 0 else 0)).to(BF) for i in range(4))
    ang = torch.rand(M - text, 64, generator=g, device=dev) * 6.3
    cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    heads = width // 64
    two = torch.zeros(3, B, M, width, dtype=BF, device=dev)
    one = torch.full_like(two, float("nan"))
    o2, o1 = (two[0], one[0]) if B > 1 else (two[0, 0], one[0, 0])
    split = (width, B * M * width)
    ops.gemm(x, w, o2, bias=bias, split=split)
    ops.qknorm_rope(two[0], two[1], qw, qb, kw, kb, cos, sin, heads=heads, text_rows=text, eps=1e-6, k_scale=0.18)
    with ops.options(**opts):
        plan = ops.gemm_qkv_norm_rope_plan(x, w, o1, bias, split, qw, qb, kw, kb, cos, sin, text, eps=1e-6, k_scale=0.18)
        assert ops.plan_key(plan) == expect, plan
        assert ops.gemm_qkv_norm_rope(x, w, o1, bias, split, qw, qb, kw, kb, cos, sin, text, eps=1e-6, k_scale=0.18)
    torch.cuda.synchronize()
    bad = bad_elements(one, two)
    assert not bool(bad.any()), f"qkn {expect}: {describe(bad.reshape(-1, width), one.reshape(-1, width), two.reshape(-1, width))}"


ACT_REF = {"gelu_tanh": lambda y: F.gelu(y, approximate="tanh"), "gelu_erf": F.gelu, "relu": F.relu, "silu": F.silu,
           "leaky_relu": lambda y: F.leaky_relu(y, 0.01)}
# worst error in bf16 ulps (results below 2^-6: in ulps of 2^-6), measured 1 / 0.125 / 0 / 0 / 0: GELU(tanh) in fp32 lands on
# the other side of a bf16 rounding tie (pre-activation 4.984375, on the exact grid, is one)
ACT_ULPS = {"gelu_tanh": 1, "gelu_erf": 0.25, "relu": 0, "silu": 0, "leaky_relu": 0}


@pytest.mark.parametrize("act,tile,expect", [("gelu_tanh", 1, "t128x128"), ("gelu_erf", 1, "t128x128"), ("relu", 1, "t128x128"),
                                             ("silu", 1, "t128x128"), ("leaky_relu", 1, "t128x128"), ("gelu_tanh", 4, "p256"),
                                             ("gelu_tanh", 6, "p128s")])
def test_activation_of_the_exact_pre_activation(ops, dev, act, tile, expect):
    """Activations are not exact: the kernel's act(pre-activation) against the fp64 activation of the EXACT pre-activation,
    element by element, within ``ACT_ULPS`` bf16 ulps (relu / leaky_relu: exact)."""
    M, N, K = 515, 264, 512
    a, w = exact_operands(M, N, K, dev, seed=7)
    a = (a.float() * 2 ** -7).to(BF)                      # pre-activations of order 1, where the curves bend
    ep = exact_epilogue(w, dev, 3, bias=True)
    out = GuardedOut(M, N, dev)
    with ops.options(gemm_tile=tile):
        plan = ops.gemm_plan(a, w, out.view(), bias=ep["bias"], act=act)
        assert plan["path"] == expect, plan
        ops.gemm(a, w, out.view(), bias=ep["bias"], act=act)
    torch.cuda.synchronize()
    pre = reference(a, w, ep["bias"])
    want = ACT_REF[act](pre).to(BF)
    got = out.gathered().double()
    # error in bf16 ulps of the exact result; results below 2^-6 (the flat tails of GELU / SiLU, where fp32 1 + tanh(u) cancels)
    # count in ulps of 2^-6
    mag = want.double().abs().clamp_min(2.0 ** -6)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    err = (got - want.double()).abs() / ulp
    worst = int(err.flatten().argmax())
    ulps = float(err.max())
    print(f"{act} on {expect}: worst {ulps:.3f} bf16 ulp(s) from the activation of the exact pre-activation "
          f"(at pre-activation {float(pre.flatten()[worst]):.4g}: got {float(got.flatten()[worst]):.6g}, want {float(want.flatten()[worst]):.6g})")
    assert ulps <= ACT_ULPS[act], (act, ulps)
    assert out.guard_intact()

