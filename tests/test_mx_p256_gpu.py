"""The persistent one-wave-per-SIMD 256 x 256 MX GEMM (csrc/gemm_mx_v4.hip; option mx_kernel) for mxfp8 activations and
weights: exact data against the fp64 product, bit for bit against the 128 x 128 kernel of csrc/gemm_mx.hip on the same
bytes (plain and quantising epilogue), and the engine's step with enable_mx_weights(persistent_gemm=...).  The plan is
asserted before every launch."""
import pytest
import torch

from exact_gemm import GuardedOut, assert_exact, exact_epilogue, reference
from test_mx_cpu import dequant_mx
from test_mx_gpu import exact_operand

pytestmark = pytest.mark.gpu
FMT = "mxfp8"


def exact_pair(rows, K, dev, seed, batch=1):
    """(codes, scales) on the device and the dequantised fp64 values, [(batch,) rows, ..]."""
    c, s = exact_operand(batch * rows, K, FMT, seed)
    v = dequant_mx(c, s, FMT)
    lead = (batch, rows) if batch > 1 else (rows,)
    return c.reshape(*lead, -1).to(dev), s.reshape(*lead, -1).to(dev), v.reshape(*lead, -1).to(dev)


@pytest.mark.parametrize("B,M,N,K,opt", [
    (1, 3621, 3848, 512, 1),        # 240 tiles, ragged M and N; the shortest K: each K-tile variant A / B / C / D once
    (2, 1811, 3848, 640, 1),        # odd K-tile count, batch
    (1, 300, 264, 512, 2),          # four tiles: most workgroups have none
    (1, 1, 8, 1024, 2),             # one tile
])
def test_p256_exact_data_with_the_whole_epilogue(dev, B, M, N, K, opt):
    """Elements in {0, +-0.5 .. +-3} under block scales 2^-2 .. 2^2 (test_mx_gpu.exact_operand): every product is a multiple of
    2^-6 below 2^8 and every partial sum exact in fp32, as is the epilogue on the grid of exact_gemm.exact_epilogue -- the one
    rounding is the final one to bf16, so the result EQUALS the fp64 reference rounded to bf16.  Scales differ between rows,
    between the blocks of a K-tile and between K-tiles."""
    from bind_your_avatar_implementation_amd import ops
    ac, asc, a = exact_pair(M, K, dev, seed=M + K, batch=B)
    wc, wsc, w = exact_pair(N, K, dev, seed=N + K + 1)
    split = M // 3
    epi = exact_epilogue(w, dev, seed=7, bias=True, gates=True, res_rows=M, batch=B)
    out = GuardedOut(M, N, dev, batch=B)
    res = epi["res"] if B > 1 else epi["res"][0]
    out.fill(res)
    ref = reference(a, w, epi["bias"], epi["gate0"], epi["gate1"], split, out.gathered().clone())
    kw = dict(fmt=FMT, bias=epi["bias"], res=out.view(), gate0=epi["gate0"], gate1=epi["gate1"], gate_split=split)
    with ops.options(mx_kernel=opt):
        plan = ops.gemm_mx_plan(ac, asc, wc, wsc, out.view(), **kw)
        assert plan["path"] == "p256", plan
        ops.gemm_mx(ac, asc, wc, wsc, out.view(), **kw)
    assert_exact(out.gathered(), ref, plan, f"{B}x{M}x{N}x{K}")
    assert out.guard_intact()


def test_p256_operand_and_scale_map(dev):
    """The construction of test_gemm_mx_operand_map_on_exact_data at 3621 x 3848 x 768 on the persistent kernel: a stale ring
    stage, a wrong byte of the scale dword or a W scale row that missed the slot map each change the answer."""
    from bind_your_avatar_implementation_amd import ops
    M, N, K = 3621, 3848, 768
    ac, asc, a = exact_pair(M, K, dev, seed=M)
    wc, wsc, w = exact_pair(N, K, dev, seed=N + 1)
    for sc, rows in ((asc, M), (wsc, N)):           # scales differ between K-tiles, between the blocks of a K-tile, between rows
        s = sc.view(rows, K // 128, 4).long()
        assert bool((s[:, 1:] != s[:, :-1]).any()) and bool((s[..., 1:] != s[..., :-1]).any()) and bool((s[1:] != s[:-1]).any())
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    with ops.options(mx_kernel=1):
        plan = ops.gemm_mx_plan(ac, asc, wc, wsc, out, fmt=FMT)
        assert plan["path"] == "p256", plan
        ops.gemm_mx(ac, asc, wc, wsc, out, fmt=FMT)
    assert_exact(out, a @ w.T, plan, "operand map")


def spread_operand(rows, K, dev, seed):
    """Quantised gaussian rows whose blocks spread over 20 binades, with all-zero blocks: (codes, scales) on the device (by the
    device quantiser, which test_mx_gpu.py holds to the definition byte for byte)."""
    from bind_your_avatar_implementation_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K // 32, 32, generator=g) * torch.exp2(torch.randint(-10, 11, (rows, K // 32, 1), generator=g).float())
    x[torch.rand(rows, K // 32, generator=g) < 0.02] = 0.0
    return ops.quantize_mx(x.reshape(rows, K).to(torch.bfloat16).to(dev), FMT)


_SPREAD = {}


def spread(rows, K, dev, seed):
    key = (rows, K, seed)
    if key not in _SPREAD:
        _SPREAD[key] = spread_operand(rows, K, dev, seed)
    return _SPREAD[key]


@pytest.mark.parametrize("case", ["k3072", "k12288", "qkv_split", "batch"])
def test_p256_equals_the_128_tile_kernel_bit_for_bit(dev, case):
    from bind_your_avatar_implementation_amd import ops
    B, M, N, K, parts = {"k3072": (1, 3621, 3848, 3072, 1), "k12288": (1, 3621, 3848, 12288, 1),
                         "qkv_split": (1, 3621, 3840, 3072, 3), "batch": (2, 1811, 3848, 1024, 1)}[case]
    ac, asc = spread(B * M, K, dev, 1)
    wc, wsc = spread(N, K, dev, 2)
    if B > 1:
        ac, asc = ac.view(B, M, -1), asc.view(B, M, -1)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(3)) * 4).to(torch.bfloat16).to(dev)
    got = {}
    for opt, want in ((0, "t128x128"), (1, "p256")):
        out = GuardedOut(M, N, dev, batch=B, parts=parts)
        with ops.options(mx_kernel=opt):
            plan = ops.gemm_mx_plan(ac, asc, wc, wsc, out.view(), fmt=FMT, bias=bias, split=out.split)
            assert plan["path"] == want, plan
            ops.gemm_mx(ac, asc, wc, wsc, out.view(), fmt=FMT, bias=bias, split=out.split)
        assert out.guard_intact()
        got[opt] = out.gathered()
    assert not bool(torch.isnan(got[0].float()).any())
    assert torch.equal(got[0].view(torch.int16), got[1].view(torch.int16))


@pytest.mark.parametrize("M,N,K,opt", [(3621, 3840, 512, 1), (300, 256, 512, 2)])
@pytest.mark.parametrize("epi", [False, True])
def test_p256_quantising_epilogue_writes_the_128_tile_kernels_bytes(dev, M, N, K, opt, epi):
    from bind_your_avatar_implementation_amd import ops
    ac, asc = spread(M, K, dev, 4)
    wc, wsc = spread(N, K, dev, 5)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(6)) * 4).to(torch.bfloat16).to(dev) if epi else None
    act = "gelu_tanh" if epi else None
    PADR = 3                                # canary rows behind the M rows; codes and scales are contiguous [M, N] / [M, N / 32]
    got = {}
    for o, want in ((0, "t128x128"), (opt, "p256")):
        codes = torch.full((M + PADR, N), 0xA5, dtype=torch.uint8, device=dev)
        scales = torch.full((M + PADR, N // 32), 0xA5, dtype=torch.uint8, device=dev)
        with ops.options(mx_kernel=o):
            plan = ops.gemm_mx_quant_plan(ac, asc, wc, wsc, codes[:M], scales[:M], fmt=FMT, out_fmt=FMT, bias=bias, act=act)
            assert plan["path"] == want, plan
            ops.gemm_mx_quant(ac, asc, wc, wsc, codes[:M], scales[:M], fmt=FMT, out_fmt=FMT, bias=bias, act=act)
        assert bool((codes[M:] == 0xA5).all()) and bool((scales[M:] == 0xA5).all())
        got[o] = (codes[:M].clone(), scales[:M].clone())
    assert torch.equal(got[0][0], got[opt][0]) and torch.equal(got[0][1], got[opt][1])
    # ... and so the two launches' bytes (checked once), and the pair feeds a following GEMM
    if epi and M == 300:
        y = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac, asc, wc, wsc, y, fmt=FMT, bias=bias, act=act)
        c2, s2 = ops.quantize_mx(y, FMT)
        assert torch.equal(c2, got[opt][0]) and torch.equal(s2, got[opt][1])
        w2c, w2s = spread(264, N, dev, 8)
        z = {}
        for o in (0, 2):
            z[o] = torch.full((M, 264), float("nan"), dtype=torch.bfloat16, device=dev)
            with ops.options(mx_kernel=o):
                ops.gemm_mx(*got[opt], w2c, w2s, z[o], fmt=FMT)
        assert torch.equal(z[0].view(torch.int16), z[2].view(torch.int16)) and not bool(torch.isnan(z[0].float()).any())


def test_p256_quant_row_stride_padding_is_left_alone(dev):
    """Codes in a buffer whose row stride is wider than N: the padding keeps its canary bytes (ldc comes from the wrapper as
    the dense row, so the strided form goes through the C ABI)."""
    import ctypes
    from bind_your_avatar_implementation_amd import _hip, ops
    M, N, K, LD = 300, 256, 512, 256 + 64
    ac, asc = spread(M, K, dev, 4)
    wc, wsc = spread(N, K, dev, 5)
    d = ops._mx_quant_desc(ac, asc, wc, wsc, torch.empty(M, N, dtype=torch.uint8, device=dev),
                           torch.empty(M, N // 32, dtype=torch.uint8, device=dev), FMT, None, FMT, None, 1.0)
    d.ldc = LD
    lib = _hip.load()
    got = {}
    for o, want in ((0, 1), (2, 4)):
        codes = torch.full((M + 2, LD), 0xA5, dtype=torch.uint8, device=dev)
        scales = torch.full((M + 2, N // 32), 0xA5, dtype=torch.uint8, device=dev)
        args = (ac.data_ptr(), asc.data_ptr(), wc.data_ptr(), wsc.data_ptr(), None, codes.data_ptr(), scales.data_ptr(), ctypes.byref(d), 0, 0, 0)
        with ops.options(mx_kernel=o):
            p = _hip.GemmPlan()
            assert lib.bya_gemm_mx_quant_plan(*args, ctypes.byref(p)) == 0 and p.path == want
            assert lib.bya_gemm_mx_quant(*args, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert bool((codes[:, N:] == 0xA5).all()) and bool((codes[M:] == 0xA5).all()) and bool((scales[M:] == 0xA5).all())
        got[o] = (codes, scales)
    assert torch.equal(got[0][0], got[2][0]) and torch.equal(got[0][1], got[2][1])


class Recorder:
    """Wraps an ops launch: asks the matching plan query with the launch's own arguments (inside the engine's option block)."""

    def __init__(self, fn, plan_fn):
        self.fn, self.plan_fn, self.paths = fn, plan_fn, []

    def __call__(self, *a, **kw):
        self.paths.append(self.plan_fn(*a, **kw)["path"])
        return self.fn(*a, **kw)


def recorded_forward(model, gi, monkeypatch):
    from bind_your_avatar_implementation_amd import ops
    model(**gi)                                                                           # builds the engine (packs weights)
    with monkeypatch.context() as mp:
        g, q = Recorder(ops.gemm_mx, ops.gemm_mx_plan), Recorder(ops.gemm_mx_quant, ops.gemm_mx_quant_plan)
        mp.setattr(ops, "gemm_mx", g)
        mp.setattr(ops, "gemm_mx_quant", q)
        out = model(**gi)[0].clone()
    return out, g.paths, q.paths


def test_engine_step_on_the_persistent_kernel_keeps_its_bits(dev, monkeypatch):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    model.enable_mx_weights("mxfp8")
    off, g_off, q_off = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_kernel == 0 and set(g_off + q_off) == {"t128x128"}
    model.enable_mx_weights("mxfp8", persistent_gemm="always")
    assert model._engine is None                                                          # the switch invalidates the engine
    on, g_on, q_on = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_kernel == 2
    print(f"gemm_mx paths {g_on}, gemm_mx_quant paths {q_on}")
    # qkv, out, ff2 per block through gemm_mx, ff1 through the quantising launch: all on the persistent kernel
    assert len(g_on) == 3 * blocks and len(q_on) == blocks and set(g_on + q_on) == {"p256"}
    assert torch.equal(on, off)
    # graph replay of the step: bit for bit the eager result
    model.use_hip_graph = True
    try:
        model(**gi)                                                                       # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], off)
    finally:
        model.use_hip_graph = False
        model._graphs = {}
    # together with the attention writing to_out's operand
    model.enable_mx_weights("mxfp8", persistent_gemm="always", fuse_attention_quant=True)
    both, g_b, q_b = recorded_forward(model, gi, monkeypatch)
    assert len(g_b) == 3 * blocks and len(q_b) == blocks and set(g_b + q_b) == {"p256"}
    assert torch.equal(both, off)
    model.use_hip_graph = True
    try:
        model(**gi)                                                                       # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], off)
    finally:
        model.use_hip_graph = False
        model._graphs = {}
    # mxfp6: the switch changes no launch
    model.enable_mx_weights("mxfp6")
    ref6, g6, q6 = recorded_forward(model, gi, monkeypatch)
    model.enable_mx_weights("mxfp6", persistent_gemm="always")
    got6, g6p, q6p = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_kernel == 0 and (g6p, q6p) == (g6, q6) and "p256" not in g6p + q6p
    assert torch.equal(got6, ref6)
