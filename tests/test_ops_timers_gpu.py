"""The per-entry-point timers of the GEMM front end (ops.enable_kernel_timers / collect_kernel_timers / kernel_timer_flops; what
bench.py's rooflines are read from): one launch of every GEMM wrapper at a tiny shape, and two that the library declines.  The
bucket names, the launches per bucket, the FLOPs per bucket and -- ``by_shape=True`` -- the shape labels are written out here;
a declined launch leaves no bucket and counts no FLOPs.  The bf16 q/k-norm wrapper takes no shape label: it counts under the
bare name of the bf16 GEMM's bucket."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, K, WIDTH, BIG_M = 128, 384, 256, 128, 1024
FLOPS, BIG_FLOPS = 2.0 * M * N * K, 2.0 * BIG_M * N * K
DECLINED_WIDTH = 96                                                      # no whole heads: tests/test_mx_qkn_cpu.py


@pytest.fixture(scope="module")
def operands(dev):
    """Everything the launches read, built (and quantised) before any timer runs."""
    from bind_your_avatar_implementation_amd import ops
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).to(torch.bfloat16).to(dev)
    a, big, w, w96 = rnd(M, K), rnd(BIG_M, K), rnd(N, K, std=K ** -0.5), rnd(3 * DECLINED_WIDTH, K, std=K ** -0.5)
    o = dict(a=a, big=big, w=w, bias=rnd(N), res=rnd(BIG_M, N), gate=rnd(N), norm=[rnd(64) + 1, rnd(64), rnd(64) + 1, rnd(64)],
             cos=torch.rand(M, 64, generator=g).to(dev), sin=torch.rand(M, 64, generator=g).to(dev),
             a8=ops.quantize_rows_fp8(a), w8=ops.quantize_rows_fp8(w))
    for fmt in ("mxfp6", "mxfp8"):
        o["a", fmt], o["w", fmt], o["w96", fmt] = ops.quantize_mx(a, fmt), ops.quantize_mx(w, fmt), ops.quantize_mx(w96, fmt)
    o["w", "mxfp4"] = ops.quantize_mx(w, "mxfp4")
    torch.cuda.synchronize()
    return o


def launch_everything(o, dev):
    """One accepted launch per wrapper (two of ``gemm``: under and at 1024 rows; three of ``gemm_mx_call``: its three epilogues),
    then the declined ones.  -> what the declined ones returned."""
    from bind_your_avatar_implementation_amd import ops
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device=dev)
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)
    split, norm = (WIDTH, M * WIDTH), (*o["norm"], o["cos"], o["sin"], 0)
    ops.gemm(o["a"], o["w"], bf(M, N))
    ops.gemm(o["big"], o["w"], bf(BIG_M, N), bias=o["bias"], res=o["res"], gate0=o["gate"], act="gelu_tanh")
    ops.gemm_fp8(*o["a8"], *o["w8"], bf(M, N), res=o["res"][:M])
    ops.gemm_mx(*o["a", "mxfp6"], *o["w", "mxfp6"], bf(M, N), "mxfp6", gate0=o["gate"])
    ops.gemm_mx(*o["a", "mxfp8"], *o["w", "mxfp4"], bf(M, N), "mxfp8", w_fmt="mxfp4", bias=o["bias"], act="gelu_tanh")
    ops.gemm_mx_quant(*o["a", "mxfp6"], *o["w", "mxfp6"], u8(M, N * 6 // 8), u8(M, N // 32), "mxfp6", bias=o["bias"], act="gelu_tanh")
    assert ops.gemm_qkv_norm_rope(o["a"], o["w"], bf(3, M, WIDTH)[0], o["bias"], split, *norm) is True
    assert ops.gemm_fp8_qkv_norm_rope(*o["a8"], *o["w8"], bf(3, M, WIDTH)[0], o["bias"], split, *norm) is True
    assert ops.gemm_mx_qkv_norm_rope(*o["a", "mxfp6"], *o["w", "mxfp6"], bf(3, M, WIDTH)[0], o["bias"], split, *norm, fmt="mxfp6",
                                     kernel=0) is True
    call = lambda *a, **kw: ops.gemm_mx_call(*o["a", "mxfp8"], *a, 0, "mxfp8", **kw)
    out = bf(M, N)
    assert call(*o["w", "mxfp8"], out, res=o["res"][:M]) is out
    oc, osc = u8(M, N), u8(M, N // 32)
    got = call(*o["w", "mxfp8"], oc, out_scales=osc, act="gelu_tanh")
    assert got[0] is oc and got[1] is osc
    qkn = dict(zip(("qw", "qb", "kw", "kb", "cos", "sin", "text_rows"), norm))
    assert call(*o["w", "mxfp8"], bf(3, M, WIDTH)[0], split=split, norm=qkn) is True
    # declined: width 96 holds no whole heads (the matching plan queries answer None)
    split96 = (DECLINED_WIDTH, M * DECLINED_WIDTH)
    args = (*o["a", "mxfp8"], *o["w96", "mxfp8"], bf(3, M, DECLINED_WIDTH)[0])
    assert ops.gemm_mx_qkv_norm_rope_plan(*args, None, split96, *norm, fmt="mxfp8") is None
    assert ops.gemm_mx_call_plan(*args, 0, "mxfp8", split=split96, norm=qkn) is None
    declined = [ops.gemm_mx_qkv_norm_rope(*args, None, split96, *norm, fmt="mxfp8", kernel=0),
                ops.gemm_mx_call(*args, 0, "mxfp8", split=split96, norm=qkn)]
    torch.cuda.synchronize()
    return declined


def run(o, dev, by_shape):
    from bind_your_avatar_implementation_amd import ops
    ops.enable_kernel_timers(by_shape=by_shape)
    try:
        declined = launch_everything(o, dev)
        flops = ops.kernel_timer_flops()
        timers = ops.collect_kernel_timers()
    finally:
        ops.enable_kernel_timers()                                       # (shape labels off again)
        ops.collect_kernel_timers()                                      # ... and the timers
    assert declined == [False, False]
    assert all(t >= 0.0 for v in timers.values() for t in v)
    return {k: len(v) for k, v in timers.items()}, {k: v for k, v in flops.items() if v}, flops


def test_buckets_launches_and_flops_per_entry_point(dev, operands):
    launches, flops, _ = run(operands, dev, by_shape=False)
    assert launches == {"bya_gemm_bf16_small_m": 2,                      # gemm under 1024 rows + the bf16 q/k-norm launch
                        "bya_gemm_bf16": 1, "bya_gemm_fp8": 1, "bya_gemm_mx": 1, "bya_gemm_mx_mixed": 1, "bya_gemm_mx_quant": 1,
                        "bya_gemm_fp8_qkv_norm_rope": 1, "bya_gemm_mx_qkv_norm_rope": 1, "bya_gemm_mx_call": 3}
    assert flops == {"bya_gemm_bf16_small_m": 2 * FLOPS, "bya_gemm_bf16": BIG_FLOPS, "bya_gemm_fp8": FLOPS, "bya_gemm_mx": FLOPS,
                     "bya_gemm_mx_mixed": FLOPS, "bya_gemm_mx_quant": FLOPS, "bya_gemm_fp8_qkv_norm_rope": FLOPS,
                     "bya_gemm_mx_qkv_norm_rope": FLOPS, "bya_gemm_mx_call": 3 * FLOPS}


def test_shape_labels(dev, operands):
    launches, flops, all_flops = run(operands, dev, by_shape=True)
    dims = f"1x{M}x{N}x{K}"
    want = {"bya_gemm_bf16_small_m:" + dims + ":none": FLOPS,
            f"bya_gemm_bf16:1x{BIG_M}x{N}x{K}:gelu_tanh+gate+res": BIG_FLOPS,
            "bya_gemm_fp8:" + dims + ":none+res": FLOPS,
            "bya_gemm_mx:mxfp6:" + dims + ":none+gate": FLOPS,
            "bya_gemm_mx_mixed:mxfp8*mxfp4:" + dims + ":gelu_tanh": FLOPS,
            "bya_gemm_mx_quant:mxfp6*mxfp6>mxfp6:" + dims + ":gelu_tanh": FLOPS,
            "bya_gemm_bf16_small_m": FLOPS,                                                # the bf16 q/k-norm launch: no label
            "bya_gemm_fp8_qkv_norm_rope:" + dims: FLOPS,
            "bya_gemm_mx_qkv_norm_rope:mxfp6*mxfp6:" + dims: FLOPS,
            "bya_gemm_mx_call:bf16:k0:mxfp8*mxfp8:" + dims + ":none": FLOPS,
            "bya_gemm_mx_call:quant:k0:mxfp8*mxfp8:" + dims + ":gelu_tanh": FLOPS,
            "bya_gemm_mx_call:qkn:k0:mxfp8*mxfp8:" + dims + ":none": FLOPS}
    assert launches == {k: 1 for k in want}
    assert flops == want
    # the declined launches: no bucket, no FLOPs under their own labels
    d96 = f"1x{M}x{3 * DECLINED_WIDTH}x{K}"
    for label in ("bya_gemm_mx_qkv_norm_rope:mxfp8*mxfp8:" + d96, "bya_gemm_mx_call:qkn:k0:mxfp8*mxfp8:" + d96 + ":none"):
        assert label not in launches and all_flops.get(label, 0.0) == 0.0
