"""CPU side of tests/test_fp8_exact_gpu.py: the exactness argument of tests/exact_gemm.py for the fp8 product through the whole
epilogue, confirmed in fp32 at K = 12288; the GPU case tables planned on meta tensors of the same shapes, strides and view
offsets (every case reaches the path, the fallback or the refusal it names, without a GPU); and why an exact comparator: a
planted fault on fp8 data that a relative-Frobenius bar of 1e-3 passes."""
import math

import pytest
import torch

from conftest import rel_fro
from exact_gemm import BF, assert_exact, bad_elements, exact_fp8_epilogue, exact_fp8_operand, pow2, reference


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import build
    build.build_hip_library()
    from bind_your_avatar_implementation_amd import ops
    return ops


def test_fp8_product_and_epilogue_are_exact_in_fp32_at_k12288_in_two_k_orders():
    """K = 12288, bias + alpha + two gates + residual: the fp32 evaluation -- accumulated forward, one product after the other,
    and tile-interleaved as the kernels walk K (per 128-byte K-tile the four 32-element lane groups summed apart, then
    combined, then added to the accumulator) -- equals the fp64 reference BIT FOR BIT at every partial sum and at every step of
    the epilogue, before the bf16 rounding.  Row 0 x channel 0 is the worst case of the grid (every product 3 x 3, both scales
    4), rows 1 / 2 its negative and its smallest scales: the bound of the module docstring is met and nearly attained."""
    M, N, K, alpha, gate_split = 6, 8, 12288, 2.0, 3
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0])
    g = torch.Generator().manual_seed(7)
    ea, ew = vals[torch.randint(0, 11, (M, K), generator=g)], vals[torch.randint(0, 11, (N, K), generator=g)]
    sa, sw = pow2((M,), "cpu", 8, -2, 2), pow2((N,), "cpu", 9, -2, 2)
    ea[0], ea[1], ea[2], ew[0], ew[1] = 3.0, -3.0, 3.0, 3.0, 3.0
    sa[0], sa[1], sa[2], sw[0], sw[1] = 4.0, 4.0, 0.25, 4.0, 0.25
    for e in (ea, ew):                                                  # the values ARE e4m3 codes
        assert torch.equal(e.to(torch.float8_e4m3fn).float(), e)
    ep = exact_fp8_epilogue(N, "cpu", 3, bias=True, gates="two", alpha=alpha, res_rows=M)
    bias, g0, g1, res = ep["bias"].float(), ep["gate0"].float(), ep["gate1"].float(), ep["res"][0]
    g0[0], g1[0] = 0.5, 1.0                                             # the worst element under the SMALLER gate: the finest unit
    res = (res / torch.maximum(ep["gate0"].float(), ep["gate1"].float())) * torch.maximum(g0, g1)
    assert torch.equal(res.to(BF).float(), res)
    prod = ea[:, None, :] * ew[None, :, :]                              # fp32 [M, N, K]: every product exact
    p64 = prod.double()
    assert torch.equal(p64, ea.double()[:, None, :] * ew.double()[None, :, :])
    # forward
    cum64 = torch.cumsum(p64, dim=-1)
    acc = torch.zeros(M, N)
    for k in range(K):
        acc = acc + prod[..., k]
    fwd = acc
    assert torch.equal(torch.cumsum(prod, dim=-1).double(), cum64)      # (every prefix, in torch's own fp32 order as well)
    assert torch.equal(fwd.double(), cum64[..., -1])
    # tile-interleaved
    p5, acc = prod.reshape(M, N, K // 128, 4, 32), torch.zeros(M, N)
    for kt in range(K // 128):
        part = torch.zeros(M, N, 4)
        for i in range(32):
            part = part + p5[:, :, kt, :, i]
        acc = acc + ((part[..., 0] + part[..., 1]) + (part[..., 2] + part[..., 3]))
        assert torch.equal(acc.double(), cum64[..., 128 * kt + 127])
    assert torch.equal(acc, fwd)
    assert float(acc[0, 0]) == 9.0 * K
    # the epilogue of csrc/gemm_common.h step by step, fp32 against fp64
    rows = torch.arange(M)[:, None]
    gate = torch.where(rows < gate_split, g0, g1)
    v32 = acc * (sa[:, None] * sw[None, :])
    v64 = cum64[..., -1] * (sa.double()[:, None] * sw.double()[None, :])
    assert torch.equal(v32.double(), v64)
    v32, v64 = v32 + bias, v64 + bias.double()
    assert torch.equal(v32.double(), v64)
    v32, v64 = alpha * v32, alpha * v64
    v32, v64 = v32 * gate, v64 * gate.double()
    assert torch.equal(v32.double(), v64)
    v32, v64 = v32 + res, v64 + res.double()
    assert torch.equal(v32.double(), v64)
    da, dw = ea.double() * sa.double()[:, None], ew.double() * sw.double()[:, None]
    ref = reference(da, dw, bias.to(BF), g0.to(BF), g1.to(BF), gate_split, res, None, alpha)
    assert torch.equal(v32.double(), ref)
    # the bound: multiples of U = 2^(min(s, 0) - 2) * alpha * gate, at most 7078032 of them
    s = torch.log2(sa.double()[:, None] * sw.double()[None, :])
    units = ref / (torch.exp2(torch.clamp(s, max=0.0) - 2) * alpha * gate.double())
    assert torch.equal(units, units.round())
    print(f"largest value before the rounding: {float(units.abs().max()):.0f} units of U (bound 7078032 < 2^23 = 8388608)")
    assert 2.0 ** 22 < float(units.abs().max()) <= 7078032


def test_exact_comparator_names_a_planted_fp8_fault_a_global_bar_passes_it():
    """test_gemm_exact_cpu.py's planted fault on fp8 data: one 16 x 16 fragment that lost one of its 24 128-byte K-tiles fails
    ``assert_exact``, while at the proportions of the FF1 output (17776 x 12288, K = 3072: the same per-element RMS) it scores
    far below the rel-Fro bar of 1e-3."""
    M, N, K = 256, 192, 24 * 128
    _, _, da = exact_fp8_operand(M, K, "cpu", 5)
    _, _, dw = exact_fp8_operand(N, K, "cpu", 6)
    ref = reference(da, dw)
    r, c, kt = slice(32, 48), slice(80, 96), slice(7 * 128, 8 * 128)
    got = ref.to(BF).clone()
    got[r, c] = (ref[r, c] - reference(da[r, kt], dw[c, kt])).to(BF)
    bad = bad_elements(got, ref.to(BF))
    assert bool(bad[r, c].any()) and int(bad.sum()) == int(bad[r, c].sum())
    with pytest.raises(AssertionError, match=r"elements differ.*16: rows 2\.\.2 cols 5\.\.5"):
        assert_exact(got, ref, plan="planted")
    delta = (got.double() - ref.to(BF).double()).norm()
    rms = ref.to(BF).double().norm() / math.sqrt(M * N)
    full = float(delta / (rms * math.sqrt(17776 * 12288)))
    print(f"one fragment short of one of 24 K-tiles at 17776 x 12288: rel-Fro {full:.2e}")
    assert full <= 1e-3                                       # passes the global bar ...
    assert rel_fro(got.float(), ref.to(BF).float()) > 0      # ... though the result is wrong


def _call(fn, args, **more):
    kw = dict(args, **more)
    return fn(kw.pop("a8"), kw.pop("a_scale"), kw.pop("w8"), kw.pop("w_scale"), kw.pop("out"), **kw)


def test_the_fp8_exact_gpu_matrix_reaches_the_paths_it_names(ops):
    """Every case of test_fp8_exact_gpu.py planned on meta tensors: the path, the fallback or the refusal it names."""
    import test_fp8_exact_gpu as g
    from bind_your_avatar_implementation_amd._hip import ByaError
    assert len({c[0] for c in g.FP8_EXACT_CASES}) == len(g.FP8_EXACT_CASES)
    for cid, B, M, N, K, opts, expect, kw in g.FP8_EXACT_CASES:
        args = g.meta_case(B, M, N, K, **kw)
        with ops.options(**opts):
            if expect.startswith("BYA_ERR"):
                with pytest.raises(ByaError, match=expect):
                    _call(ops.gemm_fp8_plan, args)
                continue
            plan = _call(ops.gemm_fp8_plan, args)
        assert plan["path"] == expect and plan["row_chunks"] == 1 and plan["m0"] == 0, (cid, plan)
        # the persistent kernel is reached by the library's own choice only, and not below 200 tiles of 256 x 256
        tiles = B * ((M + 255) // 256) * ((N + 255) // 256)
        assert expect != "p256" or (tiles >= 200 and K >= 512 and not opts), cid
    for M, N, K, expect in g.FP8_ACT_SHAPES:
        args = g.meta_case(1, M, N, K, bias=True)
        for act in g.FP8_ACTS:
            assert _call(ops.gemm_fp8_plan, args, act=act)["path"] == expect, (act, expect)
        for act in g.FP8_ACTS_REFUSED:
            with pytest.raises(ByaError, match="BYA_ERR_UNSUPPORTED"):
                _call(ops.gemm_fp8_plan, args, act=act)
    assert set(g.FP8_ACTS) | set(g.FP8_ACTS_REFUSED) | {None, "none"} == set(ops.ACT)       # every activation there is
    for cid, B, M, N, K, expect, chunks in g.CHUNK_CASES:
        plan = _call(ops.gemm_fp8_plan, g.chunk_meta_case(B, M, N, K))
        assert (plan["path"], plan["row_chunks"], plan["m0"]) == (expect, chunks, 0), (cid, plan)
    # the issue's example for the persistent kernel, 769 x 12800 x 512, runs as TWO pieces (512 + 257 rows): why CHUNK_CASES
    # has 513 x 17152 x 512 instead
    two = g.chunk_meta_case(1, 769, 12800, 512)
    plan = _call(ops.gemm_fp8_plan, two)
    assert (plan["path"], plan["row_chunks"]) == ("p256", 2), plan


def test_forcing_the_persistent_kernel_below_200_tiles_is_not_possible(ops):
    """fp8_path sends launches under 200 tiles of 256 x 256 to the 128 x 128 kernel whatever option fp8_kernel says."""
    import test_fp8_exact_gpu as g
    for value in (0, 1):
        with ops.options(fp8_kernel=value):
            assert _call(ops.gemm_fp8_plan, g.meta_case(1, 256, 256, 512, bias=True))["path"] == "t128x128"
            assert _call(ops.gemm_fp8_plan, g.meta_case(1, 3621, 3328, 512))["path"] == "t128x128"      # 15 x 13 = 195 tiles
    assert _call(ops.gemm_fp8_plan, g.meta_case(1, 3621, 3848, 512))["path"] == "p256"
