"""Every MX GEMM kernel instance (ops.gemm_mx_call: T128X128, P256, T256X256 x the four operand pairs) and both e4m3 GEMM
kernels (ops.gemm_fp8) on full-range bytes, every element against fp64: tests/cond_gemm.py has the data, the measure and the
derivation of the bars; tests/test_gemm_cond_cpu.py holds the restatement inside them and plants the faults they must catch.  The
plan's path is asserted before every launch and every case prints, per family, the worst e with its eps, the differing share and
the restatement's."""
import pytest
import torch

import cond_gemm as C
from exact_gemm import GuardedOut

pytestmark = pytest.mark.gpu


def case_id(c):
    return "-".join(str(v) for v in c)


def epilogue_args(e, M, N, batch):
    kw = {k: e[k] for k in ("bias", "gate0", "gate1", "act") if e[k] is not None}
    if e["gate0"] is not None:
        kw["gate_split"] = e["gate_split"]
    if e["alpha"] != 1.0:
        kw["alpha"] = e["alpha"]
    if e["res"] is not None:
        kw["res"] = e["res"].reshape(batch, M, N) if batch > 1 else e["res"]
    return kw


_TERM = {}


def block_term(key, *operands):
    """cond_gemm.block_term of a case's operands, kept for the next launch on the same data (the epilogue cases share it)."""
    if key not in _TERM:
        _TERM.clear()
        _TERM[key] = C.mx_block_term(*operands) if key[0] == "mx" else C.fp8_block_term(*operands)
    return _TERM[key]


def run_mx(dev, path, fmt, w_fmt, M, N, K, group, epi=None, parts=1, batch=1, name=None):
    """One launch on (A, W) of ``cond_gemm.mx_data`` with the plan asserted first, then ``cond_gemm.check`` of every element
    against fp64 on the device.  -> (got [batch * M, N], operands on the device, plan)."""
    from bind_your_avatar_implementation_amd import ops
    a, w = C.mx_data(fmt, w_fmt, M, N, K, group, batch)
    e = C.epilogue_to(C.make_epilogue(M, N, C.seed_of(f"{M}x{N}"), batch=batch, **epi) if epi else C.NO_EPILOGUE, dev)
    lead = (batch, M) if batch > 1 else (M,)
    ac, asc = C.packed(a, fmt).reshape(*lead, -1).to(dev), a["scales"].reshape(*lead, -1).to(dev)
    wc, wsc = C.packed(w, w_fmt).to(dev), w["scales"].to(dev)
    out = GuardedOut(M, N, dev, batch=batch, parts=parts)
    kw = epilogue_args(e, M, N, batch)
    if e["rowscale"] is not None:
        kw["bias_rowscale"] = e["rowscale"]
    if parts > 1:
        kw["split"] = out.split
    kernel = C.KERNEL_OF[(path, fmt)]
    plan = ops.gemm_mx_call_plan(ac, asc, wc, wsc, out.view(), kernel, fmt, w_fmt, **kw)
    assert plan is not None and plan["path"] == path, (path, kernel, plan)
    ops.gemm_mx_call(ac, asc, wc, wsc, out.view(), kernel, fmt, w_fmt, **kw)
    torch.cuda.synchronize()
    assert out.guard_intact(), "guard band"
    got = out.gathered().reshape(batch * M, N)
    a64, w64 = C.values(a, fmt).to(dev), C.values(w, w_fmt).to(dev)
    y64, S, T = C.reference(a64, w64, e, M, T=block_term(("mx", fmt, w_fmt, M, N, K, group, batch), a64, w64, fmt, w_fmt,
                                                               a["scales"], w["scales"]))
    name = name or f"{path} {fmt} x {w_fmt} {batch}x{M}x{N}x{K} {group}"
    C.check(name, got, y64, S, K, C.out_family(a, w), restated=C.restate(a64, w64, e, M), ops=C.epilogue_ops(e), act=e["act"],
            plan=plan, exact=() if epi else C.exact_families(fmt, w_fmt, K), T=T)
    return got, (ac, asc, wc, wsc), plan


@pytest.mark.parametrize("case", C.mx_cases(), ids=case_id)
def test_mx_gemm_every_element_against_fp64(dev, case):
    """near / spread / cancel / subnormal / extreme rows in one launch, the far blocks in a second one on the same shape."""
    path, fmt, w_fmt, M, N, K = case
    for group in ("mid", "far"):
        run_mx(dev, path, fmt, w_fmt, M, N, K, group)


def test_the_instructions_block_sum_is_the_model_of_cond_gemm(dev):
    """The probes behind the block term (cond_gemm.block_sum_probes), through the T128X128 e4m3 kernel, one instruction per output
    at K = 128: the kernel returns the bits the MODEL predicts -- s cut to its bit 2^-11 under a pair of field exponents 2, with
    either sign, under mantissas 1.75 x 1.75 and under SUBNORMAL codes times 2^8 alike; zero from the next exponent on; s whole
    beside zero codes, and with the pair in another block or K-step at any distance.  If the instruction did otherwise the
    term of bar (a) would be wrong, or wider than it need be."""
    from bind_your_avatar_implementation_amd import ops
    from mx_ref import dequant_mx
    for name, K, a, asc, w, wsc, want in C.block_sum_probes():
        W, WS = w[None].expand(16, K).contiguous(), wsc[None].expand(16, K // 32).contiguous()
        out = GuardedOut(a.shape[0], 16, dev)
        args = (a.to(dev), asc.to(dev), W.to(dev), WS.to(dev), out.view(), 0, "mxfp8", "mxfp8")
        assert ops.gemm_mx_call_plan(*args)["path"] == "t128x128"
        ops.gemm_mx_call(*args)
        torch.cuda.synchronize()
        got = out.gathered().double().cpu()
        a64, w64 = dequant_mx(a, asc, "mxfp8"), dequant_mx(W, WS, "mxfp8")
        model = C.restate(a64, w64, model=True, floors=(C.exp_floor(asc, "mxfp8"), C.exp_floor(WS, "mxfp8"))).double()
        print(f"{name}: got {got[:, 0].tolist()}")
        assert out.guard_intact()
        assert torch.equal(got, want[:, None].expand(-1, 16)), (name, got[:, 0].tolist(), want.tolist())
        assert torch.equal(got, model), name


@pytest.mark.parametrize("inst", C.mx_instances(), ids=case_id)
def test_mx_gemm_one_hot_equals_the_single_product(dev, inst):
    """Every output is one product: the code decode, the K position and the scale byte (0 .. 254) at every position, with no
    accumulation involved -- bit for bit."""
    path, fmt, w_fmt = inst
    M, N, K = C.T256_SHAPE if path == "t256x256" else C.ONE_HOT_SHAPE
    run_mx(dev, path, fmt, w_fmt, M, N, K, "one-hot")


def epi_shape(path, which, p256=None):
    """(batch, M, N, K, parts) of an epilogue case: the instance's smallest launch, N a multiple of 3 under a column split."""
    M, N, K = C.EPI_SHAPE[path] if p256 is None else p256
    big = M > 1000
    if which == "split3":
        return 1, M, N - N % 24 if big else N, K, 3
    if which == "batch2":
        return 2, M // 2 if big else M, N, K, 1
    return 1, M, N, K, 1


@pytest.mark.parametrize("which", list(C.EPILOGUES))
@pytest.mark.parametrize("inst", C.mx_instances(), ids=case_id)
def test_mx_gemm_epilogues_against_fp64(dev, inst, which):
    """bias not on a grid, GELU, two gates changing at a row that is no tile boundary + residual, n_split 3, alpha 0.5,
    bias_rowscale, batch 2 -- each through the fp64 definition, on the ``mid`` rows."""
    path, fmt, w_fmt = inst
    B, M, N, K, parts = epi_shape(path, which)
    run_mx(dev, path, fmt, w_fmt, M, N, K, "mid", epi=C.EPILOGUES[which], parts=parts, batch=B,
           name=f"{path} {fmt} x {w_fmt} {which} {B}x{M}x{N}x{K}")


@pytest.mark.parametrize("out_fmt", ["mxfp8", "mxfp6"])
@pytest.mark.parametrize("inst", C.mx_instances(), ids=case_id)
def test_mx_quantising_epilogue_equals_the_quantiser_on_the_checked_output(dev, inst, out_fmt):
    """gemm_mx_quant's codes and scales equal quantize_mx of the plain launch's bf16 output -- the output ``run_mx`` has just held
    to fp64 per element -- on spread and far operands."""
    from bind_your_avatar_implementation_amd import ops
    path, fmt, w_fmt = inst
    M, N, K = (3500, 3712, 256) if path == "t256x256" else (300, 256, 512)
    kernel = 18 if path == "p256" else 0
    for group in ("mid", "far"):
        got, (ac, asc, wc, wsc), _ = run_mx(dev, path, fmt, w_fmt, M, N, K, group)
        c_ref, s_ref = ops.quantize_mx(got.contiguous(), out_fmt)
        codes = torch.full_like(c_ref, 0xA5)
        scales = torch.full_like(s_ref, 0xA5)
        plan = ops.gemm_mx_call_plan(ac, asc, wc, wsc, codes, kernel, fmt, w_fmt, out_scales=scales, out_fmt=out_fmt)
        assert plan is not None and plan["path"] == path, (path, kernel, plan)
        ops.gemm_mx_call(ac, asc, wc, wsc, codes, kernel, fmt, w_fmt, out_scales=scales, out_fmt=out_fmt)
        torch.cuda.synchronize()
        assert torch.equal(scales, s_ref), (inst, out_fmt, group, int((scales != s_ref).sum()))
        assert torch.equal(codes, c_ref), (inst, out_fmt, group, int((codes != c_ref).sum()))


# ------------------------------------------------------------------------------------------------------------------- fp8
def run_fp8(dev, path, M, N, K, epi=None, parts=1, batch=1, one_hot=False, name=None):
    from bind_your_avatar_implementation_amd import ops
    a, w = C.fp8_data(M, N, K, one_hot, batch)
    e = C.epilogue_to(C.make_epilogue(M, N, C.seed_of(f"fp8-{M}x{N}"), batch=batch, **epi) if epi else C.NO_EPILOGUE, dev)
    lead = (batch, M) if batch > 1 else (M,)
    a8, w8 = C.packed(a, "fp8").reshape(*lead, K).to(dev), C.packed(w, "fp8").to(dev)
    asc, wsc = a["scales"].to(dev), w["scales"].to(dev)
    out = GuardedOut(M, N, dev, batch=batch, parts=parts)
    kw = epilogue_args(e, M, N, batch)
    if parts > 1:
        kw["split"] = out.split
    plan = ops.gemm_fp8_plan(a8, asc, w8, wsc, out.view(), **kw)
    assert plan["path"] == path, (path, plan)
    ops.gemm_fp8(a8, asc, w8, wsc, out.view(), **kw)
    torch.cuda.synchronize()
    assert out.guard_intact(), "guard band"
    got = out.gathered().reshape(batch * M, N)
    y64, S, T = C.reference(C.values(a, "fp8").to(dev), C.values(w, "fp8").to(dev), e, M,
                            T=block_term(("fp8", M, N, K, one_hot, batch), a, w, dev), base_ops=2)
    C.check(name or f"fp8 {path} {batch}x{M}x{N}x{K}" + (" one-hot" if one_hot else ""), got, y64, S, K, C.out_family(a, w),
            restated=C.restate_fp8(a, w, e, M, dev), ops=C.epilogue_ops(e, 2), act=e["act"], plan=plan, exact=(), T=T)


@pytest.mark.parametrize("case", C.FP8_CASES, ids=case_id)
def test_fp8_gemm_every_element_against_fp64(dev, case):
    run_fp8(dev, *case)


@pytest.mark.parametrize("case", [("t128x128", 300, 512, 512), ("p256", 3500, 3704, 512)], ids=case_id)
def test_fp8_gemm_one_hot_is_one_product_rounded_once(dev, case):
    """S is the single product, so eps = 2 (K + 2) u32 S / ulp is at most 2 * 514 * 2^-24 * 2^8 = 0.016 ulp: in effect the
    correctly rounded a_scale * w_scale * a * w."""
    run_fp8(dev, *case, one_hot=True)


@pytest.mark.parametrize("which", [k for k in C.EPILOGUES if k != "rowscale"])
@pytest.mark.parametrize("path", ["t128x128", "p256"])
def test_fp8_gemm_epilogues_against_fp64(dev, path, which):
    B, M, N, K, parts = epi_shape(path, which, (300, 264, 512) if path == "t128x128" else C.FP8_P256_SHAPE)
    run_fp8(dev, path, M, N, K, epi=C.EPILOGUES[which], parts=parts, batch=B, name=f"fp8 {path} {which} {B}x{M}x{N}x{K}")
