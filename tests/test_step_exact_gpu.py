"""GPU: the small kernels of the denoise step (csrc/misc.hip) and the router's scores / head (csrc/router.hip) on exact data
(tests/exact_step.py).  Every case asserts its plan before the launch, runs into a poisoned output inside a sentinel buffer that
must survive, and must equal the fp64 definition rounded once, bit for bit (+0 and -0 equal); SiLU and the sigmoid follow the
window rule, the timestep features a derived bound, the GELUs the bound on record in test_gemm_exact_gpu.py.  A failure names the
element with its row, workgroup, wave and lane.  The case tables live in exact_step.py, where test_step_exact_cpu.py checks their
conditions.  Measured on an MI355X: every exact case bit-equal; SiLU and sigmoid 0 ulp from bf16(fp64) on every element (at most
1.2 % of a case inside the window); GELU(tanh) 0 and GELU(erf) 0.001 ulp; timestep features at most 0.999 of their bound (an
element half a bf16 ulp from its reference, where the bound is 1.954e-3)."""
import pytest
import torch
import torch.nn.functional as F

import exact_step as xs
from exact_step import BF, bad_elements

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def _window(name, got, ref64, describe):
    wrong, share, worst = xs.window_check(got, ref64)
    differ = bad_elements(got, ref64.to(BF))
    print(f"{name}: {float(differ.double().mean()) * 100:.3f} % of the elements differ from bf16(fp64), {share * 100:.3f} % lie in the window "
          f"(cap {xs.WINDOW_CAP * 100:g} %), worst distance {worst} ulp (bound 1, and 0 outside the window)")
    assert share <= xs.WINDOW_CAP
    assert not bool(wrong.any()), describe(wrong, got, ref64.to(BF))


# ------------------------------------------------------------------------------------------------------------ small-M linear
@pytest.mark.parametrize("c", xs.ALL_LIN_CASES, ids=lambda c: c["name"])
def test_linear_small_m_exact(ops, dev, c):
    dat = xs.lin_data(c)
    x, w = dat["x"].to(dev), dat["w"].to(dev)
    bias = None if dat["bias"] is None else dat["bias"].to(dev)
    out, buf, rest = xs.guarded((c["M"], c["N"]), dev)
    act = "silu" if c["kind"] == "siluout" else None
    plan = ops.linear_small_m_plan(x, w, out, act_out=act)
    assert plan == xs.lin_plan(c), plan
    ops.linear_small_m(x, w, bias, out, silu_in=c["kind"] == "siluin", act_out=act)
    torch.cuda.synchronize()
    pre = xs.lin_pre(c, dat, dev)
    print(f"{c['name']}: plan {plan}")
    if c["kind"] == "siluout":
        _window(c["name"], out, xs.silu64(pre), lambda bad, got, ref: xs.describe_lin(c, bad, got, ref))
    else:
        ref = pre.to(BF)
        bad = bad_elements(out, ref)
        assert not bool(bad.any()), f"[plan {plan}] {xs.describe_lin(c, bad, out, ref)}"
    assert xs.guard_intact(buf, rest), f"{c['name']}: a write outside out[M, N]"


# ------------------------------------------------------------------------------------------------------------ timestep features
@pytest.mark.parametrize("flip,dim", xs.TS_EXACT_CASES, ids=lambda v: str(v))
def test_timestep_features_layout_exact(ops, dev, flip, dim):
    """t = 0: sin = 0 and cos = 1 bit for bit, [cos | sin] with flip and [sin | cos] without."""
    t = torch.zeros(3, dtype=torch.int64, device=dev)
    out, buf, rest = xs.guarded((3, dim), dev)
    ops.timestep_features(t, out, flip_sin_to_cos=bool(flip), freq_shift=0.0)
    torch.cuda.synchronize()
    ref, _, _ = xs.ts_reference(t.cpu(), dim, flip, 0.0)
    bad = bad_elements(out, ref.to(BF).to(dev))
    assert not bool(bad.any()), f"flip {flip} dim {dim}: first bad (sample, column) {xs.first_bad(bad)}: got {float(out[xs.first_bad(bad)])!r}"
    assert xs.guard_intact(buf, rest)


@pytest.mark.parametrize("flip,shift,dim", xs.TS_BOUND_CASES, ids=lambda v: str(v))
def test_timestep_features_within_the_derived_bound(ops, dev, flip, shift, dim):
    """t in {1, 500, 999}: every element within half a bf16 ulp + the derived angle budget of fp64 sin / cos (exact_step.py)."""
    t = torch.tensor(xs.TS_VALUES, dtype=torch.int64, device=dev)
    out, buf, rest = xs.guarded((3, dim), dev)
    ops.timestep_features(t, out, flip_sin_to_cos=bool(flip), freq_shift=shift)
    torch.cuda.synchronize()
    ref, ang, expo = xs.ts_reference(t.cpu(), dim, flip, shift)
    bound = xs.ts_bound(ref, ang, expo)
    err = (out.cpu().double() - ref).abs()
    ratio = err / bound
    at = int(ratio.flatten().argmax())
    b, j = at // dim, at % dim
    print(f"flip {flip} shift {shift} dim {dim}: worst error / bound {float(ratio.max()):.3f} at t = {xs.TS_VALUES[b]}, column {j}: error {float(err[b, j]):.3e}, "
          f"bound {float(bound[b, j]):.3e} (largest bound {float(bound.max()):.3e}; the older bar {xs.TS_OLD_BAR})")
    assert bool((err <= bound).all()), (b, j, float(out[b, j]), float(ref[b, j]))
    assert xs.guard_intact(buf, rest)


# ------------------------------------------------------------------------------------------------------------ router scores
@pytest.mark.parametrize("c", xs.SCORES_CASES, ids=lambda c: c["name"])
def test_router_scores_exact(ops, dev, c):
    n_id, N = c["n_id"], c["N"]
    dat = xs.scores_data(c)
    qr, kr, w, b, pos = (dat[k].to(dev) for k in ("qr", "kr", "ln_w", "ln_b", "pos"))
    out, buf, rest = xs.guarded((n_id, N, 512), dev)
    forms = dict(reference_forms="router_scores_wave") if c["wave_form"] else {}
    with ops.options(**forms):
        plan = ops.router_scores_plan(qr, kr, w, b, pos, out, n_id, N)
        assert plan == xs.scores_plan(c), plan
        ops.router_scores(qr, kr, w, b, pos, out, n_id, N, eps=c["eps"])
    torch.cuda.synchronize()
    print(f"{c['name']}: plan {plan}")
    ref = xs.scores_reference(c, dat, dev).to(BF)
    bad = bad_elements(out, ref)
    assert not bool(bad.any()), f"[plan {plan}] {xs.describe_scores(c, bad, out, ref)}"
    assert xs.guard_intact(buf, rest), f"{c['name']}: a write outside out[n_id, N, 512]"


# ------------------------------------------------------------------------------------------------------------ router head
@pytest.mark.parametrize("c", xs.HEAD_CASES, ids=lambda c: c["name"])
def test_router_head_exact(ops, dev, c):
    dat = xs.head_data(c)
    x, w, b = dat["x"].to(dev), dat["w"].to(dev), dat["b"].to(dev)
    r, buf, rest = xs.guarded((c["N"], c["n_id"]), dev)
    ops.router_head(x, w, b, r, c["n_id"], c["N"])
    torch.cuda.synchronize()
    ref64 = xs.head_reference(dat, dev)
    if c["kind"] == "classes":
        ref = ref64.to(BF)
        bad = bad_elements(r, ref)
        assert not bool(bad.any()), xs.describe_head(c, bad, r, ref)
    else:
        _window(c["name"], r, ref64, lambda bad, got, ref: xs.describe_head(c, bad, got, ref))
    assert xs.guard_intact(buf, rest), f"{c['name']}: a write outside r[N, n_id]"


# ------------------------------------------------------------------------------------------------------------ combines
@pytest.mark.parametrize("c", xs.MIX_CASES, ids=lambda c: c["name"])
def test_masked_combine_exact(ops, dev, c):
    """x is an offset, strided view (x_row > D, spare rows per sample) whose surroundings must survive."""
    B, N, D = c["B"], c["N"], c["D"]
    dat = xs.mix_data(c)
    T, spare, Dw = 3, 2, D + 16
    buf = xs.sentinel((B, T + N + spare, Dw), dev)
    x = buf[:, T:T + N, 8:8 + D]
    x.copy_(dat["x"].to(dev))
    rest = torch.ones(buf.shape, dtype=torch.bool, device=dev)
    rest[:, T:T + N, 8:8 + D] = False
    assert x.stride(1) > D and x.stride(0) > N * x.stride(1)
    af = None if dat["af"] is None else dat["af"].to(dev)
    ops.masked_combine(x, dat["feat"].to(dev), dat["r"].to(dev), af, c["mode"], c["alpha"])
    torch.cuda.synchronize()
    _, _, want = xs.mix_reference(c, dat, dev)
    ref = want.to(BF)
    bad = bad_elements(x, ref)
    assert not bool(bad.any()), xs.describe_mix(c, bad, x, ref)
    assert bool(xs.is_sentinel(buf)[rest].all()), f"{c['name']}: a write outside the x view (rows before / after it, or columns beside it)"


@pytest.mark.parametrize("c", xs.MIX_CASES, ids=lambda c: c["name"])
def test_routed_mix_exact(ops, dev, c):
    B, N, D = c["B"], c["N"], c["D"]
    dat = xs.mix_data(c)
    z, zbuf, zrest = xs.guarded((B, N, D), dev)
    wsum, wbuf, wrest = xs.guarded((B, N), dev, dtype=torch.float32)
    af = None if dat["af"] is None else dat["af"].to(dev)
    ops.routed_mix(dat["feat"].to(dev), dat["r"].to(dev), af, c["mode"], z, wsum)
    torch.cuda.synchronize()
    want, wantsum, _ = xs.mix_reference(c, dat, dev)
    ref = want.to(BF)
    bad = bad_elements(z, ref)
    assert not bool(bad.any()), xs.describe_mix(c, bad, z, ref)
    wbad = wsum.double() != wantsum
    assert not bool(wbad.any()), (f"{c['name']}: wsum differs at (sample, token) {xs.first_bad(wbad)}: got {float(wsum[xs.first_bad(wbad)])!r}, "
                                  f"want {float(wantsum[xs.first_bad(wbad)])!r}")
    assert xs.guard_intact(zbuf, zrest) and xs.guard_intact(wbuf, wrest), f"{c['name']}: a write outside z or wsum"


# ------------------------------------------------------------------------------------------------------------ forcing, patches
@pytest.mark.parametrize("frames,per_frame,n_id", xs.FORCING_CASES, ids=lambda v: str(v))
def test_forcing_max_over_frames_exact(ops, dev, frames, per_frame, n_id):
    f, _ = xs.forcing_data(frames, per_frame, n_id)
    out, buf, rest = xs.guarded(tuple(f.shape), dev)
    ops.forcing_max_over_frames(f.to(dev), out, frames, per_frame, n_id)
    torch.cuda.synchronize()
    ref = f.float().max(0).values[None].expand_as(f).to(BF).to(dev)
    bad = bad_elements(out, ref)
    assert not bool(bad.any()), (f"first bad (frame, position, identity) {xs.first_bad(bad)} (column {xs.first_bad(bad)[1] * n_id + xs.first_bad(bad)[2]}: workgroup "
                                 f"{(xs.first_bad(bad)[1] * n_id + xs.first_bad(bad)[2]) // 256}): got {float(out[xs.first_bad(bad)])!r}, want {float(ref[xs.first_bad(bad)])!r}")
    assert xs.guard_intact(buf, rest)


@pytest.mark.parametrize("shape", xs.PATCH_SHAPES, ids=lambda v: str(v))
def test_patchify_unpatchify_every_element(ops, dev, shape):
    """Every element is a different int16 pattern: cols and the round trip compared as int16."""
    B, T, C, H, W = shape
    x = xs.counter(shape, 1234).to(dev)
    n = T * (H // 2) * (W // 2)
    cols, cbuf, crest = xs.guarded((B, n, C * 4), dev)
    ops.patchify(x.view(BF), cols)
    torch.cuda.synchronize()
    want = xs.patchify_reference(x)
    bad = cols.view(torch.int16) != want
    assert not bool(bad.any()), f"patchify {shape}: first bad (sample, patch, column) {xs.first_bad(bad)}"
    assert xs.guard_intact(cbuf, crest)
    y = xs.counter((B, n, C * 4), 4321).to(dev)
    out, obuf, orest = xs.guarded(shape, dev)
    ops.unpatchify(y.view(BF), out)
    torch.cuda.synchronize()
    want = xs.unpatchify_reference(y, shape)
    bad = out.view(torch.int16) != want
    assert not bool(bad.any()), f"unpatchify {shape}: first bad (b, t, c, h, w) {xs.first_bad(bad)}"
    assert xs.guard_intact(obuf, orest)
    back, bbuf, brest = xs.guarded(shape, dev)
    ops.unpatchify(cols, back)
    torch.cuda.synchronize()
    assert torch.equal(back.view(torch.int16), x) and xs.guard_intact(bbuf, brest), f"{shape}: the round trip is not the identity"


# ------------------------------------------------------------------------------------------------------------ activation + add
ACT_REF64 = {"gelu_tanh": lambda y: F.gelu(y, approximate="tanh"), "gelu_erf": F.gelu, "silu": xs.silu64}


def _check_act(act, n, x, got, plan):
    what = f"act_add {act} n={n} [plan {plan}]"
    if act in ("none", "relu", "leaky_relu"):
        ref = xs.act_fp32(act, x).to(BF)
        bad = bad_elements(got, ref)
        assert not bool(bad.any()), f"{what}: {xs.describe_act(n, bad, got, ref)}"
    elif act == "silu":
        _window(what, got, xs.silu64(x.double()), lambda bad, g, ref: f"{what}: {xs.describe_act(n, bad, g, ref)}")
    else:
        from test_gemm_exact_gpu import ACT_ULPS                       # the bound on record for the same device functions
        want = ACT_REF64[act](x.double()).to(BF)
        mag = want.double().abs().clamp_min(2.0 ** -6)                  # results below 2^-6 count in ulps of 2^-6 (that test's rule)
        ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
        err = (got.double() - want.double()).abs() / ulp
        print(f"{what}: worst {float(err.max()):.3f} bf16 ulp(s) from the fp64 activation (bound {ACT_ULPS[act]})")
        assert float(err.max()) <= ACT_ULPS[act], f"{what}: {xs.describe_act(n, err > ACT_ULPS[act], got, want)}"


def _run_act(ops, dev, act, n, residual, inplace):
    x, r = xs.act_data(n, dev)
    plan = ops.act_add_plan(x, x, act=act, res=r if residual else None)
    assert plan == xs.act_plan(n), plan
    y0, buf0, rest0 = xs.guarded((n,), dev)
    ops.act_add(x, y0, act=act)                                        # the activation alone, checked against fp64
    torch.cuda.synchronize()
    _check_act(act, n, x, y0, plan)
    assert xs.guard_intact(buf0, rest0), f"act_add {act} n={n}: a write outside y"
    if not residual and not inplace:
        return
    res = r if residual else None
    want = (y0.float() + r.float()).to(BF) if residual else y0          # bf16(bf16(act) + r) of the kernel's own activation
    if inplace:
        y, buf, rest = xs.guarded((n,), dev)
        y.copy_(x)
        ops.act_add(y, y, act=act, res=res)                            # as the engine calls it: ops.act_add(t, t, ...)
    else:
        y, buf, rest = xs.guarded((n,), dev)
        ops.act_add(x, y, act=act, res=res)
    torch.cuda.synchronize()
    bad = bad_elements(y, want)
    assert not bool(bad.any()), f"act_add {act} n={n} residual={residual} in place={inplace} [plan {plan}]: {xs.describe_act(n, bad, y, want)}"
    assert xs.guard_intact(buf, rest), f"act_add {act} n={n}: a write outside y"


@pytest.mark.parametrize("act", xs.ACTS)
@pytest.mark.parametrize("residual,inplace", [(False, False), (True, False), (True, True)], ids=["plain", "residual", "residual-inplace"])
def test_act_add_small(ops, dev, act, residual, inplace):
    _run_act(ops, dev, act, xs.ACT_SMALL_N, residual, inplace)


@pytest.mark.parametrize("act,residual,inplace", xs.ACT_LARGE_CASES, ids=lambda v: str(v))
def test_act_add_second_round_of_the_grid_stride_loop(ops, dev, act, residual, inplace):
    assert xs.act_plan(xs.ACT_LARGE_N)["rounds"] == 2
    _run_act(ops, dev, act, xs.ACT_LARGE_N, residual, inplace)
    print(f"act_add {act}: plan {xs.act_plan(xs.ACT_LARGE_N)}")


# ------------------------------------------------------------------------------------------------------------ CFG + scheduler step
@pytest.mark.parametrize("name", xs.SCHED_CASES)
def test_cfg_scheduler_step_second_round_and_strided_predictions(ops, dev, name):
    """n = 8192 * 256 + 1000 (two rounds of the grid-stride loop); the CFG pair as rows of a wider buffer (pred_stride > n); with and
    without old_x0, noise and x0_out; prev_sample and x0_out guarded.  Reference: oracle.scheduler's restatement, bit for bit."""
    from oracle import scheduler as osch
    from bind_your_avatar_implementation_amd.pipeline import DDIMScheduler, DPMScheduler
    n = xs.SCHED_N
    g = torch.Generator(device=dev).manual_seed(xs.seed_of(name))
    rnd = lambda *shape: torch.randn(*shape, generator=g, device=dev).to(BF)
    cfg = "nocfg" not in name
    if cfg:
        wide = rnd(2, n + xs.SCHED_PAD)
        pred = wide[:, :n]
        assert pred.stride(0) > n and not pred.is_contiguous()
    else:
        pred = rnd(1, n)
    x = rnd(1, n)
    guidance = 6.0 if cfg else 1.0
    n32 = osch.cfg_combine(pred, guidance) if cfg else pred.float()
    prev, pbuf, prest = xs.guarded((1, n), dev)
    x0buf = x0rest = x0 = None
    if name.startswith("ddim"):
        s, o = DDIMScheduler(), osch.DDIM()
        s.set_timesteps(50), o.set_timesteps(50)
        coef, old, noise, t = s.coefficients(499, guidance), None, None, 499
        ref, ref_x0 = o.step(n32, t, x).to(BF), None
    else:
        s, o = DPMScheduler(), osch.DPM()
        ts = s.set_timesteps(3, dev)
        o.set_timesteps(3)
        second = "second" in name
        t, back = (ts[1], ts[0]) if second else (ts[0], None)
        old = torch.randn(1, n, generator=g, device=dev) if second else None
        noise = rnd(1, n)
        coef, is_second = s.coefficients(t, back, guidance, have_old=second)
        assert is_second == second
        x0, x0buf, x0rest = xs.guarded((1, n), dev, dtype=torch.float32)
        pr, ref_x0 = o.step(n32, old, t, back, x, noise)
        ref = pr.to(BF)
    plan = ops.cfg_scheduler_step_plan(pred, x, coef, out=prev)
    assert plan == xs.sched_plan(n) and plan["rounds"] == 2, plan
    ops.cfg_scheduler_step(pred, x, coef, old_x0=old, noise=noise, x0_out=x0, out=prev)
    torch.cuda.synchronize()
    print(f"{name}: plan {plan}")
    bad = bad_elements(prev, ref)
    assert not bool(bad.any()), f"{name} [plan {plan}]: {xs.describe_sched(n, bad.view(-1), prev.view(-1), ref.view(-1))}"
    assert xs.guard_intact(pbuf, prest), f"{name}: a write outside prev_sample"
    if x0 is not None:
        xbad = x0.view(torch.int32) != ref_x0.float().view(torch.int32)
        assert not bool(xbad.any()), f"{name}: x0_out {xs.describe_sched(n, xbad.view(-1), x0.view(-1), ref_x0.view(-1))}"
        assert xs.guard_intact(x0buf, x0rest), f"{name}: a write outside x0_out"
