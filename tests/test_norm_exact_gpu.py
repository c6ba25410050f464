"""GPU: csrc/norm.hip on exact data (tests/exact_norm.py).  Every case asserts its plan (ops.layernorm_plan /
ops.qknorm_rope_plan) BEFORE the launch, runs into a NaN-poisoned, strided, offset view with a sentinel guard band, and asserts
bit equality with the fp64 definition rounded once; a failure names the element, its row, its wave and its lane."""
import pytest
import torch

import exact_norm as xn
from exact_norm import BF, SENTINEL, GuardedOut

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


_CACHE = {}


def _ln_case(c, dev):
    """Data and fp64 reference of a case, made once per module (the largest is 75 MB) -> (dat, x view on the device, ref bf16)."""
    if c["name"] not in _CACHE:
        dat = xn.ln_data(c)
        ref = xn.ln_reference_case(c, dat, dev).to(BF)
        _CACHE[c["name"]] = (dat, ref)
    dat, ref = _CACHE[c["name"]]
    # x as an offset view: row stride D + 40, two spare rows per batch entry (batch stride > rows * ld)
    B, M, D = dat["x"].shape
    wide = torch.full((B, M + 2, D + 40), 77.0, dtype=BF, device=dev)
    x = wide[:, 1:M + 1, 16:16 + D]
    x.copy_(dat["x"].to(dev))
    return dat, (x if B > 1 else x[0]), ref


def _params(dat, dev):
    mv = lambda t: None if t is None else t.to(dev)
    kw = dict(weight=mv(dat["w"]), bias=mv(dat["b"]))
    if dat["sh"] is not None:
        sh, sc = mv(dat["sh"]), mv(dat["sc"])                          # [B, 2, D]: set (z, side)
        kw.update(shift0=sh[0, 0], scale0=sc[0, 0], shift1=sh[0, 1], scale1=sc[0, 1], mod_batch_stride=2 * sh.shape[-1])
    return kw


def _run_ln(ops, c, dat, x, ref, kw, generic_form):
    out = GuardedOut(c["rows"], c["D"], x.device, batch=c["batch"])
    assert out.view().stride(-2) != x.stride(-2) and x.stride(-2) != c["D"]
    with ops.options(reference_forms="ln_generic" if generic_form else []):
        plan = ops.layernorm_plan(x, out.view(), split=c["split"], **kw)
        ops.layernorm(x, out.view(), eps=dat["eps"], split=c["split"], **kw)
        torch.cuda.synchronize()
    got = out.view() if c["batch"] > 1 else out.view()[None]
    xn.assert_ln_exact(c, plan, got, ref, "ln_generic" if generic_form else "")
    assert out.guard_intact(), f"{c['name']} [plan {plan}]: the guard band around the output was written"
    return plan


@pytest.mark.parametrize("c", xn.GENERIC_CASES, ids=lambda c: c["name"])
def test_layernorm_generic_exact(ops, dev, c):
    dat, x, ref = _ln_case(c, dev)
    kw = _params(dat, dev)
    vec, nv = xn.VEC_NV[c["D"]]
    with ops.options(reference_forms="ln_generic" if c["generic_form"] else []):
        plan = ops.layernorm_plan(x, _like_out(c, dev), split=c["split"], **kw)
    total = c["rows"] * c["batch"]
    assert plan == {"kernel": "generic", "vec": vec, "nv": nv, "modulated": xn.modulated(c), "rows_per_wave": 1, "waves": total,
                    "grid": (total + 3) // 4}, plan
    _run_ln(ops, c, dat, x, ref, kw, c["generic_form"])
    _CACHE.pop(c["name"], None)


@pytest.mark.parametrize("c", xn.ROWS_CASES, ids=lambda c: c["name"])
def test_layernorm_rows_kernel_exact(ops, dev, c):
    dat, x, ref = _ln_case(c, dev)
    kw = _params(dat, dev)
    total = c["rows"] * c["batch"]
    plan = ops.layernorm_plan(x, _like_out(c, dev), split=c["split"], **kw)
    waves = (total + c["rpw"] - 1) // c["rpw"]
    assert plan == {"kernel": "rows", "vec": 8, "nv": 6, "modulated": xn.modulated(c), "rows_per_wave": c["rpw"], "waves": waves,
                    "grid": (waves + 3) // 4}, plan
    assert c["events"] <= xn.ln_events(c, plan), (c["events"], xn.ln_events(c, plan))
    _run_ln(ops, c, dat, x, ref, kw, False)
    # ... and the one-row-per-wave kernel on the same data: both must equal the reference
    plan_g = _run_ln(ops, c, dat, x, ref, kw, True)
    assert plan_g["kernel"] == "generic" and plan_g["rows_per_wave"] == 1
    _CACHE.pop(c["name"], None)


def _like_out(c, dev):
    """A meta stand-in with GuardedOut's view geometry (the plan only reads shape, strides and alignment)."""
    return GuardedOut(c["rows"], c["D"], "meta", batch=c["batch"]).view()


@pytest.mark.parametrize("c", xn.QUANT_CASES, ids=lambda c: c["name"])
def test_layernorm_fp8_and_mx_exact(ops, dev, c):
    dat, x, _ = _ln_case(c, dev)
    kw = _params(dat, dev)
    B, M, D = c["batch"], c["rows"], c["D"]
    codes_ref, scales_ref = xn.quant_expected(c, dat)
    rb = codes_ref.shape[-1]
    # codes in a wider, guarded byte matrix: row pitch rb + 64, three rows before and five after each batch entry
    GUARD = 0xA5
    buf = torch.full((B, M + 8, rb + 64), GUARD, dtype=torch.uint8, device=dev)
    q = buf[:, 3:3 + M, 8:8 + rb]
    q = q if B > 1 else q[0]
    plan = ops.layernorm_plan(x, q, split=c["split"], out_kind=c["out"], **kw)
    total = B * M
    assert plan == {"kernel": "generic", "vec": 8, "nv": 6, "modulated": True, "rows_per_wave": 1, "waves": total, "grid": (total + 3) // 4}, plan
    if c["out"] == "fp8":
        scales = torch.full((B, M), float("nan"), dtype=torch.float32, device=dev)
        ops.layernorm_fp8(x, q, scales, eps=dat["eps"], split=c["split"], **kw)
    else:
        scales = torch.full((B, M, D // 32), 0xEE, dtype=torch.uint8, device=dev)
        ops.layernorm_mx(x, q, scales, fmt=c["out"], eps=dat["eps"], split=c["split"], **kw)
    torch.cuda.synchronize()
    got, want = q.reshape(total, rb).cpu(), codes_ref.reshape(total, rb)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"{c['name']} [plan {plan}]: {bad.shape[0]} code bytes differ; first: row {int(bad[0, 0])} (batch entry "
                              f"{int(bad[0, 0]) // M}) byte {int(bad[0, 1])}: got {int(got[tuple(bad[0])])}, want {int(want[tuple(bad[0])])}")
    sg, sw = scales.reshape(total, -1).cpu(), scales_ref.reshape(total, -1)
    bad = (sg != sw).nonzero()
    assert bad.numel() == 0, f"{c['name']} [plan {plan}]: {bad.shape[0]} scales differ; first: row {int(bad[0, 0])} block {int(bad[0, 1])}"
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, 3:3 + M, 8:8 + rb] = False
    assert bool((buf[mask] == GUARD).all()), f"{c['name']} [plan {plan}]: bytes outside the rows' code bytes were written"
    _CACHE.pop(c["name"], None)


# ------------------------------------------------------------------------------------------------------------ q/k-norm + RoPE
@pytest.mark.parametrize("c", xn.QK_CASES, ids=lambda c: c["name"])
def test_qknorm_rope_exact(ops, dev, c):
    dat = xn.qk_data(c)
    B, S, H, T, only = c["batch"], c["S"], c["heads"], c["text_rows"], c["only"]
    W = H * 64
    # q | k | v packed: ld = 3 * heads * 64, three spare rows per batch entry; v and the spare rows hold a sentinel
    buf = torch.full((B, S + 3, 3 * W), 0, dtype=torch.int16, device=dev)
    buf.fill_(SENTINEL)
    bf = buf.view(BF)
    bf[:, :S, :W] = dat["q"].to(dev)
    bf[:, :S, W:2 * W] = dat["k"].to(dev)
    before = buf.clone()
    q, k = bf[:, :S, :W], bf[:, :S, W:2 * W]
    assert q.stride(1) == 3 * W and q.stride(0) > S * 3 * W
    qa, ka = (None if only == 2 else q), (None if only == 1 else k)
    mv = lambda t: None if t is None else t.to(dev)
    cos, sin = mv(dat["cos"]), mv(dat["sin"])
    stats = torch.zeros(c["slots"], 2, B * H, dtype=torch.float32, device=dev) if c["slots"] else None
    plan = ops.qknorm_rope_plan(qa, ka, H, T, cos=cos, stats=stats)
    pairs = B * S * H * (1 if only else 2)
    assert plan == {"stats": bool(c["slots"]), "only": only, "slots": c["slots"], "pairs": pairs, "waves": (pairs + 7) // 8,
                    "grid": ((pairs + 7) // 8 + 3) // 4}, plan
    assert c["events"] <= xn.qk_waves(c), (c["events"], xn.qk_waves(c))
    ops.qknorm_rope(qa, ka, *(mv(dat[n]) for n in ("qw", "qb", "kw", "kb")), cos, sin, heads=H, text_rows=T, eps=dat["eps"],
                    k_scale=c["k_scale"], stats=stats)
    torch.cuda.synchronize()
    refs = xn.qk_reference_case(c, dat)                                    # the fp64 definition; q never takes k_scale
    for which, (t, r64) in enumerate(zip((q, k), refs)):
        if only and only - 1 != which:
            continue
        ref = r64.to(BF).to(dev)
        bad = xn.bad_elements(t, ref)
        assert not bool(bad.any()), f"{c['name']} [plan {plan}]: {xn.describe_qk(c, bad, t, ref, which)}"
    # everything the launch does not own -- the other tensor of a one-tensor call, v, the spare rows -- is untouched
    mask = torch.ones_like(buf, dtype=torch.bool)
    if only != 2:
        mask[:, :S, :W] = False
    if only != 1:
        mask[:, :S, W:2 * W] = False
    assert torch.equal(buf[mask], before[mask]), f"{c['name']} [plan {plan}]: elements outside the processed tensors were written"
    if stats is not None:
        ref = torch.stack([r.to(BF).double() for r in refs])
        want = xn.qk_stats_table(c, ref)
        if only:
            want[:, 2 - only] = 0                                          # the tensor that is not processed: entries stay 0
        got = stats.cpu().double()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (f"{c['name']} [plan {plan}]: {bad.shape[0]} statistics entries differ; first (slot, q|k, batch * heads + head) "
                                  f"{tuple(int(v) for v in bad[0])}: got {float(got[tuple(bad[0])])!r}, want {float(want[tuple(bad[0])])!r}")
        assert bool((want[plan["grid"]:] == 0).all()) and bool((got[plan["grid"]:] == 0).all())      # slots the grid never reaches
        assert torch.equal(got.amax(0), want.amax(0))
