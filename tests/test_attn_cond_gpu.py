"""GPU: every attention path on the hard score rows of tests/cond_attn.py, every output element against the fp64 softmax of the
bf16 values the kernel reads.  Each case holds every score family its path admits, asserts the plan or instance BEFORE the launch
(as test_attn_exact_gpu.py does), prints per family the worst e, eps and the bias b next to the restatement's, and asserts the three
bars of cond_attn's docstring: e <= 1 + eps per element, |b| <= |b of the restatement| + 0.25, everything finite with the guard
band intact.  The last three tests run launches twice, with zeros and then with NaN in everything that surrounds the inputs (row
padding, rows directly behind the last key / query row, rows of no group): the outputs must be equal bit for bit.

docs/kernels.md holds the figures these tests print."""
import pytest
import torch

import cond_attn as C
import exact_attn as X
import test_attn_exact_gpu as G
from cond_attn import BF

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def _heads(o, c):
    """The launch's output [B L2, Sq, H D] -> [B H L2, Sq, D], the order of cond_attn.per_variant."""
    B, H, L2, Sq, D = c["B"], c["H"], c["L2"], c["Sq"], c["D"]
    return o.reshape(B, L2, Sq, H, D).permute(0, 3, 1, 2, 4).reshape(B * H * L2, Sq, D)


def _device_bound(c, d, kw, dev):
    """The case's own statistics table in place of attn_layout's -> the heads expected to be flagged (B > 90)."""
    if c["kind"] != "dev":
        return None
    stats, bound = C.device_bound_stats(d, c["B"], c["H"], dev)
    assert not bool(((bound >= 89) & (bound <= 91)).any()), "fp32 rounding of the square roots would decide a flag"
    kw["bound"] = (stats, 2, torch.full((bound.numel(),), -7, dtype=torch.int32, device=dev))
    return (bound > 90).to(dev)


def _plan(ops, c, o, kw):
    plan = ops.attention_plan(o, **kw)
    key = ops.attention_plan_key(plan)
    assert key == X.attn_case_key(c), (key, plan)
    assert plan["q_tile"] == (512 if c["kind"] in ("w4", "dev") else 128) and plan["second_launch"] == (c["kind"] == "dev")
    return plan, key


def _forms(c):
    return ["attn_narrow_store"] if c["narrow"] else []


@pytest.mark.parametrize("case", C.ATTN_CASES, ids=[c["name"] for c in C.ATTN_CASES])
def test_attn_fwd_cond(ops, dev, case):
    c = case
    d = C.attn_case_data(c)
    qv, kv, vv, fam = C.per_variant(d, dev)
    o64, A = C.reference64(qv, kv, vv)
    eps = C.case_eps(c, qv, kv)
    dd = dict(q=d["q"].to(dev), k=d["k"].to(dev), v=d["v"].to(dev), want=o64.view(c["B"] * c["H"], c["L2"], c["Sq"], c["D"]))
    q, k, v, g, o, _, kw, _ = G.attn_layout(c, dd, dev)
    flagged = _device_bound(c, d, kw, dev)
    with ops.options(attn_streamk=c["sk_opt"], reference_forms=_forms(c)):
        plan, key = _plan(ops, c, o, kw)
        ops.attention(q, k, v, o, tag="cond", **kw)
        if c["sk"] or not c["sk_opt"]:
            assert ops.attn_workspace_status() == 0
    C.check(c["name"], _heads(o, c), o64, A, C.restate(qv, kv, vv), fam, C.families_of(c["kind"]), eps, plan=f"{key} {plan}")
    assert g.guard_intact(), f"{c['name']} [plan {key}]: wrote outside its output view"
    if flagged is not None:
        flags = kw["bound"][2]
        assert torch.equal(flags != 0, flagged) and bool((flags != -7).all()), (flags.tolist(), flagged.tolist())
        assert c["Sq"] * c["B"] * c["H"] < 10 or (bool(flagged.any()) and not bool(flagged.all()))


def _mix_layout(c, d, dev, surround=None):
    """q [G, Sq, H D], k, v [n_id, G, Skv, H D] (bf16, rows ``pad`` wider or inside ``surround`` = (pad, extra rows, fill)), the
    guarded z and the launch's keywords."""
    Gr, H, n_id, Sq, Skv, D = c["grp"], c["H"], c["n_id"], c["Sq"], c["Skv"], c["D"]
    wrap = (lambda t: X.strided(t, c["pad"])) if surround is None else (lambda t: _surround(t, *surround))
    q = wrap(d["q"].to(dev).view(Gr, H, Sq, D).permute(0, 2, 1, 3).reshape(Gr, Sq, H * D).to(BF))
    k = wrap(d["k"].to(dev).view(Gr, H, n_id, Skv, D).permute(2, 0, 3, 1, 4).reshape(n_id, Gr, Skv, H * D).to(BF))
    v = wrap(d["v"].to(dev).view(Gr, H, n_id, Skv, D).permute(2, 0, 3, 1, 4).reshape(n_id, Gr, Skv, H * D).to(BF))
    g = X.GuardedOut(Sq, H * D, dev, batch=Gr, col0=c["col0"])
    z = g.bf[:, g.r0:g.r0 + Sq, g.c0:g.c0 + H * D]
    kw = dict(head_dim=D, heads=H, n_id=n_id, n_grp=Gr, Sq=Sq, Skv=Skv, q_strides=(q.stride(0), q.stride(1)),
              k_strides=(k.stride(0), k.stride(1), k.stride(2)), v_strides=(v.stride(0), v.stride(1), v.stride(2)),
              z_strides=(z.stride(0), z.stride(1)), scale=X.UNIT_SCALE)
    return q, k, v, g, z, kw


def _mix_launch(ops, c, d, q, k, v, z, kw, dev):
    Gr, Sq = c["grp"], c["Sq"]
    wsum = torch.full((Gr * Sq + 8,), -5.0, device=dev)
    with ops.options(reference_forms=["kv_mix_generic"] if c["generic"] else []):
        plan = ops.attn_kv_mix_plan(z, d["af"], **kw)
        key = f"{plan['form']}_d{plan['head_dim']}" + ("+big_lds" if plan["big_lds"] else "")
        assert key == X.mix_case_key(c) and plan["form"] == c["form"], (key, plan)
        ops.attn_kv_mix(q, k, v, d["r"], d["af"], z, wsum[:Gr * Sq], **kw)
    bad = (wsum[:Gr * Sq] != d["wsum"]).nonzero()
    assert bad.numel() == 0, f"{c['name']}: wsum differs at {bad[:4].flatten().tolist()}"
    assert bool((wsum[Gr * Sq:] == -5.0).all())
    return plan


@pytest.mark.parametrize("case", C.MIX_CASES, ids=[c["name"] for c in C.MIX_CASES])
def test_attn_kv_mix_cond(ops, dev, case):
    c = case
    Gr, H, Sq, D = c["grp"], c["H"], c["Sq"], c["D"]
    d = C.mix_case_data(c, dev)
    z64, A, restated, fam = C.mix_reference(c, d, dev)
    qv, kv, _, _ = C.per_variant(d, dev)
    eps = C.eps_of(c["Skv"], D, C.s_abs(qv, kv), n_id=c["n_id"])
    q, k, v, g, z, kw = _mix_layout(c, d, dev)
    plan = _mix_launch(ops, c, d, q, k, v, z, kw, dev)
    got = z.reshape(Gr, Sq, H, D).permute(0, 2, 1, 3).reshape(Gr * H, Sq, D)
    C.check("mix " + c["name"], got, z64, A, restated, fam, C.families_of("mix"), eps, plan=plan)
    assert g.guard_intact(), f"{c['name']}: wrote outside z"


def _tiny_layout(c, d, rows, idx, dev, fill=1.0, extra=3):
    """The q | k | v matrix [rows + extra, 3 H 64 + 8] with ``fill`` in the rows of no group and in the columns no head owns, the
    three views, the guarded output (rows of no group hold 3.0)."""
    L, H = c["L"], c["H"]
    groups, W = c["n_outer"] * c["n_inner"], H * 64
    col0 = 4 if c["unaligned"] else 0
    qkv = torch.full((rows + extra, 3 * W + 8), fill, dtype=BF, device=dev)
    idx = idx.to(dev)
    for t, name in enumerate(("q", "k", "v")):
        src = d[name].to(dev).reshape(groups, H, L, 64).permute(0, 2, 1, 3).reshape(groups * L, W).to(BF)
        qkv[idx.reshape(-1), col0 + t * W:col0 + (t + 1) * W] = src
    g = X.GuardedOut(rows + extra, W, dev, col0=8 if not c["unaligned"] else 4)
    o = g.view()
    o[rows:] = 3.0
    q, k, v = (qkv[:, col0 + t * W:col0 + (t + 1) * W] for t in range(3))
    return qkv, q, k, v, g, o


def _tiny_launch(ops, c, qkv, q, k, v, o):
    L, H, no, ni = c["L"], c["H"], c["n_outer"], c["n_inner"]
    plan = ops.attn_tiny_plan(q, k, v, o, L, H, no, ni, qkv.stride(0), o.stride(0))
    assert plan["instance"] == c["instance"], plan
    assert plan["waves"] == no * ni * (H // 8 if plan["instance"].startswith("tiny8") else H)
    ops.attn_tiny(q, k, v, o, L, H, no, ni, L * ni if c["temporal"] else 0, ni, qkv.stride(0), o.stride(0), X.LN2)
    return plan


@pytest.mark.parametrize("case", C.TINY_CASES, ids=[c["name"] for c in C.TINY_CASES])
def test_attn_tiny_cond(ops, dev, case):
    c = case
    L, H = c["L"], c["H"]
    d, rows, idx = C.tiny_case_data(c)
    groups = c["n_outer"] * c["n_inner"]
    qv, kv, vv, fam = C.per_variant(d, dev)
    o64, A = C.reference64(qv, kv, vv)
    eps = C.eps_of(L, 64, C.s_abs(qv, kv), tiny=True)
    qkv, q, k, v, g, o = _tiny_layout(c, d, rows, idx, dev)
    plan = _tiny_launch(ops, c, qkv, q, k, v, o)
    got = o[idx.to(dev).reshape(-1)].reshape(groups, L, H, 64).permute(0, 2, 1, 3).reshape(groups * H, L, 64)
    C.check("tiny " + c["name"], got, o64, A, C.restate(qv, kv, vv), fam, C.families_of("tiny"), eps, plan=plan)
    assert g.guard_intact() and bool((o[rows:] == 3.0).all()), f"{c['name']}: wrote outside its groups' rows"


# ------------------------------------------------------------------------------------------------ poisoned surroundings of the inputs
def _surround(t, pad, extra, fill):
    """``t`` [..., R, W] as a view of a buffer [..., R + extra, W + pad] that holds ``fill`` everywhere else: the pad columns of
    every row, and ``extra`` rows directly behind row R - 1 of every leading index."""
    buf = torch.full((*t.shape[:-2], t.shape[-2] + extra, t.shape[-1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-2], :t.shape[-1]] = t
    return buf[..., :t.shape[-2], :t.shape[-1]]


@pytest.mark.parametrize("kind", ["run", "pre", "d128", "w4", "dev"])
def test_attn_fwd_ignores_what_surrounds_its_inputs(ops, dev, kind):
    """The kernels rely on the buffer descriptor's range check: keys past Skv land in LDS as zeros.  A descriptor one row too long
    would turn 0 * NaN in P . V into NaN; a q row read past Sq - 1, or a pad column read as data, shows the same way."""
    for shape in C.POISON_SHAPES:
        c = next(c for c in C.ATTN_CASES if c["name"] == f"{kind}-{shape}")
        B, H, L2, Sq, Skv, D = c["B"], c["H"], c["L2"], c["Sq"], c["Skv"], c["D"]
        assert Skv % 64
        d = C.attn_case_data(c)
        dd = dict(q=d["q"].to(dev), k=d["k"].to(dev), v=d["v"].to(dev), want=torch.empty(B * H, L2, Sq, D, device="meta"))
        outs = []
        for extra, fill in ((0, 0.0), (3, NAN)):
            _, _, _, g, o, _, kw, _ = G.attn_layout(c, dd, dev)
            flagged = _device_bound(c, d, kw, dev)
            q = _surround(dd["q"].view(B, H, Sq, D).permute(0, 2, 1, 3).reshape(B, Sq, H * D).to(BF), 8, extra, fill)
            k = _surround(dd["k"].view(B, H, L2, Skv, D).permute(0, 2, 3, 1, 4).reshape(B, L2, Skv, H * D).to(BF), 8, extra, fill)
            v = _surround(dd["v"].view(B, H, L2, Skv, D).permute(0, 2, 3, 1, 4).reshape(B, L2, Skv, H * D).to(BF), 8, extra, fill)
            kw.update(q_strides=(q.stride(0), 0, q.stride(1)), k_strides=(k.stride(0), k.stride(1), k.stride(2)),
                      v_strides=(v.stride(0), v.stride(1), v.stride(2)))
            _plan(ops, c, o, kw)
            ops.attention(q, k, v, o, tag="cond", **kw)
            assert g.guard_intact() and bool(torch.isfinite(o.float()).all()), (c["name"], "NaN" if extra else "zeros")
            assert flagged is None or torch.equal(kw["bound"][2] != 0, flagged)
            outs.append(o.clone())
        assert torch.equal(outs[0], outs[1]), f"{c['name']}: the output depends on what lies behind the last row or in the row padding"


def test_attn_kv_mix_ignores_what_surrounds_its_inputs(ops, dev):
    """The row clamp in stage_kv: rows past Skv - 1 of an identity's K and V are never fetched."""
    for name in C.MIX_POISON:
        c = next(c for c in C.MIX_CASES if c["name"] == name)
        assert c["Skv"] % 32
        d = C.mix_case_data(c, dev)
        outs = []
        for extra, fill in ((0, 0.0), (3, NAN)):
            q, k, v, g, z, kw = _mix_layout(c, d, dev, surround=(8, extra, fill))
            _mix_launch(ops, c, d, q, k, v, z, kw, dev)
            assert g.guard_intact() and bool(torch.isfinite(z.float()).all()), (name, "NaN" if extra else "zeros")
            outs.append(z.clone())
        assert torch.equal(outs[0], outs[1]), f"{name}: z depends on what lies behind the last key or in the row padding"


def test_attn_tiny_ignores_the_rows_of_no_group(ops, dev):
    for name in C.TINY_POISON:
        c = next(c for c in C.TINY_CASES if c["name"] == name)
        d, rows, idx = C.tiny_case_data(c)
        outs = []
        for fill in (0.0, NAN):
            qkv, q, k, v, g, o = _tiny_layout(c, d, rows, idx, dev, fill=fill)
            _tiny_launch(ops, c, qkv, q, k, v, o)
            assert g.guard_intact() and bool(torch.isfinite(o.float()).all()), (name, fill)
            outs.append(o.clone())
        assert torch.equal(outs[0], outs[1]), f"{name}: the output depends on rows of no group or on the columns no head owns"
