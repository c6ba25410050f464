"""Every attention kernel path on exact data (tests/exact_attn.py): build the data, ask the plan, assert the plan is the one the
case is meant to reach, launch into a guarded output, compare bit for bit with the closed form; the guard band must be intact
and no poison may be left inside.  The data condition that makes equality the right bar is checked on the CPU
(test_attn_exact_cpu.py); the matrix is shared with that file."""
import pytest
import torch

import exact_attn as X
from exact_attn import BF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def _forms(*names):
    return [n for n in names if n]


def attn_layout(c, d, dev):
    """The case's tensors in the layout of bya_attn_fwd: q [B, Sq, H D] (shared by the L2 level-2 batches: stride 0), k, v
    [B, L2, Skv, H D], rows ``pad`` elements wider; the guarded output [B L2, Sq, H D]; strides; the expected output."""
    B, H, L2, Sq, Skv, D = c["B"], c["H"], c["L2"], c["Sq"], c["Skv"], c["D"]
    q = X.strided(d["q"].view(B, H, Sq, D).permute(0, 2, 1, 3).reshape(B, Sq, H * D).to(BF), c["pad"])
    k = X.strided(d["k"].view(B, H, L2, Skv, D).permute(0, 2, 3, 1, 4).reshape(B, L2, Skv, H * D).to(BF), c["pad"])
    v = X.strided(d["v"].view(B, H, L2, Skv, D).permute(0, 2, 3, 1, 4).reshape(B, L2, Skv, H * D).to(BF), c["pad"])
    want = d["want"].view(B, H, L2, Sq, D).permute(0, 2, 3, 1, 4).reshape(B * L2, Sq, H * D)
    g = X.GuardedOut(Sq, H * D, dev, batch=B * L2, col0=c["col0"])
    o = g.bf[:, g.r0:g.r0 + Sq, g.c0:g.c0 + H * D]
    kw = dict(head_dim=D, heads=H, nb1=B, nb2=L2, Sq=Sq, Skv=Skv, q_strides=(q.stride(0), 0, q.stride(1)),
              k_strides=(k.stride(0), k.stride(1), k.stride(2)), v_strides=(v.stride(0), v.stride(1), v.stride(2)),
              o_strides=(L2 * o.stride(0), o.stride(0), o.stride(1)))
    kind = c["kind"]
    flagged = None
    if kind in ("run", "d128"):
        kw.update(scale=X.UNIT_SCALE)
    elif kind == "pre":
        kw.update(scale=1.0, prescaled=True)
    elif kind == "w4":
        kw.update(scale=1.0, prescaled=True, score_bound=X.BOUND)
    else:
        # squared norms as bya_qknorm_rope would leave them: sqrt(q2 k2) = 80 <= 90 (static kernel) or 100 (flagged: the
        # running-maximum kernel behind it computes the head); the larger of the two slots counts
        nbh = B * L2 * H
        flagged = torch.arange(nbh, device=dev) % 3 == 1
        stats = torch.full((2, 2, nbh + 5), 1.0, device=dev)
        stats[1, :, 2:2 + nbh] = torch.where(flagged, 100.0, 80.0)
        flags = torch.full((nbh,), -7, dtype=torch.int32, device=dev)
        kw.update(scale=1.0, prescaled=True, bound=(stats, 2, flags))
    return q, k, v, g, o, want, kw, flagged


@pytest.mark.parametrize("case", X.ATTN_CASES, ids=[c["name"] for c in X.ATTN_CASES])
def test_attn_fwd_exact(ops, dev, case):
    c = case
    d = X.attn_case_data(c, dev)
    assert d["lo"] >= -X.BOUND and d["top"] <= X.BOUND or c["kind"] in ("run", "pre", "d128")
    q, k, v, g, o, want, kw, flagged = attn_layout(c, d, dev)
    with ops.options(attn_streamk=c["sk_opt"], reference_forms=_forms("attn_narrow_store" if c["narrow"] else None)):
        plan = ops.attention_plan(o, **kw)
        key = ops.attention_plan_key(plan)
        assert key == X.attn_case_key(c), (key, plan)
        assert plan["q_tile"] == (512 if c["kind"] in ("w4", "dev") else 128) and plan["second_launch"] == (c["kind"] == "dev")
        reps = 4 if plan["stream_k"] else 1              # the hand-off flags must be back at 0 after every launch
        for rep in range(reps):
            if rep:
                g.bf[:, g.r0:g.r0 + c["Sq"], g.c0:g.c0 + c["H"] * c["D"]] = float("nan")
            ops.attention(q, k, v, o, tag="exact", **kw)
            X.assert_exact(o, want, what=f"{c['name']} launch {rep} [plan {key} {plan}] (batch, row, head * {c['D']} + col)")
    assert g.guard_intact(), f"{c['name']} [plan {key}]: wrote outside its output view"
    if flagged is not None:
        flags = kw["bound"][2]
        assert torch.equal(flags != 0, flagged) and bool((flags != -7).all()), (flags.tolist(), flagged.tolist())
    if plan["stream_k"]:
        assert ops.attn_workspace_status() == 0


def test_attn_stream_k_equals_one_workgroup_per_item_bit_for_bit(ops, dev):
    """On exact data the cut items too are bit-identical between the two grids (both equal the closed form)."""
    c = next(c for c in X.ATTN_CASES if c["name"] == "w4-streamk-5056x32")
    d = X.attn_case_data(c, dev)
    q, k, v, g, o, want, kw, _ = attn_layout(c, d, dev)
    outs = []
    for opt in (1, 0):
        with ops.options(attn_streamk=opt):
            assert ops.attention_plan(o, **kw)["stream_k"] == opt
            o.fill_(float("nan"))
            ops.attention(q, k, v, o, tag="exact", **kw)
            outs.append(o.clone())
    assert torch.equal(outs[0], outs[1]) and ops.attn_workspace_status() == 0
    X.assert_exact(outs[0], want, what="stream-K grid")


@pytest.mark.parametrize("case", X.MIX_CASES, ids=[c["name"] for c in X.MIX_CASES])
def test_attn_kv_mix_exact(ops, dev, case):
    c = case
    G, H, n_id, Sq, Skv, D = c["grp"], c["H"], c["n_id"], c["Sq"], c["Skv"], c["D"]
    d = X.mix_case_data(c, dev)
    q = X.strided(d["q"].view(G, H, Sq, D).permute(0, 2, 1, 3).reshape(G, Sq, H * D).to(BF), c["pad"])
    k = X.strided(d["k"].view(G, H, n_id, Skv, D).permute(2, 0, 3, 1, 4).reshape(n_id, G, Skv, H * D).to(BF), c["pad"])
    v = X.strided(d["v"].view(G, H, n_id, Skv, D).permute(2, 0, 3, 1, 4).reshape(n_id, G, Skv, H * D).to(BF), c["pad"])
    want = d["z_want"].view(G, H, Sq, D).permute(0, 2, 1, 3).reshape(G, Sq, H * D)
    g = X.GuardedOut(Sq, H * D, dev, batch=G, col0=c["col0"])
    z = g.bf[:, g.r0:g.r0 + Sq, g.c0:g.c0 + H * D]
    wsum = torch.full((G * Sq + 8,), -5.0, device=dev)
    kw = dict(head_dim=D, heads=H, n_id=n_id, n_grp=G, Sq=Sq, Skv=Skv, q_strides=(q.stride(0), q.stride(1)),
              k_strides=(k.stride(0), k.stride(1), k.stride(2)), v_strides=(v.stride(0), v.stride(1), v.stride(2)),
              z_strides=(z.stride(0), z.stride(1)), scale=X.UNIT_SCALE)
    with ops.options(reference_forms=_forms("kv_mix_generic" if c["generic"] else None)):
        plan = ops.attn_kv_mix_plan(z, d["af"], **kw)
        key = f"{plan['form']}_d{plan['head_dim']}" + ("+big_lds" if plan["big_lds"] else "")
        assert key == X.mix_case_key(c) and plan["form"] == c["form"], (key, plan)
        ops.attn_kv_mix(q, k, v, d["r"], d["af"], z, wsum[:G * Sq], **kw)
    X.assert_exact(z, want, what=f"{c['name']} [plan {plan}] (group, row, head * {D} + col)")
    assert g.guard_intact(), f"{c['name']}: wrote outside z"
    bad = (wsum[:G * Sq] != d["wsum"]).nonzero()
    assert bad.numel() == 0, f"{c['name']}: wsum differs at {bad[:4].flatten().tolist()}"
    assert bool((wsum[G * Sq:] == -5.0).all())


@pytest.mark.parametrize("case", X.TINY_CASES, ids=[c["name"] for c in X.TINY_CASES])
def test_attn_tiny_exact(ops, dev, case):
    c = case
    L, H, no, ni = c["L"], c["H"], c["n_outer"], c["n_inner"]
    d, rows, idx = X.tiny_case_data(c, dev)
    groups, W = no * ni, H * 64
    col0 = 4 if c["unaligned"] else 0
    extra = 3                                                       # rows of no group: sentinel in q | k | v, untouched in o
    qkv = torch.full((rows + extra, 3 * W + 8), 1.0, dtype=BF, device=dev)
    for t, name in enumerate(("q", "k", "v")):
        src = d[name].reshape(groups, H, L, 64).permute(0, 2, 1, 3).reshape(groups * L, W).to(BF)
        qkv[idx.reshape(-1), col0 + t * W:col0 + (t + 1) * W] = src
    want = torch.zeros(rows + extra, W, device=dev)
    want[idx.reshape(-1)] = d["want"].reshape(groups, H, L, 64).permute(0, 2, 1, 3).reshape(groups * L, W)
    g = X.GuardedOut(rows + extra, W, dev, col0=8 if not c["unaligned"] else 4)
    o = g.view()
    o[rows:] = 3.0
    want[rows:] = 3.0
    q, k, v = (qkv[:, col0 + t * W:col0 + (t + 1) * W] for t in range(3))
    outer_stride = L * ni if c["temporal"] else 0
    plan = ops.attn_tiny_plan(q, k, v, o, L, H, no, ni, qkv.stride(0), o.stride(0))
    assert plan["instance"] == c["instance"], plan
    assert plan["waves"] == groups * (H // 8 if plan["instance"].startswith("tiny8") else H)
    ops.attn_tiny(q, k, v, o, L, H, no, ni, outer_stride, ni, qkv.stride(0), o.stride(0), X.LN2)
    X.assert_exact(o, want, what=f"{c['name']} [plan {plan}] (row, head * 64 + col)")
    assert g.guard_intact(), f"{c['name']}: wrote outside its output"

