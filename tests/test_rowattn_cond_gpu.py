"""GPU: the softmax of the router's fused row kernels on hard score rows (tests/cond_rowattn.py): bya_router_group_attn (both
rowattn512_kernel instances) and bya_router_group_attn_out, at the production scale 0.125, every output element against the fp64
softmax of the designed q, k, v under cond_attn's bars, the kernel and schedule of every case asserted through the plan queries
BEFORE the launch, inside a NaN-poisoned view with a sentinel guard band, strided x, the chain in place."""
import pytest
import torch

import cond_rowattn as R
import exact_rowk as xr
from exact_gemm import POISON
from exact_rowk import BF, GuardedOut, bad_elements, describe, strided

pytestmark = pytest.mark.gpu
ids = lambda c: c["name"]


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _x(x, c, dev):
    x = strided(x.to(dev), c["pad"])
    assert x.stride(0) in (640, 768)
    return x


def _touched(dat, dev):
    t = torch.zeros(dat["M"], dtype=torch.bool, device=dev)
    t[dat["rows"].reshape(-1).to(dev)] = True
    return t


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_group_attn_plan(ops, c, x, out):
    plan = ops.router_group_attn_plan(x, *xr.geometry(c), out=out)
    assert {k: plan[k] for k in ("P", "G", "wide", "tiles")} == R.expected_plan(c), plan
    assert (plan["tiles"] / 16 * 8 > plan["blocks"]) == c["multi"], plan
    return plan


def _assert_chain_plan(ops, c, x):
    plan = ops.router_group_attn_out_plan(x, *xr.geometry(c), tiles_pass0=c["tp0"])
    assert (plan["tiles"], plan["tp0"], plan["passes"]) == R.expected_chain_plan(c), plan
    return plan


@pytest.mark.parametrize("c", R.GROUP_ATTN_CASES, ids=ids)
def test_router_group_attn_cond(ops, dev, c):
    dat = R.case_data(c)
    M, geo = c["M"], xr.geometry(c)
    x, pack, out = _x(dat["x"], c, dev), R.pack(ops, dat, dev), GuardedOut(M, 512, dev)
    plan = _assert_group_attn_plan(ops, c, x, out.view())
    ops.router_group_attn(x, pack, out.view(), *geo, eps=R.EPS_ATTN, scale=R.SCALE)
    torch.cuda.synchronize()
    assert out.guard_intact(), f"{c['name']} [plan {plan}]: the guard band around the output was written"
    rest = _bits(out.view())[~_touched(dat, dev)]
    assert bool((rest == POISON).all()), f"{c['name']} [plan {plan}]: rows outside the groups were written"
    got = R.per_head(out.view(), dat["rows"].to(dev)).cpu()
    R.check(c["name"], got, dat, plan=plan)


@pytest.mark.parametrize("c", R.ATTN_OUT_CASES, ids=ids)
def test_router_group_attn_out_cond(ops, dev, c):
    dat = R.chain_case_data(c)
    M, geo = c["M"], xr.geometry(c)
    x, pack = _x(dat["x"], c, dev), R.pack(ops, dat, dev)
    pack_o = ops.pack_rowgemm512(dat["wo"].to(dev), dat["bo"].to(dev))
    plan = _assert_chain_plan(ops, c, x)
    rows = dat["rows"].reshape(-1).to(dev)
    # the two launches first: x is still the input
    a = torch.zeros(M, 512, dtype=BF, device=dev)
    two = torch.zeros(M, 512, dtype=BF, device=dev)
    ops.router_group_attn(x, pack, a, *geo, eps=R.EPS_ATTN, scale=R.SCALE)
    ops.rowgemm512(a, pack_o, two, res=x)
    ops.router_group_attn_out(x, pack, pack_o, *geo, eps=R.EPS_ATTN, scale=R.SCALE, tiles_pass0=c["tp0"])      # in place
    torch.cuda.synchronize()
    assert not bool(x._base[:, 512:].any()), f"{c['name']} [plan {plan}]: the padding between the rows of x was written"
    rest = ~_touched(dat, dev)
    assert torch.equal(_bits(x)[rest], _bits(dat["x"].to(dev))[rest]), f"{c['name']} [plan {plan}]: rows outside the groups changed"
    R.chain_check(c["name"], x[rows], dat, plan=plan)
    bad = bad_elements(x[rows], two[rows])
    assert not bool(bad.any()), f"{c['name']} [plan {plan}] chain against its two launches: {describe(bad, x[rows], two[rows])}"


def _hostile(x, rest):
    """x with the rows ``rest`` filled with NaN, +inf, -inf and the largest bf16, in turn."""
    fill = torch.tensor([float("nan"), float("inf"), float("-inf"), 3.3895313892515355e38], dtype=BF, device=x.device)
    x = x.clone()
    idx = rest.nonzero()[:, 0]
    x[idx] = fill[(idx[:, None] + torch.arange(512, device=x.device)[None, :]) % 4]
    return x


def _zeroed(x, rest):
    x = x.clone()
    x[rest] = 0
    return x


@pytest.mark.parametrize("c", R.NO_GROUP_CASES + R.NO_GROUP_OUT_CASES, ids=ids)
def test_router_group_attn_ignores_the_rows_of_no_group(ops, dev, c):
    """include/bya.h: rows outside every group are neither read nor written.  With NaN, inf and the largest bf16 in them the group
    rows come out bit for bit as with zeros in them (and, in place, they stay what they were)."""
    chain = c["tp0"] is not None
    dat = R.chain_case_data(c) if chain else R.case_data(c)
    M, geo = c["M"], xr.geometry(c)
    rest = ~_touched(dat, dev)
    assert 3 <= int(rest.sum()) <= 5
    pack = R.pack(ops, dat, dev)
    rows = dat["rows"].reshape(-1).to(dev)
    outs = []
    for make in (_zeroed, _hostile):
        x0 = make(dat["x"].to(dev), rest)
        x = _x(x0, c, dev)
        if chain:
            plan = _assert_chain_plan(ops, c, x)
            pack_o = ops.pack_rowgemm512(dat["wo"].to(dev), dat["bo"].to(dev))
            ops.router_group_attn_out(x, pack, pack_o, *geo, eps=R.EPS_ATTN, scale=R.SCALE, tiles_pass0=c["tp0"])
            torch.cuda.synchronize()
            assert torch.equal(_bits(x)[rest], _bits(x0)[rest]), f"{c['name']} [plan {plan}]: rows outside the groups changed"
            outs.append(x[rows])
        else:
            out = GuardedOut(M, 512, dev)
            plan = _assert_group_attn_plan(ops, c, x, out.view())
            ops.router_group_attn(x, pack, out.view(), *geo, eps=R.EPS_ATTN, scale=R.SCALE)
            torch.cuda.synchronize()
            assert out.guard_intact() and bool((_bits(out.view())[rest] == POISON).all()), f"{c['name']} [plan {plan}]"
            outs.append(out.view()[rows])
    assert bool(torch.isfinite(outs[0].float()).all())
    bad = bad_elements(outs[1], outs[0])
    assert not bool(bad.any()), f"{c['name']} [plan {plan}] hostile rows of no group against zeros there: {describe(bad, outs[1], outs[0])}"
