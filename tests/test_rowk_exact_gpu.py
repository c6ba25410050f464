"""GPU: the router's K = 512 row kernels on exact data (tests/exact_rowk.py): bit equality with an fp64 reference inside a
NaN-poisoned view with a sentinel guard band, strided x, residual in place, and the kernel path of every case asserted through
the host-side plan queries BEFORE the launch -- a retuned threshold fails here instead of moving a case onto another kernel."""
import pytest
import torch

import exact_rowk as xr
from exact_gemm import POISON
from exact_rowk import GuardedOut, assert_exact, strided

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _pack(ops, dat, dev, w="w", b="b", ln=True):
    """ops.pack_rowgemm512 of the un-folded Linear; its fold must be the exact one (integers / halves in fp32)."""
    gamma, beta = (dat["gamma"], dat["beta"]) if ln else (None, None)
    pack = ops.pack_rowgemm512(dat[w].to(dev), dat[b].to(dev), None if gamma is None else gamma.to(dev),
                               None if beta is None else beta.to(dev))
    if gamma is not None:
        wg = dat[w].double() * gamma.double()
        assert torch.equal(pack["w"].cpu().double(), wg) and torch.equal(pack["colsum"].cpu().double(), wg.sum(1))
        assert torch.equal(pack["cvec"].cpu().double(), dat[w].double() @ beta.double() + dat[b].double())
    return pack


def _x(dat, c, dev):
    x = strided(dat["x"].to(dev), c["pad"])
    assert x.stride(0) in (640, 768)
    return x


@pytest.mark.parametrize("c", xr.ROWGEMM_CASES, ids=lambda c: c["name"])
def test_rowgemm512_exact(ops, dev, c):
    M, N = c["M"], c["N"]
    folded = c["ln"] or c["gelu"]
    dat = xr.folded_data(M, N, c["ln"], c["gelu"], c["res"], xr.seed_of(c)) if folded else xr.plain_data(M, N, c["res"], xr.seed_of(c))
    if folded:
        xr.assert_fold_conditions(dat)
    x, pack, out = _x(dat, c, dev), _pack(ops, dat, dev, ln=c["ln"]), GuardedOut(M, N, dev)
    act = "gelu_erf" if c["gelu"] else None
    with ops.options(reference_forms="rowgemm_chunked" if c["chunked"] else []):
        plan = ops.rowgemm512_plan(x, N, out=out.view(), ln=c["ln"], res=out.view() if c["res"] else None, act=act)
        assert (plan["form"], plan["ln"], plan["res"], plan["gelu"]) == (c["form"], c["ln"], c["res"], c["gelu"]), plan
        assert c["crosses"] is None or plan["crosses_row_block"] == c["crosses"], plan
        if c["res"]:
            out.fill(dat["r"].to(dev))
        ops.rowgemm512(x, pack, out.view(), res=out.view() if c["res"] else None, act=act, eps=xr.EPS_LN)
        torch.cuda.synchronize()
    assert_exact(out.view(), dat["ref"].to(dev), plan, c["name"])
    assert out.guard_intact(), f"{c['name']} [plan {plan}]: the guard band around the output was written"


@pytest.mark.parametrize("c", xr.MLP_CASES, ids=lambda c: c["name"])
def test_router_mlp_fused_exact(ops, dev, c):
    M = c["M"]
    dat = xr.mlp_data(M, xr.seed_of(c))
    xr.assert_fold_conditions(dat)
    x, out = _x(dat, c, dev), GuardedOut(M, 512, dev)
    pack1 = _pack(ops, dat, dev)
    pack2 = ops.pack_rowgemm512(dat["w2"].to(dev), dat["b2"].to(dev))
    plan = ops.router_mlp_fused_plan(x, out=out.view(), tiles_pass0=c["tp0"])
    assert plan["tiles"] == (M + 15) // 16 and (c["tp0"] == 0 or plan["tp0"] == c["tp0"]), plan
    ops.router_mlp_fused(x, pack1, pack2, eps=xr.EPS_LN, out=out.view(), tiles_pass0=c["tp0"])
    torch.cuda.synchronize()
    assert_exact(out.view(), dat["ref"].to(dev), plan, c["name"])
    assert out.guard_intact(), f"{c['name']} [plan {plan}]: the guard band around the output was written"


def _untouched_keep_poison(out, rows, M, what):
    """Rows outside every group were never written: they still hold the view's NaN poison."""
    touched = torch.zeros(M, dtype=torch.bool, device=out.buf.device)
    touched[rows.reshape(-1).to(out.buf.device)] = True
    rest = out.view().view(torch.int16)[~touched]
    assert bool((rest == POISON).all()), f"{what}: rows outside the groups were written"


@pytest.mark.parametrize("c", xr.GROUP_ATTN_CASES, ids=lambda c: c["name"])
def test_router_group_attn_exact(ops, dev, c):
    M, geo = c["M"], xr.geometry(c)
    dat = xr.attn_data(c["kind"], *geo, M, xr.seed_of(c))
    xr.assert_attn_conditions(dat)
    x, pack, out = _x(dat, c, dev), _pack(ops, dat, dev), GuardedOut(M, 512, dev)
    plan = ops.router_group_attn_plan(x, *geo, out=out.view())
    L = c["L"]
    assert (plan["P"], plan["wide"]) == (16 if L > 8 else 1 << (L - 1).bit_length(), L > 16), plan
    ops.router_group_attn(x, pack, out.view(), *geo, eps=xr.EPS_ATTN, scale=xr.UNIT_SCALE)
    torch.cuda.synchronize()
    rows = dat["rows"].to(dev)
    assert_exact(out.view()[rows.reshape(-1)], dat["want"].reshape(-1, 512).to(dev), plan, c["name"])
    _untouched_keep_poison(out, dat["rows"], M, c["name"])
    assert out.guard_intact(), f"{c['name']} [plan {plan}]: the guard band around the output was written"


@pytest.mark.parametrize("c", xr.ATTN_OUT_CASES, ids=lambda c: c["name"])
def test_router_group_attn_out_exact(ops, dev, c):
    M, geo = c["M"], xr.geometry(c)
    dat = xr.attn_data(c["kind"], *geo, M, xr.seed_of(c), chain=True)
    xr.assert_attn_conditions(dat)
    x, pack, out = _x(dat, c, dev), _pack(ops, dat, dev), GuardedOut(M, 512, dev)
    pack_o = ops.pack_rowgemm512(dat["wo"].to(dev), dat["bo"].to(dev))
    plan = ops.router_group_attn_out_plan(x, *geo, out=out.view(), tiles_pass0=c["tp0"])
    assert c["tp0"] == 0 or plan["tp0"] == c["tp0"], plan
    ops.router_group_attn_out(x, pack, pack_o, *geo, eps=xr.EPS_ATTN, scale=xr.UNIT_SCALE, out=out.view(), tiles_pass0=c["tp0"])
    torch.cuda.synchronize()
    rows = dat["rows"].to(dev)
    assert_exact(out.view()[rows.reshape(-1)], dat["ref"].to(dev), plan, c["name"])
    _untouched_keep_poison(out, dat["rows"], M, c["name"])
    assert out.guard_intact(), f"{c['name']} [plan {plan}]: the guard band around the output was written"
