"""CPU: the data conditions behind tests/test_rowk_exact_gpu.py, the kernel paths its case table reaches (through the host-side
plan queries), and planted faults that the exact check catches and the relative-Frobenius bar of test_kernels_gpu.py lets pass."""
import numpy as np
import pytest
import torch

import exact_rowk as xr
from exact_rowk import BF, bad_elements


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def _linear_data(c):
    if c["ln"] or c["gelu"]:
        return xr.folded_data(c["M"], c["N"], c["ln"], c["gelu"], c["res"], xr.seed_of(c))
    return xr.plain_data(c["M"], c["N"], c["res"], xr.seed_of(c))


# ------------------------------------------------------------------------------------------------------------ data conditions
@pytest.mark.parametrize("c", xr.ROWGEMM_CASES, ids=lambda c: c["name"])
def test_linear_data_is_exact_for_every_element(c):
    """Integer pre-activations with 14 <= |y| < 256, and the kernel's fp32 expression with rstd one ulp either side, contracted
    or not, rounds to the reference's bf16 on EVERY element; the plain cases stay below 2^24 units of 2^-3."""
    dat = _linear_data(c)
    ref = dat["ref"].to(BF)
    if not (c["ln"] or c["gelu"]):
        assert torch.equal(dat["ref"] * 8, (dat["ref"] * 8).round()) and float(dat["ref"].abs().max()) * 8 < 2 ** 24
        return
    xr.assert_fold_conditions(dat)
    for ulp in (-1, 0, 1):
        for fma in (False, True):
            got = xr.emulate_fold(dat, ulp, fma)
            assert not bool(bad_elements(got, ref).any()), (c["name"], ulp, fma)


@pytest.mark.parametrize("M", sorted({c["M"] for c in xr.MLP_CASES}))
def test_mlp_data_is_exact(M):
    c = next(c for c in xr.MLP_CASES if c["M"] == M)
    dat = xr.mlp_data(M, xr.seed_of(c))
    xr.assert_fold_conditions(dat)
    hidden = dat["h"].to(BF)
    for ulp in (-1, 1):
        for fma in (False, True):
            assert not bool(bad_elements(xr.emulate_fold(dat, ulp, fma), hidden).any())
    assert torch.equal(dat["ref"] * 4, (dat["ref"] * 4).round()) and float(dat["ref"].abs().max()) * 4 < 2 ** 24
    assert np.float32(1.0) + np.float32(xr.EPS_ATTN) == np.float32(1.0) and xr.EPS_ATTN > 0      # d^2 + EPS_ATTN == d^2 in fp32


@pytest.mark.parametrize("c", xr.GROUP_ATTN_CASES + xr.ATTN_OUT_CASES, ids=lambda c: c["name"])
def test_attention_data_has_its_closed_form(c):
    dat = xr.attn_data(c["kind"], *xr.geometry(c), c["M"], xr.seed_of(c), chain=c["tp0"] is not None)
    xr.assert_attn_conditions(dat)
    ref, want = xr.attn_reference64(dat), dat["want"]
    assert bool(((ref - want).abs() <= 2.0 ** -16 * want.abs()).all())
    if c["tp0"] is not None:
        assert torch.equal(dat["ref"] * 64, (dat["ref"] * 64).round()) and float(dat["ref"].abs().max()) * 64 < 2 ** 24


# ------------------------------------------------------------------------------------------------------------ coverage
def test_case_table_covers_every_path(ops):
    cells = {}

    def fill(cell, name):
        cells.setdefault(cell, name)

    for c in xr.ROWGEMM_CASES:
        with ops.options(reference_forms="rowgemm_chunked" if c["chunked"] else []):
            p = ops.rowgemm512_plan(c["M"], c["N"], ln=c["ln"], res=True if c["res"] else None, act="gelu_erf" if c["gelu"] else None)
        assert p["form"] == c["form"], (c["name"], p)
        fill((p["form"], p["ln"], p["res"], p["gelu"]), c["name"])
        if p["crosses_row_block"]:
            fill("range crosses a row block", c["name"])
        if p["form"] == "chunk_balanced" and p["work_items"] > p["grid"]:
            fill("more work items than workgroups", c["name"])
        if p["form"] == "chunk_balanced" and c["N"] == 512 and not c["ln"] and c["M"] >= 2048:
            fill("N = 512 at M >= 2048 on the chunk-balanced kernel", c["name"])
        if p["form"] == "w_stationary":
            share = xr.wstat_wave_tiles(c["M"])
            assert sum(share) == (c["M"] + 15) // 16
            for n, what in ((0, "wave with no tile"), (1, "wave with one tile")):
                if n in share:
                    fill(what, c["name"])
            if any(n > 1 and n % 2 for n in share):
                fill("wave with an odd number of tiles", c["name"])
            if c["M"] % 16 in (1, 15):
                fill(f"last tile of {c['M'] % 16} rows", c["name"])
    for c in xr.MLP_CASES:
        p = ops.router_mlp_fused_plan(c["M"], tiles_pass0=c["tp0"])
        fill(f"mlp chain: {p['passes']} passes", c["name"])
        fill(f"mlp chain: tp0 {p['tp0']}", c["name"])
        if p["passes"] > 1 and p["wgs_last"] * 2 < p["grid"]:
            fill("mlp chain: remainder pass with most workgroups idle", c["name"])
    for c in xr.ATTN_OUT_CASES:
        p = ops.router_group_attn_out_plan(c["M"], *xr.geometry(c), tiles_pass0=c["tp0"])
        fill(f"attention chain: {p['passes']} passes", c["name"])
        fill(f"attention chain: L {c['L']}", c["name"])
        fill(f"attention chain: tiles_pass0 {c['tp0']}", c["name"])
    for c in xr.GROUP_ATTN_CASES:
        p = ops.router_group_attn_plan(c["M"], *xr.geometry(c))
        fill(f"group attention {c['kind']}: L {c['L']}", c["name"])
        fill("group attention: wide" if p["wide"] else f"group attention: P {p['P']}", c["name"])
        if not p["wide"] and (c["n_outer"] * c["n_inner"]) % p["G"]:
            fill("group attention: ragged tail", c["name"])
        if c["geom"] == "trailing+5":
            fill("group attention: rows outside every group", c["name"])
    want = [("chunk_balanced", ln, res, gelu) for ln, res, gelu in xr.INSTANCES]
    want += [("w_stationary", False, res, gelu) for res in (False, True) for gelu in (False, True)]
    want += ["range crosses a row block", "more work items than workgroups", "N = 512 at M >= 2048 on the chunk-balanced kernel",
             "wave with no tile", "wave with one tile", "wave with an odd number of tiles", "last tile of 1 rows", "last tile of 15 rows",
             "mlp chain: 1 passes", "mlp chain: 2 passes", "mlp chain: 3 passes", "mlp chain: remainder pass with most workgroups idle"]
    want += [f"mlp chain: tp0 {t}" for t in range(1, 9)]
    want += ["attention chain: 1 passes", "attention chain: 2 passes"] + [f"attention chain: L {L}" for L in (1, 2, 3, 13, 16)]
    want += [f"attention chain: tiles_pass0 {t}" for t in (0, 1, 6)]
    want += [f"group attention uniform: L {L}" for L in (1, 2, 4, 8, 16)]
    want += [f"group attention levels: L {L}" for L in (2, 3, 13, 16, 17, 25, 32)]
    want += [f"group attention: P {P}" for P in (1, 2, 4, 8, 16)]
    want += ["group attention: wide", "group attention: ragged tail", "group attention: rows outside every group"]
    for cell in want:
        print(f"{cell!s:70} {cells.get(cell, '-- EMPTY --')}")
    assert not [cell for cell in want if cell not in cells]


def test_plan_queries_take_tensors_and_shapes(ops):
    x = xr.strided(torch.empty(2049, 512, dtype=BF, device="meta"), 256)
    out = xr.GuardedOut(2049, 512, "meta")
    assert ops.rowgemm512_plan(x, 512, out=out.view(), res=out.view()) == ops.rowgemm512_plan(2049, 512, res=True)
    assert ops.rowgemm512_plan(2047, 512)["form"] == "chunk_balanced" and ops.rowgemm512_plan(65537, 512)["form"] == "chunk_balanced"
    assert ops.rowgemm512_plan(65536, 512)["form"] == "w_stationary" and ops.rowgemm512_plan(4394, 512, ln=True)["form"] == "chunk_balanced"
    assert ops.router_mlp_fused_plan(x, out=out.view(), tiles_pass0=3) == ops.router_mlp_fused_plan(2049, tiles_pass0=3)
    assert ops.router_mlp_fused_plan(35100) == dict(tiles=2194, tp0=8, grid=256, passes=2, tiles_last=1, wgs_last=146)
    with pytest.raises(Exception):
        ops.router_group_attn_out_plan(2250, 25, 2, 45, 25 * 45, 45)             # longer than one tile: the chain refuses
    with pytest.raises(Exception):
        ops.rowgemm512_plan(x, 512, out=out.view()[:, 4:])                        # shape / alignment are checked like a launch


# ------------------------------------------------------------------------------------------------------------ planted faults
def rel_fro(a, b):
    return float((a - b).norm() / b.norm())


class Model:
    """fp64 model of  rstd * (x . Wg^T - mean * s) + c  [-> GELU -> . W2^T + b2 + x]  on 16-row tiles with fault hooks."""

    def __init__(self, x, wg, c, w2=None, b2=None):
        self.x, self.wg, self.c, self.w2, self.b2 = x.double(), wg.double(), c.double(), w2, b2
        self.mean = self.x.mean(1, keepdim=True)
        self.rstd = 1.0 / (self.x.var(1, unbiased=False, keepdim=True)).sqrt()
        self.s = self.wg.sum(1)
        self.odd_one = 3                         # the tile row whose mean the "mean" fault takes from its neighbour

    def first(self, rows, fault=None, rounded=False):
        """``rounded``: the reference's own bf16 op chain (LayerNorm output and Linear output rounded) instead of the fold."""
        x, mean, rstd = self.x[rows], self.mean[rows], self.rstd[rows]
        if rounded:
            return (((x - mean) * rstd).to(BF).double() @ self.wg.T + self.c).to(BF).double()
        acc = x @ self.wg.T
        if fault == "k-step":
            acc[:, 64:80] -= x[:, 96:128] @ self.wg[64:80, 96:128].T             # one MFMA: k-step 3 of a 16-column block
        if fault == "mean":
            mean = mean.clone()
            mean[self.odd_one] = self.mean[rows[self.odd_one] ^ 1]
        if fault == "rstd":
            rstd = self.rstd[rows + 16]
        return rstd * (acc - mean * self.s) + self.c

    def chain(self, rows, fault=None, rounded=False):
        r_ = (lambda t: t.to(BF).double()) if rounded else (lambda t: t)
        h = xr.gelu64(self.first(rows, rounded=rounded)).to(BF).double()
        y = r_(h @ self.w2.double().T + self.b2.double())
        if fault == "fragment":                  # chunk 3's fragment u = 0 (hidden columns 192 .. 223) met k-step 7 instead of 6
            y += h[:, 192:224] @ (self.w2.double()[:, 224:256] - self.w2.double()[:, 192:224]).T
        return r_(y + self.x[rows])


def _realistic(M, seed):
    """test_kernels_gpu.py's data -- gaussian rows with a common offset, gaussian weights -- with row scales within 2 % of
    each other (rows whose statistics are similar, as the router's are after a LayerNorm'd residual stream)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, 512, generator=g) * (0.98 + 0.04 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g) * 0.1).to(BF)
    w = (torch.randn(512, 512, generator=g) * 512 ** -0.5).to(BF)
    w2 = (torch.randn(512, 512, generator=g) * 512 ** -0.5).to(BF)
    return x, w, 0.2 * torch.randn(512, generator=g), w2, 0.2 * torch.randn(512, generator=g)


TILE = torch.arange(32, 48)


@pytest.fixture(scope="module")
def bars():
    """The old bar's two sides at 35100 rows, once: the truth, the reference's own bf16 chain, and the norms."""
    M = 35100
    x, w, b, w2, b2 = _realistic(M, 5)
    m = Model(x, w, b, w2, b2)
    rows = torch.arange(M - 16)
    out = {}
    for name, fn in (("linear", m.first), ("chain", m.chain)):
        truth = fn(rows)
        out[name] = dict(truth=truth, got=truth.to(BF).double(), model=m, e_ref=rel_fro(fn(rows, rounded=True), truth))
    return out


@pytest.mark.parametrize("fault,stage", [("k-step", "linear"), ("mean", "linear"), ("rstd", "linear"), ("unwritten", "linear"),
                                         ("fragment", "chain")])
def test_planted_fault_fails_the_exact_check_and_passes_the_old_bar(bars, fault, stage):
    # (1) exact data: the fault changes bits
    if stage == "linear":
        dat = xr.folded_data(300, 512, True, False, False, 11)
        m = Model(dat["x"], dat["wg"], dat["c"])
        m.odd_one = next(i for i in range(16) if dat["mu"][TILE[i]] != dat["mu"][TILE[i] ^ 1])
        good, bad = m.first(TILE), m.first(TILE, fault)
    else:
        dat = xr.mlp_data(300, 11)
        m = Model(dat["x"], dat["wg"], dat["c"], dat["w2"], dat["b2"])
        good, bad = m.chain(TILE), m.chain(TILE, fault)
    assert not bool(bad_elements(good.to(BF), dat["ref"][TILE].to(BF)).any())            # the model is the reference
    if fault == "unwritten":
        bad = good.clone()
        bad[3, 70] = 0.0                         # what a fresh allocation holds
    n_bad = int(bad_elements(bad.to(BF), dat["ref"][TILE].to(BF)).sum())
    assert n_bad > 0
    # (2) realistic data at the router's row count: the same fault stays under  1.25 e_ref + 2e-4
    b = bars[stage]
    truth, got = b["truth"], b["got"].clone()
    e_ref = b["e_ref"]
    fn = b["model"].first if stage == "linear" else b["model"].chain
    got[TILE] = fn(TILE, None if fault == "unwritten" else fault).to(BF).double()
    if fault == "unwritten":
        got[35, 70] = 0.0
    assert not torch.equal(got, b["got"])
    e = rel_fro(got, truth)
    print(f"{fault}: {n_bad} exact elements differ; old bar: {e:.3e} <= 1.25 * {e_ref:.3e} + 2e-4")
    if fault == "fragment":
        # measured: 4.5e-3 against a bar of 3.7e-3 -- a whole tile's swapped fragment is the one planted fault that the old bar
        # does see at 35100 rows, by a factor of 1.2 (and no longer at twice the rows); only the exact half is asserted for it
        return
    assert e <= 1.25 * e_ref + 2e-4


def test_planted_unmasked_key_fails_the_exact_check_and_passes_the_old_bar():
    """One key of the NEXT group of the tile left unmasked for one group in one head (the kernel's unit of work)."""
    def attend(q, k, v, rows, leak=None):
        G, L = rows.shape
        qh, kh, vh = (t[rows].view(G, L, 8, 64).transpose(1, 2) for t in (q, k, v))
        s = qh @ kh.transpose(-1, -2)
        p = torch.exp2(s - s.max(-1, keepdim=True).values)
        o = (p @ vh) / p.sum(-1, keepdim=True)
        if leak is not None:
            g, r, h = leak
            kk, vv = (torch.cat([t[rows[g]], t[r:r + 1]])[:, 64 * h:64 * h + 64] for t in (k, v))
            s1 = qh[g, h] @ kk.T
            p1 = torch.exp2(s1 - s1.max(-1, keepdim=True).values)
            o[g, h] = (p1 @ vv) / p1.sum(-1, keepdim=True)
        return o.transpose(1, 2).reshape(G, L, 512)

    c = next(c for c in xr.GROUP_ATTN_CASES if c["name"].startswith("levels-L3"))
    dat = xr.attn_data(c["kind"], *xr.geometry(c), c["M"], xr.seed_of(c))
    rows = dat["rows"]
    bad = attend(dat["q"], dat["k"], dat["v"], rows, leak=(4, int(rows[5, 0]), 2))
    assert not bool(bad_elements(attend(dat["q"], dat["k"], dat["v"], rows).to(BF), dat["want"].to(BF)).any())
    n_bad = int(bad_elements(bad.to(BF), dat["want"].to(BF)).sum())
    assert n_bad > 0
    # realistic: the router's temporal geometry (2700 groups of 13 rows), gaussian q, k, v with scores of a few units
    rows = xr.group_rows(13, 2, 1350, 17550, 1350)
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(35100, 512, generator=g).to(BF).double() * s for s in (0.35, 0.35, 1.0))
    truth = attend(q, k, v, rows)
    ref16 = truth.to(BF).double()
    got = attend(q, k, v, rows, leak=(4, int(rows[5, 0]), 2)).to(BF).double()
    assert not torch.equal(got, ref16)
    e, e16 = rel_fro(got, truth), rel_fro(ref16, truth)
    print(f"unmasked key: {n_bad} exact elements differ; old bar {e:.3e} <= 1.25 * {e16:.3e} + 1e-3")
    assert e <= 1.25 * e16 + 1e-3
