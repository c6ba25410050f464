"""CPU: tests/cond_rowattn.py against itself -- the encoding gives the designed q, k, v (rebuilt here from the family tables, not
from Wg), the fold is exact and survives an rstd 2 ulps off, every case holds its families and keeps eps below cond_attn.EPS_MAX, the
case tables of test_rowattn_cond_gpu.py planned on meta tensors reach the kernels and schedules they name, the restatement passes
every bar and each planted fault fails the bar named beside it."""
import numpy as np
import pytest
import torch

import cond_attn as C
import cond_rowattn as R
import exact_rowk as xr
from exact_rowk import BF, bad_elements

ALL_CASES = R.GROUP_ATTN_CASES + [c for c in R.NO_GROUP_OUT_CASES if c["L"] == 13]       # every geometry the GPU file uses
ids = lambda c: c["name"]


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def test_every_gpu_geometry_is_checked_here():
    geos = {(xr.geometry(c), c["M"]) for c in ALL_CASES}
    assert {(xr.geometry(c), c["M"]) for c in R.ATTN_OUT_CASES + R.NO_GROUP_CASES + R.NO_GROUP_OUT_CASES} <= geos


# ------------------------------------------------------------------------------------------------------------ the encoding
def _designed(dat):
    """q and k of the rows of the groups from the family tables alone -> (q, k [groups, L, 8, 64] with NaN on the noise features)."""
    G, L = dat["rows"].shape
    fam, peak = dat["fam"], dat["peak"]
    q = torch.full((G, L, R.HEADS, R.D), float("nan"), dtype=torch.float64)
    k = q.clone()
    is_ = lambda *names: sum((fam == R.FAM_ID[n]) for n in names).bool()
    member = torch.arange(L)[None, :].expand(G, L)
    for h in range(R.HEADS):
        blk = R.blocks_of(h)
        for f in blk["const"]:
            q[:, :, h, f] = 7.5 * is_("shift-high").double() - 7.5 * is_("shift-low").double()
            k[:, :, h, f] = 5.5
        for f in blk["wide_a"]:
            q[:, :, h, f] = 7.5 * is_("wide", "large").double() + 2.0 * is_("shift-low", "shift-high").double()
        for f in blk["wide_b"]:
            q[:, :, h, f] = 7.5 * is_("large").double()
        for pk in range(3):
            for f in blk["peaks"][pk]:
                q[:, :, h, f] = 7.5 * (is_("peaked") & (peak == pk)).double()
                k[:, :, h, f] = 7.5 * (member == R.peaks_of(L)[pk]).double()
    return q, k


@pytest.mark.parametrize("c", ALL_CASES, ids=ids)
def test_encoding_gives_the_designed_values_and_survives_the_fold(c, ops):
    dat = R.case_data(c)
    rows, L = dat["rows"], c["L"]
    G = rows.shape[0]
    r = rows.reshape(-1)
    # x, and the kernel's view of it
    assert torch.equal(dat["x"].double(), (dat["mu"] + dat["d"] * dat["e"]).double())
    assert np.float32(1.0) + np.float32(R.EPS_ATTN) == np.float32(1.0) and R.EPS_ATTN > 0
    e = dat["e"]
    assert bool((e.abs() == 1).all()) and bool((e.sum(1) == 0).all())
    # e . Wg^T + c in fp64 is the designed q | k | v
    qkv = e.double() @ dat["wg"].T + dat["c"]
    assert torch.equal(qkv[:, :512], dat["q"]) and torch.equal(qkv[:, 512:1024], dat["k"]) and torch.equal(qkv[:, 1024:], dat["v"])
    q, k, v = (dat[n][rows].view(G, L, R.HEADS, R.D) for n in "qkv")
    dq, dk = _designed(dat)
    known = ~dq.isnan()
    assert torch.equal(q[known], dq[known]) and torch.equal(k[~dk.isnan()], dk[~dk.isnan()])
    for h in range(R.HEADS):
        blk = R.blocks_of(h)
        qn, kn = q[:, :, h, blk["noise"]], k[:, :, h, blk["noise"]]
        assert set(kn.abs().unique().tolist()) == {0.5, 1.5} and set(qn.unique().tolist()) <= {-2.0 * R.Q_NOISE, 0.0, 2.0 * R.Q_NOISE}
        flat, friendly = dat["fam"] == R.FAM_ID["flat"], dat["fam"] == R.FAM_ID["friendly"]
        assert not bool(qn[flat].any())
        assert 0.4 < float((qn[friendly] != 0).double().mean()) < 0.6
        assert 0.25 < float((qn[~flat & ~friendly] != 0).double().mean()) < 0.35
        lv = torch.cat([k[:, :, h, blk["wide_a"]], k[:, :, h, blk["wide_b"]]], -1)
        assert bool(((lv.abs() * 2) % 2 == 1).all()) and float(lv.abs().max()) == 7.5         # odd halves: never 0
        assert bool((lv[:, 0] == 7.5).all()) and (L == 1 or bool((lv[:, 1] == -7.5).all()))
        assert bool((lv[..., :8] == lv[..., :1]).all()) and bool((lv[..., 8:] == lv[..., 8:9]).all())
    assert not bool(q[dat["fam"] == R.FAM_ID["flat"]].any()), "a flat row's q is not all zero"
    # the grid: halves below 8 (at most 4 significant bits), v integers of one sign per column, zeros only where c = 0
    for t in (dat["q"][r], dat["k"][r], dat["v"][r]):
        assert torch.equal(t * 2, (t * 2).round()) and float(t.abs().max()) < 8 and torch.equal(t.to(BF).double(), t)
    vv = dat["v"][r]
    assert torch.equal(vv, vv.round()) and 1 <= float(vv.abs().min()) and float(vv.abs().max()) <= 7
    assert bool((vv.view(-1, R.HEADS, R.D)[..., :32] > 0).all()) and bool((vv.view(-1, R.HEADS, R.D)[..., 32:] < 0).any())
    zero = qkv[r] == 0
    assert not bool(zero[:, dat["c"] != 0].any()), "a column with c != 0 holds a zero"
    ck, cv = dat["c"][512:1024].view(R.HEADS, R.D), dat["c"][1024:]
    assert not bool(dat["c"][:512].any()) and bool((cv.abs() == 4).all())
    for h in range(R.HEADS):
        assert bool((ck[h, R.blocks_of(h)["const"]] == 5.5).all()) and float(ck[h].abs().sum()) == 8 * 5.5
    # pack_rowgemm512's fold is exact, and the kernel's fp32 expression rounds to the designed value with rstd up to 2 ulps off
    R.pack(ops, dat, "cpu")
    want = qkv[r].to(BF)
    for ulp in (-2, -1, 0, 1, 2):
        for fma in (False, True):
            bad = bad_elements(R.emulate(dat, ulp, fma), want)
            assert not bool(bad.any()), (c["name"], ulp, fma, xr.describe(bad, R.emulate(dat, ulp, fma), want))


# ------------------------------------------------------------------------------------------------------------ the families
@pytest.mark.parametrize("c", ALL_CASES, ids=ids)
def test_case_holds_its_families_and_the_bars_have_meaning(c):
    dat = R.case_data(c)
    fam8 = dat["fam8"]
    assert {int(f) for f in fam8.unique()} == set(R.FAM_ID.values())
    for name in R.FAMS:
        n = int((fam8 == R.FAM_ID[name]).sum())
        assert name == "flat" or n >= 150, (name, n)
    print(f"{c['name']}: S_abs {dat['s_abs']:.1f} exp2 units, eps {dat['eps']:.3f}, (row, head) pairs per family "
          f"{[int((fam8 == R.FAM_ID[n]).sum()) for n in R.FAMS]}")
    assert dat["eps"] <= C.EPS_MAX and 160 < dat["s_abs"] < 200
    # the fp64 values are what bar (d) says: O = v at L = 1, the mean of V on flat rows, v of the peak on peaked rows
    rows, L = dat["rows"], c["L"]
    G = rows.shape[0]
    o64, v = dat["o64"], R.per_head(dat["v"], rows)
    m = R.exact_mask(dat)
    want = torch.zeros_like(o64)
    peak_member = torch.tensor(R.peaks_of(L))[dat["peak"]][:, None, :].expand(G, R.HEADS, L).reshape(G * R.HEADS, L)
    want[:] = torch.gather(v, 1, peak_member[..., None].expand(-1, -1, R.D))
    if L & (L - 1) == 0:
        flat = fam8 == R.FAM_ID["flat"]
        want[flat] = v.mean(1, keepdim=True).expand(-1, L, -1)[flat]
        assert torch.equal(want[flat].to(BF).double(), want[flat]), "a flat row's mean of V is no bf16 number"
    assert bool(m.any()) and torch.equal(o64.to(BF)[m], want.to(BF)[m])
    q = R.per_head(dat["q"], rows) * R.SCALE_LOG2
    s = q @ R.per_head(dat["k"], rows).transpose(1, 2)
    if L > 1:
        top2 = s.topk(2, -1).values
        pk = fam8 == R.FAM_ID["peaked"]
        assert float((top2[..., 0] - top2[..., 1])[pk].min()) >= R.PEAK_DROP
    spans = {n: (float(s[fam8 == R.FAM_ID[n]].min()), float(s[fam8 == R.FAM_ID[n]].max())) for n in R.FAMS}
    print("    score range per family (exp2 units): " + ", ".join(f"{n} {a:+.0f}..{b:+.0f}" for n, (a, b) in spans.items()))
    if L > 1:
        assert spans["large"][0] < -140 and spans["large"][1] > 140 and spans["shift-low"][1] < -20 and spans["shift-high"][0] > 20


# ------------------------------------------------------------------------------------------------------------ the plans
def _meta(c):
    return xr.strided(torch.empty(c["M"], 512, dtype=BF, device="meta"), c["pad"]), xr.GuardedOut(c["M"], 512, "meta")


def test_the_gpu_matrix_reaches_every_kernel_and_schedule_on_meta_tensors(ops):
    seen = set()
    for c in R.GROUP_ATTN_CASES + R.NO_GROUP_CASES:
        x, out = _meta(c)
        assert x.stride(0) in (640, 768)
        plan = ops.router_group_attn_plan(x, *xr.geometry(c), out=out.view())
        assert {k: plan[k] for k in ("P", "G", "wide", "tiles")} == R.expected_plan(c), (c["name"], plan)
        multi = plan["tiles"] / 16 * 8 > plan["blocks"]
        assert multi == c["multi"], (c["name"], plan)
        seen |= {("wide" if plan["wide"] else f"P{plan['P']}"), ("multi", plan["wide"]) if multi else None, f"L{c['L']}"}
        if c["L"] < R.slots_of(c["L"]):
            seen.add(("empty slots", plan["wide"]))
        if not plan["wide"] and (c["n_outer"] * c["n_inner"]) % plan["G"]:
            seen.add("ragged last tile")
    assert seen >= {"P1", "P2", "P4", "P8", "P16", "wide", ("multi", False), ("multi", True), ("empty slots", False), ("empty slots", True),
                    "ragged last tile"} | {f"L{L}" for L in (1, 2, 3, 4, 8, 13, 16, 17, 25, 32)}
    assert all(1000 <= c["M"] <= 4500 for c in R.GROUP_ATTN_CASES if not c["multi"])
    chain = set()
    for c in R.ATTN_OUT_CASES + R.NO_GROUP_OUT_CASES:
        x, _ = _meta(c)
        plan = ops.router_group_attn_out_plan(x, *xr.geometry(c), tiles_pass0=c["tp0"])
        assert (plan["tiles"], plan["tp0"], plan["passes"]) == R.expected_chain_plan(c), (c["name"], plan)
        chain |= {f"L{c['L']}", f"tp{c['tp0']}", f"{plan['passes']} passes"}
    assert chain >= {"L1", "L2", "L3", "L13", "L16", "tp0", "tp1", "tp6", "1 passes", "2 passes"}


# ------------------------------------------------------------------------------------------------------------ restatement and faults
def _failed(dat, got, rest):
    """The bars ``got`` fails: a subset of {"a", "b", "d"} (cond_attn.check's own conditions, family by family)."""
    mine, ref = (C.figures(t, dat["o64"], dat["A"], dat["fam8"]) for t in (got, rest))
    out = set()
    for f in R.FAMS:
        if not mine[f][0] <= 1 + dat["eps"]:
            out.add("a")
        if f != "flat" and not abs(mine[f][1]) <= abs(ref[f][1]) + C.BIAS_MARGIN:
            out.add("b")
    m = R.exact_mask(dat)
    if bool(bad_elements(got[m], dat["o64"].to(BF)[m]).any()):
        out.add("d")
    return out, mine, ref


@pytest.mark.parametrize("c", ALL_CASES, ids=ids)
def test_restatement_passes_and_planted_faults_fail(c):
    """leak_next, leak_empty and drop_last fail bar (a) wherever the geometry has such a key; a truncated P fails (b) and a truncated
    O fails (a) or (b) from L = 3 up.  At L = 2 nothing is asserted of the two truncations (most of a friendly row's mass sits on the
    largest score, whose P = 1 is exact) and at L = 1 there is nothing to truncate: what is seen there is printed."""
    dat, L = R.case_data(c), c["L"]
    rest = R.restate(dat)
    R.check(c["name"], rest, dat, restated=rest)
    assert _failed(dat, rest, rest)[0] == set()
    for fault in R.FAULTS:
        if fault == "drop_last" and L == 1:
            continue
        got = R.restate(dat, fault)
        failed, mine, ref = _failed(dat, got, rest)
        print(f"{c['name']} {fault}: fails {sorted(failed) or 'nothing'}; friendly worst e {mine['friendly'][0]:.2f}, b {mine['friendly'][1]:+.2f} "
              f"(restatement {ref['friendly'][1]:+.2f})")
        has = {"leak_next": bool(R.has_next(dat).any()), "leak_empty": R.has_empty(dat), "drop_last": L >= 2}.get(fault)
        if has is False:
            assert torch.equal(got.view(torch.int16), rest.view(torch.int16)) or fault == "drop_last"
        elif has:
            assert "a" in failed, (c["name"], fault, failed)
        elif fault == "p_trunc" and L >= 3:
            assert "b" in failed, (c["name"], fault, failed)
        elif fault == "o_trunc" and L >= 3:
            assert failed & {"a", "b"}, (c["name"], fault, failed)
        if failed:
            with pytest.raises(AssertionError):
                R.check(c["name"], got, dat, restated=rest, out=lambda *_: None)


@pytest.mark.parametrize("c", R.ATTN_OUT_CASES, ids=ids)
def test_chain_restatement_passes_the_chain_bar_and_a_wrong_row_head_or_residual_fails_it(c):
    dat = R.chain_case_data(c)
    G, L = dat["rows"].shape
    a = R.restate(dat)
    fig = R.chain_check(c["name"], R.chain_restate(dat, a), dat)
    assert fig[0] <= 1 and 4 < fig[2] < 64                                # loose, and not empty: some tens of ulps of y
    heads = a.view(G, R.HEADS, L, R.D)
    wrong = {"two heads swapped": R.chain_restate(dat, heads[:, [1, 0, 2, 3, 4, 5, 6, 7]].reshape(a.shape)),
             "the attention of the next group": R.chain_restate(dat, heads.roll(1, 0).reshape(a.shape)),
             "columns rotated by one": R.chain_restate(dat, a.roll(1, -1)),
             "no residual": (R.chain_restate(dat, a).float() - dat["x"].float()[dat["rows"].reshape(-1)]).to(BF)}
    if L > 1:
        wrong["the attention of the next member"] = R.chain_restate(dat, a.roll(1, 1))
    for what, got in wrong.items():
        with pytest.raises(AssertionError):
            R.chain_check(f"{c['name']} ({what})", got, dat)
