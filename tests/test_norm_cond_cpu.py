"""CPU: the data conditions of tests/cond_norm.py -- what test_norm_cond_gpu.py assumes about its rows, its weights and its bars.
For every case: each row (group) has the R, spread or constancy its distribution claims, measured on the bf16 values; the fp32
centred restatement alone sits at about half a bf16 ulp from fp64 on every distribution, so the bar "restatement + 0.5 ulp" is
about one ulp -- it neither hides a kernel that is a whole step off nor fails a correct one; and a planted one-pass restatement
fails that bar on the out-of-domain rows, so the bar tells the two variance formulas apart."""
import math

import pytest
import torch

import cond_norm as cn
from cond_norm import BF, FAMILIES

def _rest_ok(name, restated, want64, fam, room, floor=cn.FLOOR, extra=0.0):
    """The restatement's worst error per distribution stays inside ``room`` (cond_norm.restatement_room): the bar "restatement +
    0.5 ulp" is then about one ulp wherever the operation is well conditioned in fp32."""
    fig = cn.figures(restated, want64, fam, floor)
    assert set(fig) == set(FAMILIES), (name, sorted(fig))
    for f, (worst, share, finite) in fig.items():
        print(f"{name} | {f:13s} | fp32 centred restatement: worst {worst:.4f} ulp (room {room[f] + extra:.2f}), {100 * share:.3f} % off the rounded fp64")
        assert finite and worst <= room[f] + extra, (name, f, worst, room[f] + extra)
    return fig


def test_every_distribution_is_listed_once_per_cycle():
    assert {s["family"] for s in cn.SPECS} == set(FAMILIES) and cn.NSPEC <= cn.LN_ROWS and cn.NSPEC <= 32
    offs = {(s["R"], s["sign"], s["d"]) for s in cn.SPECS if s["family"].startswith("offset")}
    assert offs == {(R, sg, d) for R in (8, 64) for sg in (1, -1) for d in (2.0 ** -6, 1.0, 2.0 ** 6)}
    assert {s["ratio"] for s in cn.SPECS if s["family"] == "eps"} == {1 / 16, 1.0, 16.0}


@pytest.mark.parametrize("c", cn.LN_CASES + cn.LN_QUANT_CASES, ids=lambda c: c["name"])
def test_layernorm_rows_and_restatement(c):
    dat = cn.ln_data(c)
    cn.assert_rows_are_what_they_claim(dat["x"], c["eps"])
    _rest_ok(c["name"], cn.ln_restate(c, dat), cn.ln_ref64(c, dat), dat["fam"][:, None], cn.restatement_room(dat["x"], c["eps"]))
    assert 0 < c["split"] < c["rows"] or "mod" not in c["form"]


@pytest.mark.parametrize("c", cn.QK_CASES, ids=lambda c: c["name"])
def test_qknorm_rows_and_restatement(c):
    dat = cn.qk_data(c)
    cn.assert_rows_are_what_they_claim(dat["q"].reshape(-1, 64), c["eps"])
    cn.assert_rows_are_what_they_claim(dat["k"].reshape(-1, 64), c["eps"], first=7)
    assert 0 < c["text_rows"] < c["S"]
    room = cn.restatement_room(dat["q"].reshape(-1, 64), c["eps"])
    room_k = cn.restatement_room(dat["k"].reshape(-1, 64), c["eps"], first=7)
    _rest_ok(c["name"], cn.qk_restate(c, dat), cn.qk_ref64(c, dat), dat["fam"], {f: max(room[f], room_k[f]) for f in room})


def test_fused_qkv_rows_have_an_offset_of_64():
    dat = cn.qkv_data()
    R = cn.measured_R(cn.qkv_projected(dat))
    print(f"projected q / k head rows: R from {float(R.min()):.1f} to {float(R.max()):.1f}, median {float(R.median()):.1f}")
    assert 40 < float(R.min()) and float(R.max()) < 110 and 55 < float(R.median()) < 75


@pytest.mark.parametrize("c", cn.SCORES_CASES, ids=lambda c: c["name"])
def test_router_scores_rows_and_restatement(c):
    dat = cn.scores_data(c)
    for i in range(c["n_id"]):
        cn.assert_rows_are_what_they_claim(dat["x"][i], cn.EPS_LN, first=5 * i)
    # the one-hot keys put the rows behind the features: the definition's raw scores are the rows themselves
    if c["N"] < 1000:
        import exact_step as xs
        assert torch.equal(xs.scores_raw(dat), dat["x"].double())
    rooms = [cn.restatement_room(dat["x"][i], cn.EPS_LN, first=5 * i) for i in range(c["n_id"])]      # identity i starts at spec 5 i
    _rest_ok(c["name"], cn.scores_restate(dat), cn.scores_ref64(dat), dat["fam"], {f: max(r[f] for r in rooms) for f in rooms[0]})


@pytest.mark.parametrize("wset", list(cn.W_MEAN))
@pytest.mark.parametrize("N", [64, 512, 1536])
def test_row_gemm_weight_sets_have_the_s_they_claim(N, wset):
    wd = cn.fold_weights(N, wset, cn.seed_of(f"{N}{wset}"))
    wg, s, _ = cn.fold_host(wd)
    print(f"N {N} {wset}: |s| from {float(s.abs().min()):.2f} to {float(s.abs().max()):.2f}; sum |Wg| about {float(wg.float().abs().sum(1).mean()):.1f}")
    if wset == "zero-mean":
        assert float(s.abs().max()) < 5 * cn.W_STD * math.sqrt(512) * 1.3            # |s| is a few spreads of a zero-mean sum
    else:
        assert float(s.min()) > 512 * 0.05 * 0.7 and float(s.max()) < 512 * 0.05 * 1.3      # s is about 25.6: mean * s cancels acc


@pytest.mark.parametrize("c", cn.ROWGEMM_CASES, ids=lambda c: c["name"])
def test_rowgemm_rows_and_restatement(c):
    dat = cn.rowgemm_data(c)
    cn.assert_rows_are_what_they_claim(dat["x"], c["eps"])
    wg, s, cvec = cn.fold_host(dat)
    want = cn.fold_ref64(dat["x"], wg, cvec, c["eps"], c["gelu"], dat["res"])
    _rest_ok(c["name"], cn.fold_restate32(dat["x"], wg, cvec, c["eps"], c["gelu"], dat["res"]).to(BF), want, dat["fam"],
             cn.restatement_room(dat["x"], c["eps"], gain=max(3.0, float(s.abs().max()))))
    const = [i for i in range(c["M"]) if cn.spec_of(i)["family"] == "constant"]
    xd = dat["x"][const].double()
    assert bool((xd.var(-1, unbiased=False) == 0).all()) and bool((xd != 0).all())
    # ... and on them the fp64 definition is the bias path alone
    pre = cn.fold_ref64(dat["x"][const], wg, cvec, c["eps"])
    assert torch.equal(pre, cvec.double().expand_as(pre))
    b = cn.constant_rows_bound(dat["x"][const], wg, c["eps"])
    print(f"{c['name']}: bound on |y - c| of the constant rows: {float(b.min()):.3g} .. {float(b.max()):.3g}")


def test_chain_rows_and_restatement():
    for c, data, cols in ((cn.ATTN, cn.attn_data, slice(1024, 1536)), (cn.ATTN_OUT, cn.attn_data, slice(1024, 1536))) + tuple(
            (m, cn.mlp_data, slice(0, 512)) for m in cn.MLP_CASES):
        dat = data(c)
        cn.assert_rows_are_what_they_claim(dat["x"][:cn.NSPEC], c["eps"])
        assert float(dat["x"].float().abs().max()) < 2.0 ** 13
        wg, s, cvec = cn.fold_host(dat)
        gelu = data is cn.mlp_data
        inner = cn.fold_ref64(dat["x"], wg[cols], cvec[cols], c["eps"], gelu)
        inner32 = cn.fold_restate32(dat["x"], wg[cols], cvec[cols], c["eps"], gelu)
        room = cn.restatement_room(dat["x"], c["eps"], gain=max(3.0, float(s[cols].abs().max())))
        if c is cn.ATTN:
            _rest_ok(c["name"], inner32.to(BF), inner, dat["fam"], room)
        else:
            # the value a chain keeps in registers is rounded to bf16 before the second product: where the fp32 restatement rounds it
            # to the other neighbour the output is a whole step off, so here the restatement's own worst error is up to 1.5 ulp
            _rest_ok(c["name"], cn.chain_restate(dat["x"], inner32), cn.chain_ref64(dat["x"], inner), dat["fam"], room,
                     floor=cn.FLOOR * cn.CHAIN_SCALE, extra=1.0)


@pytest.mark.parametrize("c", cn.GN_CASES, ids=lambda c: c["name"])
def test_groupnorm_groups_and_restatement(c):
    dat = cn.gn_data(c)
    C, G = c["C"], c["groups"]
    cg = C // G
    n = c["T"] * c["H"] * c["W"]
    per_group = dat["x"].view(n, G, cg).transpose(0, 1).reshape(G, n * cg)
    cn.assert_rows_are_what_they_claim(per_group, c["eps"])
    assert n * (C // 8) < 2 ** 31 - 256                                   # the launcher's 32-bit piece index
    blocks = (n + 511) // 512
    assert blocks >= 2 and (n < 10 ** 5 or blocks > 2 * 256)             # the large case: every thread of the final kernel adds two partials
    const = [g for g in range(G) if cn.spec_of(g)["family"] == "constant"]
    assert bool((per_group[const].double().var(-1, unbiased=False) == 0).all())
    _rest_ok(c["name"], cn.gn_restate(c, dat), cn.gn_ref64(c, dat), cn.gn_fam(c), cn.restatement_room(per_group, c["eps"]))


# ------------------------------------------------------------------------------------------------------------ the planted fault
def test_a_one_pass_restatement_fails_the_centred_kernels_bar():
    """The bar separates the two formulas: the restatement with var = max(E[x^2] - mean^2, 0) from plain sequential fp32 sums stays
    inside it on the friendly rows and is outside it on the far-offset and the near-constant rows, by more than a whole step."""
    c = cn.LN_CASES[0]
    dat = cn.ln_data(c)
    want = cn.ln_ref64(c, dat)
    fam = dat["fam"][:, None]
    rest = cn.figures(cn.ln_restate(c, dat), want, fam)
    planted = cn.figures(cn.ln_restate(c, dat, stats=cn.one_pass_stats(dat["x"])), want, fam)
    for f in FAMILIES:
        print(f"{f:13s}: one-pass worst {planted[f][0]:9.3f} ulp, centred worst {rest[f][0]:.3f} ulp")
    assert planted["friendly"][0] <= rest["friendly"][0] + cn.MARGIN
    for f in ("far-offset", "near-constant"):
        assert planted[f][0] > rest[f][0] + cn.MARGIN + 1, (f, planted[f][0])
    with pytest.raises(AssertionError, match="far-offset"):
        cn.check("planted", cn.ln_restate(c, dat, stats=cn.one_pass_stats(dat["x"])), want, cn.ln_restate(c, dat), fam)
    # q/k-norm's width: 64 values cancel less, the near-constant rows still show it
    q = cn.QK_CASES[0]
    qd = cn.qk_data(q)
    qp = cn.figures(cn.qk_restate(q, qd, stats_of=cn.one_pass_stats), cn.qk_ref64(q, qd), qd["fam"])
    qr = cn.figures(cn.qk_restate(q, qd), cn.qk_ref64(q, qd), qd["fam"])
    print(f"q/k-norm near-constant: one-pass worst {qp['near-constant'][0]:.3f} ulp, centred {qr['near-constant'][0]:.3f}")
    assert qp["near-constant"][0] > qr["near-constant"][0] + cn.MARGIN


def test_groupnorm_moments_wrapper_checks_its_scratch():
    """ops.vae_groupnorm_stats(moments=True) takes an fp64 scratch of ceil(rows / 512) * groups * 2 values and refuses an fp32 or a
    short one before anything is launched (the fp32-pair form keeps its fp32 scratch)."""
    from bind_your_avatar_implementation_amd import ops
    x = torch.empty(1100, 64, dtype=BF, device="meta")
    sums = torch.empty(2, 4, dtype=torch.float32, device="meta")
    need = 3 * 4 * 2
    for kw, dtype, n in ((dict(moments=True), torch.float32, need), (dict(moments=True), torch.float64, need - 1), (dict(), torch.float64, need)):
        with pytest.raises(AssertionError):
            ops.vae_groupnorm_stats(x, sums, 4, torch.empty(n, dtype=dtype, device="meta"), **kw)
