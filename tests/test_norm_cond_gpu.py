"""GPU: every normalising kernel on the offset, wide-range, near-constant and constant rows of tests/cond_norm.py, against the fp64
definition on the bf16 values the kernel reads.  Each case holds every distribution, asserts the plan or instance it runs on BEFORE
the launch, prints per distribution the worst error in bf16 ulps and the share of elements off the correctly rounded result next
to the same two figures of the fp32 centred restatement, and asserts the bars of cond_norm's docstring: restatement + 0.5 ulp on
every domain distribution for every kernel and on the out-of-domain ones for the centred kernels and the VAE's GroupNorm; finite
results, and the bias path within a derived bound on constant rows, for the one-pass row kernels out of their domain.

The measured figures are in include/bya.h, at each entry point, and in DESIGN.md section 1; the tests print them."""
import pytest
import torch

import cond_norm as cn
import exact_rowk as xr
import exact_step as xs
from cond_norm import BF, FAMILIES

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_plan(c):
    vec, nv = cn.xn.VEC_NV[c["D"]]
    rpw = 2 if c["kernel"] == "rows" else 1
    waves = (c["rows"] + rpw - 1) // rpw
    return {"kernel": c["kernel"], "vec": vec, "nv": nv, "modulated": "mod" in c["form"], "rows_per_wave": rpw, "waves": waves,
            "grid": (waves + 3) // 4}


@pytest.mark.parametrize("c", cn.LN_CASES, ids=lambda c: c["name"])
def test_layernorm(dev, c):
    ops = _ops()
    dat = cn.ln_data(c)
    x = dat["x"].to(dev)
    out = torch.full_like(x, NAN)
    kw = cn.ln_kwargs(c, dat, dev)
    plan = ops.layernorm_plan(x, out, **kw)
    assert plan == _ln_plan(c), plan
    ops.layernorm(x, out, eps=c["eps"], **kw)
    torch.cuda.synchronize()
    cn.check(c["name"], out, cn.ln_ref64(c, dat, dev), cn.ln_restate(c, dat), dat["fam"][:, None], plan=plan)


@pytest.mark.parametrize("c", cn.LN_QUANT_CASES, ids=lambda c: c["name"])
def test_layernorm_fp8_and_mx_equal_layernorm_then_quantise(dev, c):
    """The existing contract on hostile rows: the fused forms give the bytes and scales of ``layernorm`` followed by the stand-alone
    quantiser on the same rows (whose bf16 output the case above holds to the bar)."""
    ops = _ops()
    dat = cn.ln_data(c)
    x = dat["x"].to(dev)
    M, D = x.shape
    kw = cn.ln_kwargs(c, dat, dev)
    y = torch.full_like(x, NAN)
    q = torch.full((M, D), 0xA5, dtype=torch.uint8, device=dev)
    plan = ops.layernorm_plan(x, q, out_kind=c["out"], **kw)
    assert plan == _ln_plan(c), plan
    ops.layernorm(x, y, eps=c["eps"], **kw)
    if c["out"] == "fp8":
        scales = torch.full((M,), NAN, dtype=torch.float32, device=dev)
        ops.layernorm_fp8(x, q, scales, eps=c["eps"], **kw)
        q2, s2 = ops.quantize_rows_fp8(y)
    else:
        scales = torch.full((M, D // 32), 0xEE, dtype=torch.uint8, device=dev)
        ops.layernorm_mx(x, q, scales, fmt=c["out"], eps=c["eps"], **kw)
        q2, s2 = ops.quantize_mx(y, c["out"])
    torch.cuda.synchronize()
    cn.check(c["name"] + " (bf16 form)", y, cn.ln_ref64(c, dat, dev), cn.ln_restate(c, dat), dat["fam"][:, None], plan=plan)
    bad_q, bad_s = (q != q2.view(M, -1)).any(1).cpu(), (scales.view(M, -1) != s2.view(M, -1)).any(1).cpu()
    for i, f in enumerate(FAMILIES):
        m = dat["fam"] == i
        print(f"{c['name']} | {f:13s} | rows whose codes differ {int(bad_q[m].sum())} of {int(m.sum())}, whose scales differ {int(bad_s[m].sum())}")
    assert not bool(bad_q.any()) and not bool(bad_s.any()), (f"{c['name']} [plan {plan}]: rows {bad_q.nonzero().flatten().tolist()} differ in their codes, "
                                                             f"rows {bad_s.nonzero().flatten().tolist()} in their scales")


# ------------------------------------------------------------------------------------------------------------ q/k-norm + RoPE
@pytest.mark.parametrize("c", cn.QK_CASES, ids=lambda c: c["name"])
def test_qknorm_rope(dev, c):
    ops = _ops()
    dat = cn.qk_data(c)
    S, H, T = c["S"], c["heads"], c["text_rows"]
    W = H * 64
    buf = torch.zeros(1, S + 3, 3 * W, dtype=BF, device=dev)               # q | k | v packed, as the projection leaves them
    buf[:, :S, :W], buf[:, :S, W:2 * W] = dat["q"].to(dev), dat["k"].to(dev)
    q, k = buf[:, :S, :W], buf[:, :S, W:2 * W]
    cos, sin = dat["cos"].to(dev), dat["sin"].to(dev)
    plan = ops.qknorm_rope_plan(q, k, H, T, cos=cos)
    pairs = 2 * S * H
    assert plan == {"stats": False, "only": 0, "slots": 0, "pairs": pairs, "waves": (pairs + 7) // 8, "grid": ((pairs + 7) // 8 + 3) // 4}, plan
    ops.qknorm_rope(q, k, *(dat[n].to(dev) for n in ("qw", "qb", "kw", "kb")), cos, sin, heads=H, text_rows=T, eps=c["eps"], k_scale=c["k_scale"])
    torch.cuda.synchronize()
    got = torch.stack([q, k]).contiguous()
    cn.check(c["name"], got, cn.qk_ref64(c, dat).to(dev), cn.qk_restate(c, dat), dat["fam"], plan=plan)


def test_fused_qkv_projection_on_offset_rows(dev):
    """bya_gemm_qkv_norm_rope on projected q and k rows with an offset of R = 64 (a constant column of A against a constant column
    block of W): bit equality with the GEMM followed by qknorm_rope, whose statistics the cases above hold to the bar."""
    ops = _ops()
    c, dat = cn.QKV, cn.qkv_data()
    M, N, text = c["M"], c["N"], c["text_rows"]
    width, heads = N // 3, N // 3 // 64
    a, w, bias = (dat[n].to(dev) for n in ("a", "w", "bias"))
    qw, qb, kw, kb, cos, sin = (dat[n].to(dev) for n in ("qw", "qb", "kw", "kb", "cos", "sin"))
    two = torch.zeros(3, 1, M, width, dtype=BF, device=dev)
    one = torch.full_like(two, NAN)
    split = (width, M * width)
    ops.gemm(a, w, two[0, 0], bias=bias, split=split)
    torch.cuda.synchronize()
    R = cn.measured_R(two[:2].reshape(-1, 64).cpu())
    print(f"{c['name']}: R of the projected head rows {float(R.min()):.1f} .. {float(R.max()):.1f}, median {float(R.median()):.1f}")
    assert 40 < float(R.min()) and float(R.max()) < 110
    ops.qknorm_rope(two[0], two[1], qw, qb, kw, kb, cos, sin, heads=heads, text_rows=text, eps=cn.EPS_QK, k_scale=0.18)
    plan = ops.gemm_qkv_norm_rope_plan(a, w, one[0, 0], bias, split, qw, qb, kw, kb, cos, sin, text, eps=cn.EPS_QK, k_scale=0.18)
    assert ops.plan_key(plan) == c["expect"], plan
    assert ops.gemm_qkv_norm_rope(a, w, one[0, 0], bias, split, qw, qb, kw, kb, cos, sin, text, eps=cn.EPS_QK, k_scale=0.18)
    torch.cuda.synchronize()
    bad = cn.xn.bad_elements(one, two)
    assert not bool(bad.any()), f"{c['name']} [plan {plan}]: {cn.xn.describe(bad.reshape(-1, width), one.reshape(-1, width), two.reshape(-1, width))}"


# ------------------------------------------------------------------------------------------------------------ router scores
@pytest.mark.parametrize("c", cn.SCORES_CASES, ids=lambda c: c["name"])
def test_router_scores(dev, c):
    """The LayerNorm over the 512 features of both score kernels (router_head has no normalisation: x . w + b and a sigmoid)."""
    ops = _ops()
    dat = cn.scores_data(c)
    n_id, N = c["n_id"], c["N"]
    qr, kr, w, b, pos = (dat[k].to(dev) for k in ("qr", "kr", "ln_w", "ln_b", "pos"))
    out = torch.full((n_id, N, 512), NAN, dtype=BF, device=dev)
    plan = ops.router_scores_plan(qr, kr, w, b, pos, out, n_id, N)
    assert plan == xs.scores_plan(c), plan
    ops.router_scores(qr, kr, w, b, pos, out, n_id, N, eps=cn.EPS_LN)
    torch.cuda.synchronize()
    cn.check(c["name"], out, cn.scores_ref64(dat, dev), cn.scores_restate(dat), dat["fam"], plan=plan)


# ------------------------------------------------------------------------------------------------------------ folded-LayerNorm row kernels
def _pack(ops, dat, dev):
    pack = ops.pack_rowgemm512(dat["w"].to(dev), dat["b"].to(dev), dat["gamma"].to(dev), dat["beta"].to(dev))
    wg, s, cvec = cn.fold_host(dat)
    assert torch.equal(pack["w"].cpu(), wg)
    return pack, pack["w"].cpu(), pack["cvec"].cpu()


def _constant_rows_within_bound(name, got, cvec, x, wg, eps, M):
    """One-pass kernels on the constant rows: |y - c| within cond_norm.constant_rows_bound (plus the rounding of y to bf16), the
    rows of 3 and the rows of 50 apart: the bound has power at 3 only."""
    for a in sorted({cn.spec_of(i)["c"] for i in range(M) if cn.spec_of(i)["family"] == "constant"}):
        rows = [i for i in range(M) if cn.spec_of(i)["family"] == "constant" and cn.spec_of(i)["c"] == a]
        assert rows and bool((x[rows].double() == a).all())
        bound = cn.constant_rows_bound(x[rows], wg, eps) + cvec.double().abs()[None] * 2.0 ** -8
        off = (got[rows].cpu().double() - cvec.double()[None]).abs()
        print(f"{name} | constant rows of {a:g}: worst |y - c| {float(off.max()):.3e}, bound {float(bound.min()):.3g} .. {float(bound.max()):.3g} "
              f"(worst |y - c| / bound {float((off / bound).max()):.3e})")
        assert bool((off <= bound).all()), f"{name}: a constant row of {a:g} is {float((off / bound).max()):.3g} times its bound off the bias path"


@pytest.mark.parametrize("c", cn.ROWGEMM_CASES, ids=lambda c: c["name"])
def test_rowgemm512_folded_layernorm(dev, c):
    ops = _ops()
    dat = cn.rowgemm_data(c)
    M, N = c["M"], c["N"]
    x = dat["x"].to(dev)
    pack, wg, cvec = _pack(ops, dat, dev)
    out = torch.full((M, N), NAN, dtype=BF, device=dev)
    act = "gelu_erf" if c["gelu"] else None
    plan = ops.rowgemm512_plan(x, N, out=out, ln=True, res=out if c["res"] else None, act=act)
    assert (plan["form"], plan["ln"], plan["res"], plan["gelu"]) == ("chunk_balanced", True, c["res"], c["gelu"]), plan
    if c["res"]:
        out.copy_(dat["res"])
    ops.rowgemm512(x, pack, out, res=out if c["res"] else None, act=act, eps=c["eps"])
    torch.cuda.synchronize()
    want = cn.fold_ref64(dat["x"], wg, cvec, c["eps"], c["gelu"], dat["res"], dev)
    rest = cn.fold_restate32(dat["x"], wg, cvec, c["eps"], c["gelu"], dat["res"]).to(BF)
    cn.check(c["name"], out, want, rest, dat["fam"], barred=cn.rowk_domain(c), plan=plan)
    if not c["gelu"] and not c["res"]:
        _constant_rows_within_bound(c["name"], out, cvec, dat["x"], wg, c["eps"], M)


def test_router_group_attn_one_key(dev):
    """L = 1: the softmax is 1 and the output is bf16(v) = bf16(LN(x) . Wv^T + cv): the statistics without the attention."""
    ops = _ops()
    c = cn.ATTN
    dat = cn.attn_data(c)
    M, geo = c["M"], xr.geometry(c)
    x = dat["x"].to(dev)
    pack, wg, cvec = _pack(ops, dat, dev)
    out = torch.full((M, 512), NAN, dtype=BF, device=dev)
    plan = ops.router_group_attn_plan(x, *geo, out=out)
    assert (plan["P"], plan["wide"], plan["tiles"]) == (1, False, (M + 15) // 16), plan
    ops.router_group_attn(x, pack, out, *geo, eps=c["eps"])
    torch.cuda.synchronize()
    want = cn.fold_ref64(dat["x"], wg[1024:], cvec[1024:], c["eps"], dev=dev)
    rest = cn.fold_restate32(dat["x"], wg[1024:], cvec[1024:], c["eps"]).to(BF)
    cn.check(c["name"], out, want, rest, dat["fam"], barred=cn.rowk_domain(c), plan=plan)
    _constant_rows_within_bound(c["name"], out, cvec[1024:], dat["x"], wg[1024:], c["eps"], M)


def test_router_group_attn_out_one_key(dev):
    """The chain behind it with to_out = 2^40 I: out = bf16(x + 2^40 bf16(v))."""
    ops = _ops()
    c = cn.ATTN_OUT
    dat = cn.attn_data(c)
    M, geo = c["M"], xr.geometry(c)
    x = dat["x"].to(dev)
    pack, wg, cvec = _pack(ops, dat, dev)
    w2, b2 = cn.chain_weight()
    pack_o = ops.pack_rowgemm512(w2.to(dev), b2.to(dev))
    out = torch.full((M, 512), NAN, dtype=BF, device=dev)
    plan = ops.router_group_attn_out_plan(x, *geo, out=out, tiles_pass0=c["tp0"])
    assert (plan["tiles"], plan["passes"]) == ((M + 15) // 16, 1), plan
    ops.router_group_attn_out(x, pack, pack_o, *geo, eps=c["eps"], out=out, tiles_pass0=c["tp0"])
    torch.cuda.synchronize()
    inner = cn.fold_ref64(dat["x"], wg[1024:], cvec[1024:], c["eps"], dev=dev)
    inner32 = cn.fold_restate32(dat["x"], wg[1024:], cvec[1024:], c["eps"])
    cn.check(c["name"], out, cn.chain_ref64(dat["x"], inner, dev), cn.chain_restate(dat["x"], inner32), dat["fam"], barred=cn.rowk_domain(c),
             floor=cn.FLOOR * cn.CHAIN_SCALE, plan=plan)


@pytest.mark.parametrize("c", cn.MLP_CASES, ids=lambda c: c["name"])
def test_router_mlp_fused(dev, c):
    """mlp[2] = 2^40 I: out = bf16(x + 2^40 bf16(GELU(LN(x) . W1g^T + c1))); M = 4388 at one tile per workgroup in pass 0 leaves 19
    tiles to the remainder pass."""
    ops = _ops()
    dat = cn.mlp_data(c)
    M = c["M"]
    x = dat["x"].to(dev)
    pack1, wg, cvec = _pack(ops, dat, dev)
    w2, b2 = cn.chain_weight()
    pack2 = ops.pack_rowgemm512(w2.to(dev), b2.to(dev))
    out = torch.full((M, 512), NAN, dtype=BF, device=dev)
    plan = ops.router_mlp_fused_plan(x, out=out, tiles_pass0=c["tp0"])
    assert (plan["tiles"], plan["passes"]) == ((M + 15) // 16, c["passes"]), plan
    ops.router_mlp_fused(x, pack1, pack2, eps=c["eps"], out=out, tiles_pass0=c["tp0"])
    torch.cuda.synchronize()
    inner = cn.fold_ref64(dat["x"], wg, cvec, c["eps"], True, dev=dev)
    inner32 = cn.fold_restate32(dat["x"], wg, cvec, c["eps"], True)
    cn.check(c["name"], out, cn.chain_ref64(dat["x"], inner, dev), cn.chain_restate(dat["x"], inner32), dat["fam"], barred=cn.rowk_domain(c),
             floor=cn.FLOOR * cn.CHAIN_SCALE, plan=plan)


# ------------------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "pair"])
@pytest.mark.parametrize("c", cn.GN_CASES, ids=lambda c: c["name"])
def test_vae_groupnorm(dev, c, moments):
    """The VAE's GroupNorm: every group of the tensor holds another distribution (a group mix-up shows as a domain group off by whole
    steps).  ``moments``: bya_vae_groupnorm_moments + bya_vae_norm_act_moments, what vae.py runs -- (mean, var) formed in fp64 from
    fp64 sums -- held to the bar on every distribution, like a centred kernel.  Otherwise bya_vae_groupnorm_stats + bya_vae_norm_act on
    the fp32 pair (sum x, sum x^2): held to the bar on its domain (cond_norm.GN_PAIR_DOMAIN: R <= 8), finite beyond it, figures
    printed."""
    ops = _ops()
    dat = cn.gn_data(c)
    C, G = c["C"], c["groups"]
    x = dat["x"].to(dev)
    sums = torch.full((2 * G,), NAN, dtype=torch.float32, device=dev)
    ops.vae_groupnorm_stats(x.view(-1, C), sums, G, moments=moments)
    y = torch.full_like(x, NAN)
    kw = {}
    if dat["zyb"] is not None:
        zyb = dat["zyb"].to(dev)
        kw = dict(zy=zyb[:, :C], zb=zyb[:, C:], latent_shape=c["lat"], tmode=c["tmode"])
    gamma, beta = dat["gamma"].to(dev), dat["beta"].to(dev)
    ops.vae_norm_act(x, y, sums, gamma, beta, G, act=c["act"], eps=c["eps"], moments=moments, **kw)
    torch.cuda.synchronize()
    got = y.view(-1, C)
    name = c["name"] + ("-moments" if moments else "-pair")
    cn.check(name, got, cn.gn_ref64(c, dat, dev), cn.gn_restate(c, dat, dev), cn.gn_fam(c), barred=FAMILIES if moments else cn.GN_PAIR_DOMAIN)
    if c["form"] == "plain" and c["act"] == "none":
        cg = C // G
        for g in range(G):
            sp = cn.spec_of(g)
            if sp["family"] != "constant":
                continue
            ch = slice(g * cg, (g + 1) * cg)
            bt = dat["beta"].double()[ch]
            bound = cn.gn_constant_bound(c, dat, sp["c"])[ch] + bt.abs() * 2.0 ** -8
            off = (got[:, ch].cpu().double() - bt[None]).abs().amax(0)
            print(f"{name} | constant group {g} ({sp['name']}): worst |y - beta| {float(off.max()):.3e} (worst / bound {float((off / bound).max()):.3e})")
            assert bool((off <= bound).all()), f"{name}: constant group {g} is {float((off / bound).max()):.3g} times its bound off beta"


@pytest.mark.parametrize("C,rows", cn.xv.STATS_CASES + [cn.xv.STATS_LARGE], ids=lambda v: str(v))
def test_groupnorm_moments_exact(dev, C, rows):
    """bya_vae_groupnorm_moments on exact_vae's statistics data (x = mu_g + d_g e with as many e = +1 as -1 per group, up to one: every
    sum an integer, exact in fp64): mean and var must EQUAL the fp64 values of (sum x / n, sum x^2 / n - mean^2) rounded once to fp32
    -- mu_g and d_g^2 where the group's count is even -- bit for bit; a lost row, a lost block or a wrong count changes them.  Two
    launches agree in every bit, and nothing is written past the outputs."""
    ops = _ops()
    dat = cn.xv.stats_data(C, rows)
    G = cn.xv.GROUPS
    x = dat["x"].to(dev)
    blocks = dat["partial"].shape[0]
    n = float(dat["count"])
    s1, s2 = dat["sums"].double()[0::2], dat["sums"].double()[1::2]
    mean = s1 / n
    want = torch.stack([mean, s2 / n - mean * mean], 1).reshape(-1).float()
    if dat["count"] % 2 == 0:
        assert torch.equal(want.double()[0::2], torch.from_numpy(dat["mu"]).double())
        assert torch.equal(want.double()[1::2], torch.from_numpy(dat["d"] ** 2).double())
    runs = []
    for _ in range(2):
        mom = torch.full((2 * G + 8,), NAN, dtype=torch.float32, device=dev)
        part = torch.full((blocks * G * 2 + 8,), NAN, dtype=torch.float64, device=dev)
        ops.vae_groupnorm_stats(x, mom[:2 * G], G, part[:blocks * G * 2], moments=True)
        torch.cuda.synchronize()
        assert bool(mom[2 * G:].isnan().all()) and bool(part[blocks * G * 2:].isnan().all()), "a write past the outputs"
        runs.append((mom[:2 * G].cpu(), part[:blocks * G * 2].cpu()))
    got, gpart = runs[0]
    # an odd count leaves mean = (n mu +- d) / n and a variance that cancels in fp64: the kernel may contract q / n - mean * mean into an
    # fma, which moves the fp64 value by 1e-16 and its fp32 rounding by at most one step; an even count leaves no rounding at all
    slack = 0 if dat["count"] % 2 == 0 else 1
    bad = ((got.view(torch.int32) - want.view(torch.int32)).abs() > slack).nonzero()
    assert bad.numel() == 0, (f"C={C} rows={rows}: {bad.shape[0]} of 64 moments differ; first: group {int(bad[0]) // 2} "
                              f"{'var' if int(bad[0]) % 2 else 'mean'}: got {float(got[int(bad[0])])!r}, want {float(want[int(bad[0])])!r}")
    assert torch.equal(gpart, dat["partial"].double().reshape(-1)), f"C={C} rows={rows}: an fp64 partial is not the exact sum of its 512 rows"
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
