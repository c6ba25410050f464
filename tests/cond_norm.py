"""Conditioning of the normalising kernels (a plain helper module: no tests, no fixtures; the sibling of the ``exact_*`` modules).
The exact-data suites choose rows whose sum x and sum x^2 are exact, so mean = mu and var = d^2 whatever formula a kernel uses, and
the random-data tests draw N(0, 1), the one distribution on which a one-pass variance E[x^2] - mean^2 is as good as a centred one.
Here the rows are the ones on which the two formulas part, and the measure is the error of every element in bf16 ulps against the
fp64 definition evaluated on the bf16 values the kernel reads.

ROW DISTRIBUTIONS (``SPECS``; width K, seeded, rounded to bf16 before anything is computed from them).  R = |mean| / spread.
  in the domain      friendly   N(0, 1), the control
                     offset     mu + d e, R = |mu| / d in {8, 64}, both signs of mu, d in {2^-6, 1, 2^6}
                     outlier    N(0, 1) with max(K / 256, 1) channels multiplied by 300 (``hard_inputs`` of test_mx_gpu.py)
                     eps        N(0, 1) scaled so that var / eps is 1/16, 1, 16 at the kernel's own eps
  out of the domain  far-offset     R = 256, both signs: a bf16 row keeps less than two bits of its spread
                     near-constant  the constant 3.0 or 50.0 with 8 channels moved by one to three bf16 steps
                     constant       every channel 3.0 or 50.0: var is exactly 0, the answer is the bias path alone
Every case holds every spec at least once: a case's rows (for GroupNorm: its groups) cycle through ``SPECS``.

MEASURE (``ulp_error``): |got - fp64| / ulp, ulp = that of bf16(fp64), results below ``floor`` (2^-6 for outputs of order 1: where
an affine term cancels the normalised value) counted in ulps of the floor -- ``exact_gemm.bf16_ulps``'s unit, taken against the
unrounded fp64 value, so that a correctly rounded result scores at most 0.5.  ``figures`` gives per distribution the worst error and
the share of elements whose bits differ from bf16(fp64).

BARS (``check``).  The RESTATEMENT is the operation the model's reference runs -- F.layer_norm / F.group_norm in fp32 on the same
bf16 inputs, centred, rounded once to bf16 -- computed at test time; its worst error is about half an ulp, pure rounding.
  * a domain distribution, every kernel:        worst <= the restatement's worst + 0.5 ulp
  * an out-of-domain one, a centred kernel:     the same
  * an out-of-domain one, a one-pass kernel:    finite; the constant rows within a bound derived from the kernel's arithmetic
The row kernels' domain is narrower than the list above (``ROWK_DOMAIN``: R <= 8).  The VAE's GroupNorm
forms its one-pass variance in fp64 and is held to the bar on every distribution, like a centred kernel.
No bar is taken from a kernel's output.  The half ulp lets a correct kernel land on the other side of a rounding boundary
(rsqrtf's last bit, contraction order); it does not let it be a whole step off.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import exact_norm as xn
import exact_rowk as xr
import exact_step as xs
import exact_vae as xv
from exact_gemm import BF

DOMAIN = ("friendly", "offset R8", "offset R64", "outlier", "eps")
OUT_OF_DOMAIN = ("far-offset", "near-constant", "constant")
FAMILIES = DOMAIN + OUT_OF_DOMAIN
# What the one-pass row kernels (var = E[x^2] - mean^2 from matrix-core sums, then rstd (x . Wg^T - mean s) + c) are held to: R <= 8.
# R = 64 is whole steps off on every case (include/bya.h has the figures).  One case misses R = 8 as well and carries ``carve``:
# rowgemm512 at N = 1536 with GELU + residual and s = rowsum(Wg) = 25.6, where the second cancellation and the residual's leave
# 1.14 ulp against a bar of 1.06; there the offset rows are printed and must be finite.
ROWK_DOMAIN = ("friendly", "offset R8", "outlier", "eps")


# bya_vae_groupnorm_stats + bya_vae_norm_act carry the fp32 pair (sum x, sum x^2), which holds a group's variance to 3 u R^2: R <= 8
GN_PAIR_DOMAIN = ROWK_DOMAIN


def rowk_domain(c):
    return tuple(f for f in ROWK_DOMAIN if f not in c.get("carve", ()))
MARGIN = 0.5
FLOOR = 2.0 ** -6
EPS_LN, EPS_QK, EPS_VAE = 1e-5, 1e-6, 1e-6
U32 = 2.0 ** -24                                                     # unit roundoff of fp32


def _specs():
    s = [dict(family="friendly", name="friendly")]
    for R in (8, 64):
        for sign in (1, -1):
            for ld in (-6, 0, 6):
                s.append(dict(family=f"offset R{R}", name=f"offset R{R} {'+' if sign > 0 else '-'} d2^{ld}", R=R, sign=sign, d=2.0 ** ld))
    s.append(dict(family="outlier", name="outlier"))
    s += [dict(family="eps", name=f"var/eps {r:g}", ratio=r) for r in (1.0 / 16, 1.0, 16.0)]
    s += [dict(family="far-offset", name=f"far-offset {'+' if sign > 0 else '-'}", R=256, sign=sign, d=1.0) for sign in (1, -1)]
    s += [dict(family="near-constant", name=f"near-constant {c:g}", c=c) for c in (3.0, 50.0)]
    s += [dict(family="constant", name=f"constant {c:g}", c=c) for c in (3.0, 50.0)]
    return s


SPECS = _specs()
NSPEC = len(SPECS)                                                   # 23


def spec_of(i):
    return SPECS[i % NSPEC]


def family_index(n):
    """Family (index into ``FAMILIES``) of rows 0 .. n - 1 -> int64 [n]."""
    return torch.tensor([FAMILIES.index(spec_of(i)["family"]) for i in range(n)])


def bf16_step(c):
    return 2.0 ** (math.floor(math.log2(abs(c))) - 7)


def draw_row(spec, K, gen, eps):
    """One row of ``spec`` -> fp32 [K] (not yet rounded to bf16)."""
    fam = spec["family"]
    if fam in ("constant", "near-constant"):
        x = torch.full((K,), spec["c"])
        if fam == "near-constant":
            pos = torch.randperm(K, generator=gen)[:8]
            steps = torch.randint(1, 4, (8,), generator=gen) * (torch.randint(0, 2, (8,), generator=gen) * 2 - 1)
            x[pos] += steps * bf16_step(spec["c"])
        return x
    e = torch.randn(K, generator=gen)
    if fam == "friendly":
        return e
    if fam.startswith("offset") or fam == "far-offset":
        return spec["sign"] * spec["R"] * spec["d"] + spec["d"] * e
    if fam == "outlier":
        pos = torch.randperm(K, generator=gen)[:max(K // 256, 1)]
        e[pos] = 300.0 * torch.where(e[pos] < 0, -1.0, 1.0) * e[pos].abs().clamp_min(0.5)      # (a channel near 0 would stay small)
        return e
    assert fam == "eps"
    return e * math.sqrt(spec["ratio"] * eps)


def rows(n, K, seed, eps, first=0):
    """x bf16 [n, K]: row i holds spec ``first + i`` (mod the list)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([draw_row(spec_of(first + i), K, gen, eps) for i in range(n)]).to(BF)


def measured_R(x):
    """|mean| / spread of every row of the bf16 values, in fp64 (inf where the spread is 0)."""
    xd = x.double()
    return xd.mean(-1).abs() / xd.std(-1, unbiased=False)


def assert_rows_are_what_they_claim(x, eps, first=0):
    """Every row of ``x`` [n, K] (bf16) has the R, the spread or the constancy of its spec, measured on the bf16 values."""
    xd = x.double()
    R, var = measured_R(x), xd.var(-1, unbiased=False)
    K = x.shape[-1]
    tol = 4.0 / math.sqrt(K) + 0.02                                   # sampling error of mean / spread, and bf16's quantisation
    for i in range(x.shape[0]):
        sp = spec_of(first + i)
        fam = sp["family"]
        if fam == "friendly":
            assert float(R[i]) < tol * 2 and abs(float(var[i]) - 1) < tol * 2, (sp["name"], float(R[i]), float(var[i]))
        elif fam.startswith("offset") or fam == "far-offset":
            # the rounding of mu + d e to bf16 adds a uniform error of step^2 / 12 to the variance: step = mu's bf16 step
            step = bf16_step(sp["R"] * sp["d"])
            spread = math.sqrt(sp["d"] ** 2 + step ** 2 / 12)
            want = sp["R"] * sp["d"] / spread
            assert abs(float(R[i]) / want - 1) < 3 * tol, (sp["name"], float(R[i]), want)
            assert (float(xd[i].mean()) > 0) == (sp["sign"] > 0)
            if fam == "far-offset":
                assert float(R[i]) > 128, (sp["name"], float(R[i]))    # less than two bits of spread survive the rounding
            else:
                assert float(R[i]) <= 64 * (1 + 3 * tol)
        elif fam == "outlier":
            big = xd[i].abs() > 30
            assert 1 <= int(big.sum()) <= max(K // 256, 1) and float(xd[i].abs().max()) > 30
        elif fam == "eps":
            assert abs(float(var[i]) / (sp["ratio"] * eps) - 1) < 3 * tol, (sp["name"], float(var[i]) / eps)
        elif fam == "near-constant":
            moved = xd[i] != sp["c"]
            assert int(moved.sum()) == 8 and float((xd[i] - sp["c"]).abs().max()) <= 3 * bf16_step(sp["c"])
            assert float(R[i]) > 128
        else:
            assert bool((xd[i] == sp["c"]).all()) and float(var[i]) == 0.0 and sp["c"] != 0


def restatement_room(x, eps, gain=3.0, first=0):
    """What the fp32 centred restatement may itself be off by on the rows ``x`` [n, K], per family: half an ulp of rounding, 0.05 for
    its fp32 products and sums, and the error of its mean -- up to about 3 u |mean|, i.e. 3 u |mean| rstd in the normalised value --
    times ``gain`` (the largest factor between the normalised value and the output: |w (1 + scale)| <= 3 for the affine forms, |s| =
    |rowsum(Wg)| for a folded Linear) where the output cancels down to the floor, whose bf16 step is 2^-13.  In the domain (R <= 66
    after the rounding to bf16) that is 0.84 ulp at gain 3; with s = 25.6 it is 3 ulp: there the operation itself is uncertain by
    whole steps in fp32, and the bar follows the restatement."""
    xd = x.double()
    r = xd.mean(-1).abs() / torch.sqrt(xd.var(-1, unbiased=False) + eps)
    fam = torch.tensor([FAMILIES.index(spec_of(first + i)["family"]) for i in range(x.shape[0])])
    return {f: 0.55 + 3 * U32 * gain * float(r[fam == i].max()) / 2.0 ** -13 for i, f in enumerate(FAMILIES) if bool((fam == i).any())}


# ------------------------------------------------------------------------------------------------------------ measure and bars
def ulp_error(got, want64, floor=FLOOR):
    """-> (error of every element in bf16 ulps of the fp64 result, mask of the elements whose bits differ from bf16(fp64))."""
    want = want64.to(BF)
    ulp = torch.exp2(torch.floor(torch.log2(want.double().abs().clamp_min(floor))) - 7)
    err = (got.double() - want64).abs() / ulp
    return err, xn.bad_elements(got, want)


def figures(got, want64, fam, floor=FLOOR):
    """Per family present: (worst error in ulps, share of elements that differ from the correctly rounded result, all finite).
    ``fam``: int64 family index, broadcastable to ``got``."""
    err, differ = ulp_error(got, want64, floor)
    fam = fam.to(got.device).expand(got.shape)
    out = {}
    for i, name in enumerate(FAMILIES):
        m = fam == i
        if bool(m.any()):
            e = err[m]
            finite = bool(torch.isfinite(got[m].float()).all())
            out[name] = (float(torch.nan_to_num(e, nan=float("inf")).max()), float(differ[m].double().mean()), finite)
    return out


def check(name, got, want64, restated, fam, barred=FAMILIES, floor=FLOOR, plan=None):
    """Print the figures of ``got`` and of the restatement per distribution and assert the bars of the module docstring: restatement +
    0.5 ulp on the families ``barred`` (a centred kernel: all of them; a one-pass kernel: its domain), finite results on the others.
    -> {family: (worst, share, restatement's worst, restatement's share)}."""
    mine, rest = figures(got, want64, fam, floor), figures(restated.to(got.device), want64, fam, floor)
    assert set(mine) == set(FAMILIES), f"{name}: a distribution is missing from the case: {sorted(mine)}"
    failed = []
    for f in FAMILIES:
        (w, s, finite), (rw, rs, _) = mine[f], rest[f]
        bar = f in barred
        print(f"{name} | {f:13s} | worst {w:9.3f} ulp, {100 * s:7.3f} % off the rounded fp64 | fp32 centred restatement: worst {rw:6.3f} ulp, "
              f"{100 * rs:7.3f} % | {'bar ' + format(rw + MARGIN, '.3f') if bar else 'one-pass, out of domain: finite'}")
        if not finite:
            failed.append(f"{f}: a result is not finite")
        elif bar and not w <= rw + MARGIN:
            failed.append(f"{f}: worst {w:.3f} ulp > the restatement's {rw:.3f} + {MARGIN}")
    assert not failed, f"{name} [plan {plan}]: " + "; ".join(failed)
    return {f: (mine[f][0], mine[f][1], rest[f][0], rest[f][1]) for f in FAMILIES}


def one_pass_stats(x):
    """The planted fault: mean and var = max(E[x^2] - mean^2, 0) from plain sequential fp32 sums -> (mean, var) fp32 [n, 1]."""
    xf = x.float().numpy()
    K = xf.shape[-1]
    s = np.cumsum(xf, axis=-1, dtype=np.float32)[:, -1:]
    q = np.cumsum(xf * xf, axis=-1, dtype=np.float32)[:, -1:]
    mean = s / np.float32(K)
    var = np.maximum(q / np.float32(K) - mean * mean, np.float32(0))
    return torch.from_numpy(mean), torch.from_numpy(var)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
LN_ROWS = 37


def _ln(D, kernel, form, split=0, out="bf16"):
    return dict(name=f"ln-{kernel}-D{D}-{form}" + ("" if out == "bf16" else f"-{out}"), D=D, kernel=kernel, form=form, rows=LN_ROWS, batch=1,
                split=split, out=out, eps=EPS_LN)


# D = 768 (vec 4, nv 3) is exact_norm.GENERIC_CASES' width that is no power of two; the rows kernel with the split inside a wave
LN_CASES = [_ln(512, "generic", "wb"), _ln(768, "generic", "wbmod", split=18), _ln(3072, "rows", "wb"), _ln(3072, "rows", "wbmod", split=18)]
LN_QUANT_CASES = [_ln(3072, "generic", "wbmod", split=18, out="fp8"), _ln(3072, "generic", "wbmod", split=18, out="mxfp8")]
assert any(c["D"] == 768 for c in xn.GENERIC_CASES)


def seed_of(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def _param(gen, n, mean, std):
    return (mean + std * torch.randn(n, generator=gen)).to(BF)


def ln_data(c):
    """-> dict: x [rows, D] bf16, w, b [D], sh, sc [2, D] or None (set 0 for rows < split), fam [rows]."""
    gen = torch.Generator().manual_seed(seed_of(c["name"]) + 1)
    D = c["D"]
    dat = dict(x=rows(c["rows"], D, seed_of(c["name"]), c["eps"]), w=_param(gen, D, 1.0, 0.2), b=_param(gen, D, 0.0, 0.5), sh=None, sc=None,
               fam=family_index(c["rows"]))
    if "mod" in c["form"]:
        dat["sh"], dat["sc"] = _param(gen, 2 * D, 0.0, 0.5).view(2, D), _param(gen, 2 * D, 0.0, 0.2).view(2, D)
    return dat


def ln_sets(c):
    return (torch.arange(c["rows"]) >= c["split"]).long()


def ln_ref64(c, dat, dev="cpu"):
    mv = lambda t: None if t is None else t.to(dev)
    return xn.ln_reference64(dat["x"].to(dev), c["eps"], mv(dat["w"]), mv(dat["b"]), mv(dat["sh"]), mv(dat["sc"]), ln_sets(c).to(dev))


def ln_restate(c, dat, stats=None):
    """F.layer_norm in fp32 (+ the modulation in fp32), rounded once.  ``stats``: (mean, var) of a planted fault instead."""
    x = dat["x"].float()
    if stats is None:
        y = F.layer_norm(x, (c["D"],), dat["w"].float(), dat["b"].float(), c["eps"])
    else:
        mean, var = stats
        y = (x - mean) * torch.rsqrt(var + np.float32(c["eps"])) * dat["w"].float() + dat["b"].float()
    if dat["sh"] is not None:
        s = ln_sets(c)
        y = y * (1 + dat["sc"].float()[s]) + dat["sh"].float()[s]
    return y.to(BF)


def ln_kwargs(c, dat, dev):
    kw = dict(weight=dat["w"].to(dev), bias=dat["b"].to(dev), split=c["split"])
    if dat["sh"] is not None:
        sh, sc = dat["sh"].to(dev), dat["sc"].to(dev)
        kw.update(shift0=sh[0], scale0=sc[0], shift1=sh[1], scale1=sc[1])
    return kw


# ------------------------------------------------------------------------------------------------------------ q/k-norm + RoPE
def _qk(rot):
    return dict(name=f"qk-{rot}", rot=rot, heads=3, batch=1, S=37, text_rows=5, k_scale=0.25, eps=EPS_QK)


QK_CASES = [_qk("identity"), _qk("real")]


def qk_data(c):
    """-> q, k [1, S, heads * 64] bf16 (head row i of q holds spec i, of k spec i + 7), qw, qb, kw, kb [64], cos, sin fp32
    [S - text_rows, 64], fam [2, 1, S, heads * 64]."""
    gen = torch.Generator().manual_seed(seed_of(c["name"]) + 1)
    S, H, T = c["S"], c["heads"], c["text_rows"]
    n = S * H
    q = rows(n, 64, seed_of(c["name"]), c["eps"]).view(1, S, H * 64)
    k = rows(n, 64, seed_of(c["name"]) + 5, c["eps"], first=7).view(1, S, H * 64)
    fam = torch.stack([torch.tensor([FAMILIES.index(spec_of(f + i)["family"]) for i in range(n)]) for f in (0, 7)])
    fam = fam.view(2, 1, S, H, 1).expand(2, 1, S, H, 64).reshape(2, 1, S, H * 64)
    if c["rot"] == "identity":
        cos, sin = torch.ones(S - T, 64), torch.zeros(S - T, 64)
    else:
        ang = torch.rand(S - T, 32, generator=gen).repeat_interleave(2, 1) * 6.3
        cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    p = [_param(gen, 64, 1.0, 0.2), _param(gen, 64, 0.0, 0.5), _param(gen, 64, 1.0, 0.2), _param(gen, 64, 0.0, 0.5)]
    return dict(q=q, k=k, qw=p[0], qb=p[1], kw=p[2], kb=p[3], cos=cos, sin=sin, fam=fam)


def qk_ref64(c, dat):
    """-> fp64 [2, 1, S, heads * 64] (q, k): exact_norm's definition."""
    args = (dat["cos"], dat["sin"], c["text_rows"], c["eps"])
    return torch.stack([xn.qk_reference64(dat["q"], dat["qw"], dat["qb"], *args, 1.0),
                        xn.qk_reference64(dat["k"], dat["kw"], dat["kb"], *args, c["k_scale"])])


def qk_restate(c, dat, stats_of=None):
    """F.layer_norm(64) in fp32, the rotation and k_scale in fp32, rounded once -> bf16 [2, 1, S, heads * 64]."""
    T, S = c["text_rows"], c["S"]
    out = []
    for x, w, b, ks in ((dat["q"], dat["qw"], dat["qb"], 1.0), (dat["k"], dat["kw"], dat["kb"], c["k_scale"])):
        xh = x.float().view(1, S, -1, 64)
        if stats_of is None:
            y = F.layer_norm(xh, (64,), w.float(), b.float(), c["eps"])
        else:
            mean, var = stats_of(xh.reshape(-1, 64).to(BF))
            y = ((xh.reshape(-1, 64) - mean) * torch.rsqrt(var + np.float32(c["eps"])) * w.float() + b.float()).view(xh.shape)
        v = y[:, T:]
        rot = torch.stack([-v[..., 1::2], v[..., 0::2]], -1).flatten(-2)
        y = torch.cat([y[:, :T], v * dat["cos"][None, :, None] + rot * dat["sin"][None, :, None]], 1)
        out.append((y * np.float32(ks)).reshape(1, S, -1).to(BF))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------------------ fused q|k|v projection
QKV = dict(name="qkv-R64", B=1, M=300, N=1152, K=256, text_rows=40, expect="p128", offset=64.0)


def qkv_data():
    """A [M, K], W [N, K], bias [N]: column 0 of A is the constant 8 and column 0 of the q and k rows of W the constant 8, the other
    K - 1 columns N(0, 1) against N(0, 1 / (K - 1)): every projected q and k head row is 64 + a spread of about 1 (R = 64)."""
    c = QKV
    gen = torch.Generator().manual_seed(seed_of(c["name"]))
    M, N, K = c["M"], c["N"], c["K"]
    a = torch.randn(M, K, generator=gen)
    w = torch.randn(N, K, generator=gen) / math.sqrt(K - 1)
    a[:, 0] = 8.0
    w[:2 * N // 3, 0] = 8.0
    w[2 * N // 3:, 0] = 0.0
    ang = torch.rand(M - c["text_rows"], 32, generator=gen).repeat_interleave(2, 1) * 6.3
    p = [_param(gen, 64, 1.0, 0.2), _param(gen, 64, 0.0, 0.5), _param(gen, 64, 1.0, 0.2), _param(gen, 64, 0.0, 0.5)]
    return dict(a=a.to(BF), w=w.to(BF), bias=torch.zeros(N).to(BF), qw=p[0], qb=p[1], kw=p[2], kb=p[3], cos=torch.cos(ang).contiguous(),
                sin=torch.sin(ang).contiguous())


def qkv_projected(dat):
    """The projection's q and k head rows as the bf16 values q/k-norm reads -> [M * 2 * heads, 64]."""
    y = (dat["a"].double() @ dat["w"].double().T + dat["bias"].double()).to(BF)
    return y[:, :2 * QKV["N"] // 3].reshape(-1, 64)


# ------------------------------------------------------------------------------------------------------------ router scores
SCORES_CASES = [c for c in xs.SCORES_CASES if c["name"] in ("wave-2x150", "lds-3x4099")]


def scores_data(c):
    """exact_step.scores_data's one-hot keys (feature f of identity i reads column src[i][f] of qr), the columns behind them filled
    with this module's rows: token n of identity i holds spec n + 5 i.  pos = 0 and the LayerNorm's parameters drawn: the output is
    the LayerNorm of the row alone.  eps is the caller's 1e-5."""
    base = xs.scores_data(c)
    gen = torch.Generator().manual_seed(seed_of(c["name"]) + 1)
    n_id, N = c["n_id"], c["N"]
    qr = base["qr"].clone()
    x = torch.stack([rows(N, 512, seed_of(c["name"]) + i, EPS_LN, first=5 * i) for i in range(n_id)])      # [n_id, N, 512]
    for i in range(n_id):
        qr[:, torch.from_numpy(base["src"][i])] = x[i]
    fam = torch.stack([torch.tensor([FAMILIES.index(spec_of(5 * i + n)["family"]) for n in range(N)]) for i in range(n_id)])
    return dict(qr=qr.contiguous(), kr=base["kr"], ln_w=_param(gen, 512, 1.0, 0.2), ln_b=_param(gen, 512, 0.0, 0.5), pos=torch.zeros(N, 512).to(BF),
                x=x, fam=fam[:, :, None])


def scores_ref64(dat, dev="cpu"):
    return xn.ln_reference64(dat["x"].to(dev), EPS_LN, dat["ln_w"].to(dev), dat["ln_b"].to(dev))


def scores_restate(dat, stats=None):
    x = dat["x"].float()
    if stats is None:
        return F.layer_norm(x, (512,), dat["ln_w"].float(), dat["ln_b"].float(), EPS_LN).to(BF)
    mean, var = stats
    return ((x - mean.view(*x.shape[:-1], 1)) * torch.rsqrt(var.view(*x.shape[:-1], 1) + np.float32(EPS_LN)) * dat["ln_w"].float() + dat["ln_b"].float()).to(BF)


# ------------------------------------------------------------------------------------------------------------ folded-LayerNorm row kernels
ROW_M = 129
W_MEAN = {"zero-mean": 0.0, "mean-0.05": 0.05}
W_STD = 0.05


def fold_weights(N, wset, seed):
    """The un-folded Linear [N, 512], its bias and the LayerNorm's gamma, beta (bf16 / fp32 as pack_rowgemm512 takes them): W's
    entries N(mean, 0.05^2) with mean 0 or 0.05, so that s = rowsum(W gamma) is about 0 +- 1.2 or about 25.6."""
    gen = torch.Generator().manual_seed(seed)
    w = (W_MEAN[wset] + W_STD * torch.randn(N, 512, generator=gen)).to(BF)
    return dict(w=w, b=(0.5 * torch.randn(N, generator=gen)).float(), gamma=_param(gen, 512, 1.0, 0.1), beta=_param(gen, 512, 0.0, 0.3))


def fold_host(wd):
    """What pack_rowgemm512 computes, on the CPU -> (Wg bf16 [N, 512], s fp32 [N], c fp32 [N])."""
    wg = (wd["w"].float() * wd["gamma"].float()).to(BF)
    return wg, wg.float().sum(1), wd["w"].float() @ wd["beta"].float() + wd["b"]


def gelu64(v):
    return xr.gelu64(v)


def fold_ref64(x, wg, cvec, eps, gelu=False, res=None, dev="cpu"):
    """LN(x) . Wg^T + c in fp64 from the packed operands the kernel reads, GELU(erf), + res -> fp64 [M, N]."""
    xd = x.to(dev).double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    y = ((xd - mean) / torch.sqrt(var + eps)) @ wg.to(dev).double().T + cvec.to(dev).double()
    if gelu:
        y = gelu64(y)
    return y if res is None else y + res.to(dev).double()


def fold_restate32(x, wg, cvec, eps, gelu=False, res=None, stats=None):
    """The same in fp32, centred: F.layer_norm without affine, the product and the epilogue in fp32 (not yet rounded)."""
    xf = x.float()
    if stats is None:
        n = F.layer_norm(xf, (512,), None, None, eps)
    else:
        n = (xf - stats[0]) * torch.rsqrt(stats[1] + np.float32(eps))
    y = n @ wg.float().T + cvec.float()
    if gelu:
        y = F.gelu(y)
    return y if res is None else y + res.float()


def _rg(N, res_gelu, wset):
    carve = ("offset R8",) if (N, res_gelu, wset) == (1536, True, "mean-0.05") else ()
    return dict(name=f"rowgemm-N{N}-{'res-gelu' if res_gelu else 'plain'}-{wset}", N=N, M=ROW_M, res=res_gelu, gelu=res_gelu, wset=wset, eps=EPS_LN,
                carve=carve)


ROWGEMM_CASES = [_rg(N, rg, ws) for N in (64, 512, 1536) for rg in (False, True) for ws in W_MEAN]


def rowgemm_data(c):
    seed = seed_of(c["name"])
    gen = torch.Generator().manual_seed(seed + 2)
    wd = fold_weights(c["N"], c["wset"], seed + 1)
    res = torch.randn(c["M"], c["N"], generator=gen).to(BF) if c["res"] else None
    return dict(wd, x=rows(c["M"], 512, seed, c["eps"]), res=res, fam=family_index(c["M"])[:, None])


def constant_rows_bound(x, wg, eps, K=512):
    """The bound on |y - c| of the one-pass kernels on a CONSTANT row x = a (before the activation and the residual), from their
    arithmetic  y = rstd (acc - mean s) + c:
      * sum x = K a and sum x^2 = K a^2 are exact in fp32 for the constants used (a in {3, 50}: K a^2 <= 1 280 000 < 2^24), so
        mean = a and var = max(a^2 - a a, 0) = 0 exactly, contracted or not, and rstd = rsqrtf(eps) <= (1 + 2^-22) / sqrt(eps);
      * acc = fl(sum_k a Wg[k]) accumulated in fp32 in some order: |acc - a sum Wg| <= K u |a| sum |Wg|  (u = 2^-24);
      * s = fl(sum Wg), summed in fp32 by the packer: |s - sum Wg| <= K u sum |Wg|, so |mean s - a sum Wg| <= K u |a| sum |Wg|;
      * the subtraction (or the fma) rounds once: u (|acc| + |a s|) <= 2 u |a| sum |Wg| (1 + K u);
      * rstd * (...) + c rounds once or twice more, relative to a result that the bound below already dominates.
    |y - c| <= (1 + 2^-22) / sqrt(eps) * |a| * sum |Wg| * u * (2 K + 3)   per output column.  Loose by the factor K of a worst-case
    summation bound (the expected error grows with sqrt(K)).  With sum |Wg| about 30 it is about 29 at a = 50, against outputs of
    order 1: there it has no more power than the finiteness check.  At a = 3 it is about 1.7, which a kernel that scales cvec or
    drops the mean term (|3 s rstd| = 2.4e4 at s = 25.6) misses; the two constants are asserted apart.  -> fp64 [rows, N]."""
    a = x.double().abs().amax(-1, keepdim=True)
    return (1 + 2.0 ** -22) / math.sqrt(eps) * a * wg.double().abs().sum(1)[None] * U32 * (2 * K + 3)


# ---- group attention with one key (L = 1): softmax = 1, the output is bf16(v) = bf16(LN(x) . Wv^T + cv)
ATTN = dict(name="group-attn-L1", **xr.multi_id(1, ROW_M), wset="mean-0.05", eps=EPS_LN)
# chains: the out-projection / mlp[2] is 2^40 I with no bias, so out = bf16(2^40 a + x) with a the bf16 value in registers: a's own
# bf16 step is the output's step whatever the row's offset.  |x| <= 2^6 * 2^6 * 1.1 < 2^13 is 2^-21 of the floor 2^-6 * 2^40: the
# residual (which the exact-data tests pin) cannot move 2^40 a into another binade, where a's step would count double.
CHAIN_SCALE = 2.0 ** 40
ATTN_OUT = dict(name="group-attn-out-L1", **xr.multi_id(1, ROW_M), wset="mean-0.05", eps=EPS_LN, tp0=0)
MLP_CASES = [dict(name="mlp-M300", M=300, tp0=0, passes=1, wset="mean-0.05", eps=EPS_LN),
             dict(name="mlp-M4388-tp1", M=4388, tp0=1, passes=2, wset="zero-mean", eps=EPS_LN)]       # 275 tiles: 256 + a remainder pass of 19


def attn_data(c):
    seed = seed_of(c["name"])
    wd = fold_weights(1536, c["wset"], seed + 1)
    return dict(wd, x=rows(c["M"], 512, seed, c["eps"]), fam=family_index(c["M"])[:, None])


def mlp_data(c):
    seed = seed_of(c["name"])
    wd = fold_weights(512, c["wset"], seed + 1)
    return dict(wd, x=rows(c["M"], 512, seed, c["eps"]), fam=family_index(c["M"])[:, None])


def chain_weight():
    """(W2 = 2^40 I bf16 [512, 512], b2 = 0 fp32 [512])."""
    return (torch.eye(512) * CHAIN_SCALE).to(BF), torch.zeros(512)


def chain_ref64(x, inner64, dev="cpu"):
    """x + 2^40 bf16(inner): the chain with the value it keeps in registers rounded to bf16, as its two-launch definition does."""
    return x.to(dev).double() + CHAIN_SCALE * inner64.to(BF).double()


def chain_restate(x, inner32):
    return (x.float() + np.float32(CHAIN_SCALE) * inner32.to(BF).float()).to(BF)


# ------------------------------------------------------------------------------------------------------------ GroupNorm
GN_LARGE_ROWS = 262144 + 513


def _gn(C, form, act, shape=(27, 1, 19), lat=(3, 1, 19), tmode=1):
    T, H, W = shape
    return dict(name=f"gn-C{C}-{T * H * W}-{form}-{act}", C=C, T=T, H=H, W=W, groups=xv.GROUPS, eps=EPS_VAE, form=form, act=act,
                lat=lat if form == "mod" else None, tmode=tmode, out_pad=False)


# 513 rows: two blocks of the partial kernel, the second with one row.  262 657 rows at C = 128: 514 blocks, so that every thread of
# the final kernel adds at least two partials before its tree.
GN_CASES = [_gn(32, "plain", "none"), _gn(32, "mod", "silu"), _gn(128, "plain", "silu"), _gn(128, "mod", "none"), _gn(512, "plain", "none"),
            _gn(512, "mod", "silu"), _gn(128, "plain", "none", shape=(1, 1, GN_LARGE_ROWS))]


def gn_fam(c):
    """Family of every channel's group -> int64 [1, C] (group g holds spec g)."""
    cg = c["C"] // c["groups"]
    return family_index(c["groups"]).repeat_interleave(cg)[None]


def gn_data(c):
    """-> exact_vae.norm_data's dict: x [T, H, W, C] bf16 (group g's rows x cg elements are one row of spec g), gamma, beta, zyb
    [latent rows, 2 C] or None, zr."""
    seed = seed_of(c["name"])
    gen = torch.Generator().manual_seed(seed)
    C, G = c["C"], c["groups"]
    n, cg = c["T"] * c["H"] * c["W"], C // G
    x = torch.empty(n, C, dtype=BF)
    for g in range(G):
        x[:, g * cg:(g + 1) * cg] = draw_row(spec_of(g), n * cg, gen, c["eps"]).view(n, cg).to(BF)
    dat = dict(x=x.view(c["T"], c["H"], c["W"], C), gamma=_param(gen, C, 1.0, 0.2), beta=_param(gen, C, 0.0, 0.5), zyb=None, zr=None)
    if c["form"] == "mod":
        Tz, hz, wz = c["lat"]
        nl = Tz * hz * wz
        dat["zyb"] = torch.cat([_param(gen, nl * C, 1.0, 0.2).view(nl, C), _param(gen, nl * C, 0.0, 0.5).view(nl, C)], 1).contiguous()
        dat["zr"] = xv.latent_rows(c["T"], c["H"], c["W"], Tz, hz, wz, c["tmode"])
    return dat


def gn_ref64(c, dat, dev="cpu"):
    y = xv.norm_reference(c, dat, dev)
    return xv.silu64(y) if c["act"] == "silu" else y


def gn_restate(c, dat, dev="cpu"):
    """F.group_norm in fp32 over the chunk (channels first, one sample), the modulation and SiLU in fp32, rounded once."""
    C = c["C"]
    x = dat["x"].to(dev).float().view(-1, C)
    y = F.group_norm(x.T[None], c["groups"], dat["gamma"].to(dev).float(), dat["beta"].to(dev).float(), c["eps"])[0].T
    if dat["zyb"] is not None:
        z = dat["zyb"].to(dev).float()
        r = dat["zr"].to(dev)
        y = y * z[r, :C] + z[r, C:]
    if c["act"] == "silu":
        y = F.silu(y)
    return y.to(BF)


def gn_sum_depth(c):
    """Additions on the longest path of one group's sum in vae_gn_partial_kernel and its final kernel: rows per thread
    (512 cpr / 256), threads per channel (256 / cpr), channels per group, partials per thread of the final kernel, its tree of 8."""
    cpr = c["C"] // 8
    n = c["T"] * c["H"] * c["W"]
    blocks = (n + 511) // 512
    return 512 * cpr // 256 + 256 // cpr + c["C"] // c["groups"] + (blocks + 255) // 256 + 8


def gn_constant_bound(c, dat, const):
    """|y - beta| of a CONSTANT group x = a before the modulation and the activation.  A sum of equal-signed terms along a tree of
    depth h has relative error <= h u (1 + h u), so sum x / count = a (1 + t1) and sum x^2 / count = a^2 (1 + t2) with |t| <= (h + 2) u =: T
    (the count's conversion and the division add one rounding each).  Then |x - mean| <= |a| T (1 + u), rstd <= (1 + 2^-22) / sqrt(eps)
    (var is clamped at 0 from below), and the products with rstd and gamma add relative roundings that the factor 1.001 covers:
    |y - beta| <= 1.001 |a| (h + 2) u |gamma| / sqrt(eps)   -> fp64 [C] (per channel, for a group that holds the constant ``const``)."""
    h = gn_sum_depth(c)
    return 1.001 * abs(const) * (h + 2) * U32 * dat["gamma"].double().abs() / math.sqrt(c["eps"])
