"""Exact-data checking of the Embedding Router's K = 512 row kernels (a plain helper module: no tests, no fixtures; the sibling
of ``exact_gemm.py`` and ``exact_attn.py``, whose ``GuardedOut`` / ``bad_elements`` / ``describe`` / ``assert_exact`` /
``strided`` / ``pow2`` it reuses).  csrc/rowgemm.hip (rowgemm512_kernel, rowgemm512q_kernel, rowattn512_kernel<wide>) and
csrc/rowchain.hip (router_mlp_chain_kernel, router_attn_chain_kernel) share the code that decides their bits
(csrc/rowgemm_common.h), so comparing them with each other cannot see a fault in it.  Here every case has data for which a correct
kernel's answer is a function of the data alone, the check is bit equality with an fp64 reference rounded once to bf16, and a
failure names the element and its tile.  All data is made on the CPU from a seed (the CPU tests check the same tensors).

PLAIN LINEAR (no LayerNorm, no GELU; ``plain_data``): ``exact_gemm.exact_operands`` with K = 512: every product is a multiple of
2^-2 of magnitude <= 36, any partial sum of 512 of them a multiple of 2^-2 below 512 * 36 = 18432 < 2^15, i.e. below 2^17 units:
exact in fp32 in every order.  The kernel adds c (the bias, ``exact_epilogue``: a multiple of 2^-2 of at most 4), then the residual
(a multiple of 2^-3 of at most 8): acc + c is a multiple of 2^-2 below 2^15 + 4, + res a multiple of 2^-3 below 2^15 + 12 < 2^18
units -- every value before the one rounding to bf16 is exact.  Reference: fp64, rounded once.

LAYERNORM FOLDED IN (``folded_data``).  The kernel computes rstd * (x . Wg^T - mean * s) + c with rstd = rsqrtf(var + eps), and the
last bit of the device's rsqrtf is not known; the data takes it out of the answer.  Row m is x[m, k] = mu[m] + d[m] * e[m, k] with mu
an integer in [-4, 4], d in {1, 2, 4} and e[m, :] integers with sum 0 and sum of squares 512 exactly: 256 entries +1 and 256 -1 in a
seeded order, or (every other row of the Linear cases) 32 x +2, 32 x -2, 128 x +1, 128 x -1 and 192 zeros.  |x| <= 12: exact in
bf16; sum x = 512 mu and sum x^2 = 512 (mu^2 + d^2) are exact on the matrix core, mean = mu and var = d^2 exactly (with or without
contraction of sq / 512 - mu * mu), the true rstd at eps = 0 is 1 / d and LN(x) is the pattern e itself.  gamma is a power of two
per column (1/2, 1, 2), the un-folded weight W = Wg / gamma for an integer Wg, so pack_rowgemm512's W * gamma rounds to Wg exactly;
beta is an even integer in [-2, 2] (W beta is then an integer although W may hold halves) and the bias is chosen so that c is the
integer the case wants.  Wg is THIN: 32 entries +-1 and 8 entries +-2 per output column, sum |Wg| = 48, so |e . Wg| <= 96; c has
alternating sign per column and magnitude 110 .. 140.  The true y = e . Wg^T + c is then an integer with 14 <= |y| <= 236 < 256: a
bf16 number, the nearest rounding boundary >= 2^-9 |y| away.  In the kernel x . Wg^T = mu s + d (e . Wg) (an integer below 12 * 48
* ... <= 12288: exact), fmaf(-mean, s, acc) = d (e . Wg) exactly, and rstd off by an ulp moves the result by at most
96 * 2^-23 + one fp32 rounding < 2^-16 -- far inside the margin, PROVIDED y != 0 (at y = 0 the result would be c (1 - d rstd), a
tiny non-zero number): that is why c clears |e . Wg| on every element.  Residual: integers |r| <= 7, so 7 <= |y + r| < 256 as well.
``emulate_fold`` evaluates the kernel's expression in fp32 with rstd one ulp either side and with and without fma for EVERY element
(test_rowk_exact_cpu.py); ``assert_fold_conditions`` asserts integer y and the bounds on every case.
eps: 0 for the Linears and the MLP chain.  The group-attention kernels read the unused slots of a tile as rows of zeros, whose
rstd at eps = 0 is infinite and whose v = inf * 0 is NaN -- and NaN * (P = 0) poisons the tile's P.V product.  A positive eps
never shows that (every caller passes 1e-5), so those cases use ``EPS_ATTN`` = 2^-30: fp32 d^2 + 2^-30 == d^2 for d^2 >= 1 (half
an ulp of 1 is 2^-24), rstd is what eps = 0 gives, and an empty slot's rstd is 2^15.

GELU(erf) (``folded_data(gelu=True)``, with or without LayerNorm; without it x is the pattern e itself).  rowk::gelu_erf_f returns v
exactly for v >= 8 and -0 for v <= -8: there exp2(-1.44 ax^2) < 2^-40, erf_abs rounds to 1.0f, and 0.5 v (1 +- 1) is v or -0.  The
pre-activations above are integers with 14 <= |v| < 256, their sign alternating by column.  Why 14 and not 8 on the negative side:
the TRUE GELU(-8) is -5e-15, a bf16 number (bf16 has fp32's exponent range), where the kernel's erf (absolute error 1.5e-7 by
design) returns -0; below -13.6 the true value is under half of bf16's smallest subnormal and rounds to -0 too.  So fp64 GELU
(0.5 v erfc(-v / sqrt 2), no cancellation) rounded to bf16 is v or -0 -- asserted.  The curved part of GELU stays with the tolerance
tests of test_kernels_gpu.py.

MLP CHAIN (``mlp_data``): the hidden h = GELU(...) is an integer in {0} u [14, 236], exact in bf16 (the kernel's h, v (1 +- 2^-22),
rounds to it).  W2 and b2 are on exact_gemm's grid (|W2| <= 6 a multiple of 2^-1; b2 a multiple of 2^-2): every product is a
multiple of 2^-1 below 236 * 6 = 1416, any partial sum of 512 below 725000 < 2^20, i.e. 2^21 units; + b2 + x (integers <= 12):
below 2^22 units of 2^-2 -- exact in fp32, rounded once.

GROUP ATTENTION (``attn_data``; ``scale = exact_attn.UNIT_SCALE``, rows of +-1 patterns only).  Because LN(x) = e, the packed q|k|v
weight turns chosen positions of e into chosen q, k, v; every q, k, v below is an integer or a half of magnitude < 8, so the bf16
rounding in the kernel removes the rstd ulp (an element with c = 0 whose product is 0 is exactly 0; one with c != 0 is never 0).
  * v: a thin Wv (3 entries +-1 per column, |e . Wv| <= 3) and c = +-4 with one sign per column, rotated by head: 1 <= |v| <= 7.
  * uniform: Wk = 0 and bk = 0, all scores are 0 (q, from a dense +-1 Wq, only has to be finite), P = 1, l = L, and for L in {1, 2, 4,
    8, 16}  O = sum(V) / L  is a multiple of 1/16 of magnitude in [1, 7]: 7 significant bits, a bf16 number.  Every key of another
    group of the tile left unmasked changes it.
  * levels: member j of a group has a score level from ``exact_attn.pattern(L)`` (weights 2^level sum to a power of two) written
    into e at two code positions (e[P0] + 2 e[P1] = -3 - 2 level).  Per head, four features carry it: k = g_f (e[P0] + 2 e[P1]) / 2
    with g = (-1, -1, 2, -1) against q = (1, 2, 3, 4) (bias only), so q . k = level + 3/2 -- only in THAT pairing of features; one
    feature has q = a thin product of e (a different integer per query row: a row-constant term of the score) against k = 1; two
    have q = (2, -1) against k = (t, 2 t), t a thin product of e per key, which cancel.  The feature positions rotate with the
    head.  Score differences are exact small integers; O = sum_j 2^level_j v_j / sum_j 2^level_j is a multiple of 1/32 of magnitude
    in [1, 7]: at most 8 significant bits, never 0.
  The margin, as in exact_attn.py: the expected value is a bf16 number, the nearest boundary >= 2^-9 |O| away; v_exp / v_rcp and
  scale * log2(e) cost a few fp32 ulps.  The CPU condition: fp64 softmax of the same q, k, v within 2^-16 |O| of the closed form.
  * attention chain: the out-projection adds a . Wo^T + bo + x with a = O (a multiple of 2^-5, |a| <= 7) and Wo, bo on
    exact_gemm's grid: products are multiples of 2^-6 below 42, partial sums of 512 below 21504 < 2^15, i.e. 2^21 units; + bo + x
    (multiples of 2^-2, <= 16): exact in fp32, rounded once.
Queries of one group share their output row (scores differ by a row constant only); the chain's residual tells them apart.

Which kernel a case runs is asserted through the plan queries (ops.rowgemm512_plan, router_mlp_fused_plan,
router_group_attn_plan, router_group_attn_out_plan) before the launch; W-stationary wave shares, which the kernel derives on the
device, are modelled by ``wstat_wave_tiles``.
"""
import math

import numpy as np
import torch

import exact_gemm
from exact_attn import UNIT_SCALE, pattern
from exact_gemm import BF, GuardedOut, assert_exact, bad_elements, describe, pow2, strided  # noqa: F401  (re-exported)

K = 512
EPS_LN = 0.0
EPS_ATTN = 2.0 ** -30
P0, P1 = 5, 300                          # code positions of a key's level in e
CODE_OF_LEVEL = {0: (-1, -1), -1: (1, -1), -2: (-1, 1), -3: (1, 1)}        # e[P0] + 2 e[P1] = -3 - 2 level
Q_LEVEL, K_LEVEL = (1, 2, 3, 4), (-1, -1, 2, -1)                           # sum q g = -1
assert sum(a * g for a, g in zip(Q_LEVEL, K_LEVEL)) == -1
assert all(a + 2 * b == -3 - 2 * lv for lv, (a, b) in CODE_OF_LEVEL.items())


# ------------------------------------------------------------------------------------------------------------ patterns
def patterns(M, rng, rich=False, codes=None):
    """e [M, 512] int64: rows with sum 0 and sum of squares 512.  ``rich``: odd rows take the +-2 / +-1 / 0 multiset.  ``codes``
    [M, 2] (+-1): the values at P0, P1 (+-1 rows only)."""
    e = np.empty((M, K), np.int64)
    free = np.array([k for k in range(K) if codes is None or k not in (P0, P1)])
    plus = np.full(M, 256) - (0 if codes is None else (codes == 1).sum(1))
    rank = rng.random((M, len(free))).argsort(1).argsort(1)
    e[:, free] = np.where(rank < plus[:, None], 1, -1)
    if codes is not None:
        e[:, P0], e[:, P1] = codes[:, 0], codes[:, 1]
    if rich:
        multiset = np.array([2] * 32 + [-2] * 32 + [1] * 128 + [-1] * 128 + [0] * 192)
        odd = np.arange(1, M, 2)
        e[odd] = multiset[rng.random((len(odd), K)).argsort(1)]
    assert (e.sum(1) == 0).all() and ((e * e).sum(1) == K).all()
    return torch.from_numpy(e)


def rows_of(e, rng):
    """x = mu + d e (bf16, exact) -> (x, mu, d)."""
    M = e.shape[0]
    mu = torch.from_numpy(rng.randint(-4, 5, (M, 1)))
    d = torch.from_numpy(rng.choice([1, 2, 4], (M, 1)))
    x = (mu + d * e).to(BF)
    assert torch.equal(x.double(), (mu + d * e).double())
    return x, mu, d


def thin(N, rng, ones, twos=0):
    """Integer weight [N, 512] with ``ones`` entries +-1 and ``twos`` entries +-2 per row at seeded positions."""
    w = np.zeros((N, K), np.int64)
    pos = rng.random((N, K)).argsort(1)[:, :ones + twos]
    val = rng.choice([-1, 1], (N, ones + twos)) * np.array([1] * ones + [2] * twos)
    np.put_along_axis(w, pos, val, 1)
    return torch.from_numpy(w)


def fold(wg, c_want, rng, ln):
    """The un-folded Linear (W, b, gamma, beta) whose pack has Wg = ``wg`` (exact in bf16) and c = ``c_want``."""
    if not ln:
        return wg.to(BF), c_want.float(), None, None
    gamma = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], K))
    beta = torch.from_numpy(2.0 * rng.randint(-1, 2, K))
    w = wg.double() / gamma
    b = c_want.double() - w @ beta
    assert torch.equal(w.to(BF).double(), w) and torch.equal(b.float().double(), b)
    return w.to(BF), b.float(), gamma.to(BF), beta.to(BF)


def gelu64(v):
    return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))


# ------------------------------------------------------------------------------------------------------------ Linears
def plain_data(M, N, res, seed):
    a, w = exact_gemm.exact_operands(M, N, K, "cpu", seed=seed)
    ep = exact_gemm.exact_epilogue(w, "cpu", seed + 7, bias=True, res_rows=M if res else None)
    r = ep["res"][0] if res else None
    ref = exact_gemm.reference(a, w, bias=ep["bias"], res=r)
    return dict(x=a, w=w, b=ep["bias"].float(), gamma=None, beta=None, r=r, ref=ref, ln=False, gelu=False)


def folded_data(M, N, ln, gelu, res, seed):
    """LayerNorm and / or GELU Linear on the thin grid of the module docstring -> dict with x, the un-folded w, b, gamma, beta,
    r, the integer pre-activation y and the pieces ``emulate_fold`` needs."""
    rng = np.random.RandomState(seed)
    e = patterns(M, rng, rich=True)
    if ln:
        x, mu, d = rows_of(e, rng)
    else:
        x, mu, d = e.to(BF), torch.zeros(M, 1, dtype=torch.int64), torch.ones(M, 1, dtype=torch.int64)
    wg = thin(N, rng, 32, 8)
    sign = torch.where(torch.arange(N) % 2 == 0, 1, -1)
    c = sign * torch.from_numpy(rng.randint(110, 141, N))
    w, b, gamma, beta = fold(wg, c, rng, ln)
    t = (e.double() @ wg.double().T).long()                          # e . Wg (exact in fp64)
    y = t + c
    r = torch.from_numpy(rng.randint(-7, 8, (M, N))) if res else None
    out = gelu64(y.double()) if gelu else y.double()
    ref = out + r.double() if res else out
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, r=None if r is None else r.float(), ref=ref, ln=ln, gelu=gelu,
                y=y, t=t, c=c, d=d, mu=mu, e=e, wg=wg)


def assert_fold_conditions(dat):
    y = dat["y"]
    assert int(y.abs().min()) >= 14 and int(y.abs().max()) <= 236, (int(y.abs().min()), int(y.abs().max()))
    assert int(dat["t"].abs().max()) <= 96
    assert torch.equal(dat["x"].double(), (dat["mu"] + dat["d"] * dat["e"]).double())
    if dat["gelu"]:
        g = gelu64(y.double()).to(BF).double()
        assert torch.equal(g, torch.where(y > 0, y.double(), torch.zeros(()).double())), "fp64 GELU rounded to bf16 is not v or 0"
    tot = dat.get("fold_ref", dat["ref"])
    assert torch.equal(tot, tot.round()) or dat["gelu"]
    assert float(tot.abs().max()) < 256
    if not dat["gelu"]:
        assert float(tot.abs().min()) >= 7


def emulate_fold(dat, ulp, fma):
    """The kernel's expression in fp32 for every element, rstd = fl(1 / d) moved by ``ulp`` ulps, contracted or not -> bf16."""
    f32 = lambda v: v.float().double()
    rstd = (1.0 / dat["d"].double()).float()
    for _ in range(abs(ulp)):
        rstd = torch.nextafter(rstd, torch.full_like(rstd, 2.0 if ulp > 0 else 0.0))
    prod = rstd.double() * (dat["d"] * dat["t"]).double()            # fmaf(-mean, s, acc) = d (e . Wg), exact; this product is exact in fp64
    c = dat["c"].double()
    o = f32(prod + c) if fma else f32(f32(prod) + c)
    if dat["gelu"]:
        assert bool((o.abs() >= 8).all())
        o = torch.where(o > 0, o, -torch.zeros_like(o))              # rowk::gelu_erf_f outside (-8, 8)
    if dat["r"] is not None:
        o = f32(o + dat["r"].double())
    return o.to(BF)


def mlp_data(M, seed):
    d1 = folded_data(M, 512, True, True, False, seed)
    h = torch.where(d1["y"] > 0, d1["y"], torch.zeros((), dtype=torch.int64)).double()
    _, w2 = exact_gemm.exact_operands(1, 512, K, "cpu", seed=seed + 3)
    b2 = exact_gemm.exact_epilogue(w2, "cpu", seed + 5, bias=True)["bias"].float()
    ref = h @ w2.double().T + b2.double() + d1["x"].double()
    assert float(h.max()) <= 236 and float(ref.abs().max()) < 2 ** 20
    return dict(d1, h=h, w2=w2, b2=b2, ref=ref, fold_ref=d1["ref"])


# ------------------------------------------------------------------------------------------------------------ group attention
def group_rows(L, n_outer, n_inner, outer_stride, seq_stride):
    o = torch.arange(n_outer)[:, None, None] * outer_stride
    i = torch.arange(n_inner)[None, :, None]
    return (o + i + torch.arange(L)[None, None, :] * seq_stride).reshape(-1, L)         # [groups, L] row indices


def head_features(h):
    """Feature positions of head h: 4 level features, the row-constant one, the cancelling pair (all distinct)."""
    f = [int(v) for v in np.random.RandomState(100 + h).permutation(64)[:7]]         # distinct, different in every head
    return f[:4], f[4], f[5:]


def attn_data(kind, L, n_outer, n_inner, outer_stride, seq_stride, M, seed, chain=False):
    """-> dict: x, the un-folded packed Linear (w [1536, 512], b, gamma, beta), rows [groups, L], q, k, v [M, 512] fp64 (exact),
    want [groups, L, 512] fp64 (the closed form, a bf16 number), and with ``chain`` wo, bo and ref [M, 512] of the touched rows."""
    rng = np.random.RandomState(seed)
    rows = group_rows(L, n_outer, n_inner, outer_stride, seq_stride)
    G = rows.shape[0]
    assert rows.max() < M and len(torch.unique(rows)) == rows.numel()
    level = np.zeros((G, L), np.int64)
    if kind == "levels":
        for g in range(G):
            level[g] = rng.permutation(pattern(L, g))
    codes = rng.choice([-1, 1], (M, 2))
    lut = np.array([CODE_OF_LEVEL[-i] for i in range(4)])
    codes[rows.reshape(-1).numpy()] = lut[-level.reshape(-1)]
    e = patterns(M, rng, codes=codes)
    x, mu, d = rows_of(e, rng)
    wg = torch.zeros(1536, K, dtype=torch.float64)
    c = torch.zeros(1536, dtype=torch.float64)
    wg[1024:] = thin(512, rng, 3).double()
    base_sign = torch.from_numpy(rng.choice([-1.0, 1.0], 64))
    for h in range(8):
        c[1024 + 64 * h:1088 + 64 * h] = 4.0 * base_sign[(torch.arange(64) + 5 * h) % 64]
    if kind == "uniform":
        wg[:512] = torch.from_numpy(rng.choice([-1.0, 1.0], (512, K)))
    else:
        for h in range(8):
            lev, const, pair = head_features(h)
            for i, f in enumerate(lev):
                c[64 * h + f] = Q_LEVEL[(i + h) % 4]
                wg[512 + 64 * h + f, P0], wg[512 + 64 * h + f, P1] = K_LEVEL[(i + h) % 4] / 2, K_LEVEL[(i + h) % 4]
            wg[64 * h + const] = thin(1, rng, 3)[0].double()
            c[512 + 64 * h + const] = 1.0
            t = thin(1, rng, 3)[0].double()
            c[64 * h + pair[0]], c[64 * h + pair[1]] = 2.0, -1.0
            wg[512 + 64 * h + pair[0]], wg[512 + 64 * h + pair[1]] = t, 2 * t
    w, b, gamma, beta = fold(wg, c, rng, True)
    qkv = e.double() @ wg.T + c
    q, k, v = qkv[:, :512], qkv[:, 512:1024], qkv[:, 1024:]
    wt = torch.from_numpy(np.exp2(level.astype(np.float64)))
    wt = wt / wt.sum(1, keepdim=True)                                                    # [G, L], powers of two
    o = torch.einsum("gj,gjc->gc", wt, v[rows])                                          # the same row for every query of a group
    want = o[:, None, :].expand(G, L, 512).contiguous()
    out = dict(x=x, w=w, b=b, gamma=gamma, beta=beta, rows=rows, q=q, k=k, v=v, want=want, level=level, L=L, kind=kind)
    if chain:
        _, wo = exact_gemm.exact_operands(1, 512, K, "cpu", seed=seed + 3)
        bo = exact_gemm.exact_epilogue(wo, "cpu", seed + 5, bias=True)["bias"].float()
        out.update(wo=wo, bo=bo, ref=want.reshape(-1, 512) @ wo.double().T + bo.double() + x.double()[rows.reshape(-1)])
    return out


def assert_attn_conditions(dat):
    """q, k, v are what the docstring says, the closed form is a bf16 number and never 0."""
    q, k, v, want = dat["q"], dat["k"], dat["v"], dat["want"]
    for t in (q, k, v):
        assert torch.equal(t * 2, (t * 2).round()) and torch.equal(t.to(BF).double(), t)
    assert 1 <= float(v.abs().min()) and float(v.abs().max()) <= 7 and torch.equal(v, v.round())
    assert float(k.abs().max()) < 8 and (dat["kind"] == "uniform" or float(q.abs().max()) < 8)
    if dat["kind"] == "uniform":
        assert not bool(k.any())
    assert torch.equal(want.to(BF).double(), want) and float(want.abs().min()) >= 1 and float(want.abs().max()) <= 7


def attn_reference64(dat):
    """fp64 softmax (exp2 units) over each group and head of the same q, k, v -> [groups, L, 512]."""
    rows = dat["rows"]
    G, L = rows.shape
    q, k, v = (dat[n][rows].view(G, L, 8, 64).transpose(1, 2) for n in "qkv")
    s = q @ k.transpose(-1, -2)
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    o = (p @ v) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(G, L, 512)


# ------------------------------------------------------------------------------------------------------------ schedules
def wstat_wave_tiles(M):
    """rowgemm512q_kernel's share arithmetic: the 16-row tiles of each of the 8 waves of each of the 64 row groups."""
    tiles = (M + 15) // 16
    out = []
    for rg in range(64):
        g0, g1 = tiles * rg // 64, tiles * (rg + 1) // 64
        out += [(g0 + (g1 - g0) * (wv + 1) // 8) - (g0 + (g1 - g0) * wv // 8) for wv in range(8)]
    return out


# ------------------------------------------------------------------------------------------------------------ the GPU matrix
INSTANCES = [(ln, res, gelu) for ln in (False, True) for res in (False, True) for gelu in (False, True)]


def _g(M, N, ln, res, gelu, form="chunk_balanced", pad=128, chunked=False, crosses=None):
    name = f"M{M}-N{N}-{'ln' if ln else 'raw'}{'-res' if res else ''}{'-gelu' if gelu else ''}" + ("-chunked" if chunked else "")
    return dict(name=name, M=M, N=N, ln=ln, res=res, gelu=gelu, form=form, pad=pad, chunked=chunked, crosses=crosses)


# chunk-balanced: every instance at a small M, the sizes 15 / 129 / 300 over the widths, more work items than workgroups (M = 2831:
# 12 row blocks x 24 chunks = 288 items whose 256 ranges happen to end on the row-block boundaries; M = 3073: 312 items, ranges
# that hold chunks of two row blocks), and N = 512 without LayerNorm at M >= 2048 through the reference form
ROWGEMM_CASES = (
    [_g((15, 129, 300)[i % 3], (64, 512, 1536)[(i // 2) % 3], ln, res, gelu, pad=(128, 256)[i % 2])
     for i, (ln, res, gelu) in enumerate(INSTANCES)]
    + [_g(300, 64, True, True, False), _g(129, 512, False, False, False, pad=256), _g(15, 1536, True, False, True)]
    + [_g(2831, 1536, True, False, False, crosses=False), _g(2831, 1536, False, True, False, pad=256, crosses=False),
       _g(3073, 1536, True, True, True, crosses=True), _g(3073, 1536, False, False, False, pad=256, crosses=True)]
    + [_g(2049, 512, False, True, False, chunked=True), _g(2063, 512, False, False, True, chunked=True, pad=256)]
    # W-stationary: N = 512, the four instances at each M
    + [_g(M, 512, False, res, gelu, form="w_stationary", pad=(128, 256)[j % 2])
       for M in (2048, 2049, 2063, 4394) for j, (res, gelu) in enumerate([(False, False), (True, False), (False, True), (True, True)])]
    # ... and the router's own row count: waves with 4 and 5 tiles (an odd number of tile pairs' halves beyond one)
    + [_g(35100, 512, False, True, False, form="w_stationary")])

MLP_CASES = [dict(name=f"M{M}-tp{tp0}", M=M, tp0=tp0, pad=(128, 256)[i % 2])
             for i, (M, tp0) in enumerate([(15, 1), (300, 0), (2049, 3), (4388, 1), (4388, 0), (36960, 1)]
                                          + [(4388, t) for t in range(2, 9)])]


def _geom(name, L, n_outer, n_inner, outer_stride, seq_stride, extra=0):
    M = max((n_outer - 1) * outer_stride + (n_inner - 1) + (L - 1) * seq_stride + 1, 1) + extra
    return dict(geom=name, L=L, n_outer=n_outer, n_inner=n_inner, outer_stride=outer_stride, seq_stride=seq_stride, M=M)


def temporal(L, n_inner=169, n_outer=2):
    return _geom("temporal", L, n_outer, n_inner, L * n_inner, n_inner)


def multi_id(L, n_inner):
    return _geom("multi-id", L, 1, n_inner, 0, n_inner)


def trailing(L, n_outer=4, n_inner=77):
    return _geom("trailing+5", L, n_outer, n_inner, L * n_inner, n_inner, extra=5)


def _a(kind, geom, pad=128, tp0=None):
    c = dict(geom, kind=kind, pad=pad, tp0=tp0)
    c["name"] = f"{kind}-L{c['L']}-{c['geom']}" + ("" if tp0 is None else f"-tp{tp0}")
    return c


GROUP_ATTN_CASES = [
    _a("uniform", multi_id(1, 300)), _a("uniform", multi_id(2, 1111), pad=256), _a("uniform", temporal(4)),
    _a("uniform", temporal(8), pad=256), _a("uniform", trailing(16)), _a("uniform", multi_id(4, 333), pad=256),
    _a("levels", multi_id(2, 555)), _a("levels", multi_id(3, 1111), pad=256), _a("levels", temporal(13)),
    _a("levels", trailing(16), pad=256), _a("levels", _geom("ragged+3", 17, 2, 101, 17 * 101, 101, extra=3)),
    _a("levels", temporal(25, n_inner=45), pad=256), _a("levels", _geom("one-outer", 32, 1, 77, 0, 77)),
]
ATTN_OUT_CASES = [
    _a("uniform", multi_id(1, 300), tp0=0), _a("uniform", multi_id(2, 1111), tp0=1, pad=256), _a("levels", multi_id(3, 1111), tp0=6),
    _a("levels", temporal(13), tp0=0, pad=256), _a("levels", trailing(16), tp0=1), _a("levels", temporal(13), tp0=6),
    _a("levels", temporal(13), tp0=1, pad=256),          # 338 tiles on 256 workgroups: two passes
    _a("uniform", trailing(16), tp0=6, pad=256),
]


def geometry(c):
    return c["L"], c["n_outer"], c["n_inner"], c["outer_stride"], c["seq_stride"]


def seed_of(c):
    return sum(ord(ch) for ch in c["name"])
