"""Conditioning of the softmax inside the Embedding Router's fused row kernels (a plain helper module: no tests, no fixtures; the
sibling of ``cond_attn.py``, whose families, reference, measure and bars it uses unchanged, and of ``exact_rowk.py``, whose row
patterns, fold and geometries it uses).  csrc/rowgemm.hip (rowattn512_kernel<false> for L <= 16 in cells of P = 1, 2, 4, 8, 16 slots,
rowattn512_kernel<true> for 16 < L <= 32) and csrc/rowchain.hip (router_attn_chain_kernel) carry a softmax of their own: their own
key mask, cross-lane reductions, two-key-tile form and P^T packing.  exact_rowk.py holds it on probabilities that are powers of two
at UNIT_SCALE, where the rounding of P, v_rcp_f32 of a sum that is no power of two and exp2 of a large (s - mx) times a real scale
are all invisible; test_norm_cond_gpu.py runs it at L = 1, where there is no softmax.  Here every output element is held to the fp64
softmax of designed q, k, v at the production scale 0.125, on cond_attn's hard score rows.

THE ENCODING.  The kernels take x and a packed weight and round q | k | v to bf16 in registers after rstd * (x . Wg^T - mean s) + c
with an rsqrtf whose last bit is unknown.  The data takes that out, as exact_rowk.py does: rows are x = mu + d e with e an exact +-1
pattern of sum 0 (``exact_rowk.rows_of``, EPS_ATTN = 2^-30), LN(x) = e exactly, and a thin Wg reads CODE POSITIONS of e (NCODE = 132
of the 512, scattered by a fixed permutation; the other 380 balance the sum).  Every q, k, v element is a multiple of 1/2 of
magnitude below 8 (at most 4 significant bits): the nearest bf16 rounding boundary is >= 2^-9 |value| away and an rstd ulp moves a
value by < 2^-16 (``emulate`` evaluates the kernel's expression with rstd +-2 ulps, contracted or not, for every element).  A
designed zero comes only from a column with c = 0 whose products cancel exactly; a column with c != 0 has no entries (k's const
block) or never cancels (v).  A switch is a PAIR of code bits (a, b) read with one weight w: w (a + b) is 2 w, 0 or -2 w.  7.5 as
2 w needs w = 3.75: no sum of halves of +-1 bits reaches both 7.5 and 0 (the total 7.5 would have to split into two equal halves),
so Wg holds integers, halves and the quarter 3.75 (four significant bits; W = Wg / gamma stays a bf16 number for gamma 1/2, 1, 2).

The 64 features of a head are cut into blocks whose positions are a per-head permutation (``blocks_of``).  Scores in exp2 units
(q . k * 0.125 * log2 e):
    const   8 features   k = 5.5 (bias only)                            q = +-7.5 on shift-high / shift-low, else 0: +-59.5 under the row
    wide    2 x 8        k = one of four independent levels in          q = 7.5 on the first 8 (wide: +-81), on all 16 (large: +-162),
                         {-7.5, -6.5 .. 7.5} (4 bits; head h reads         2 on the first 8 (shifted rows: +-21.6), else 0
                         levels h % 4 and (h + 1) % 4); member 0 holds
                         +7.5 and member 1 -7.5 in all four
    peaks   3 x 4        k = 7.5 at ONE member (first, L // 2, last),   q = 7.5 on one of the three (peaked: 40.6 above the rest; the
                         else an exact 0                                   choice cycles), else 0
    noise   28           k = e[a] + e[b] / 2 in {+-0.5, +-1.5} on two   q = e[a] - e[b] on two bits of a 40-bit pool: the pool is all +1
                         bits of a 56-bit pool                             on flat rows (q = 0), 18 % -1 on the structured families (30 %
                                                                           of features non-zero), random on friendly (score sd 1.5)
Friendly rows have a score sd of 1.5 and not cond_attn's 3: the largest score of a row has P = 1 exactly, and with 4 or 8 keys at
sd 3 nearly all of a row's mass sits there, where a truncated P and a rounded one agree.  With q = 2 (e[a] - e[b]) the restatement with
P truncated gave b = -0.29 at L = 4 and -0.42 at L = 8 against bars (b) of 0.41 and 0.44 and passed; with q = e[a] - e[b] it gives
-0.61 and -0.91 against 0.37 and 0.38 and fails from L = 3 up (test_rowattn_cond_cpu.py asserts that on this data).
The family is chosen by the QUERY row: member i of group g takes family (i + g) mod 7 of ``cond_attn.families_of("tiny")``, so the
groups that share a 16-row tile hold different families.  Raw q . k products are multiples of 1/4 below 2^11: exact in fp32 in any
order, so what the bars see is the softmax.
V: integers e . Wv + c, Wv thin (3 entries +-1 anywhere in e), c = +4 on columns 0 .. 31 of every head (1 <= v <= 7: cond_attn's bias
bar needs one sign), +-4 on columns 32 .. 63.
EMPTY SLOTS (L < P, or L < 32 in the wide kernel) read rows of zeros: k = c_k (5.5 on the const block, 0 elsewhere), v = c_v = +-4.
A slot left unmasked scores like a real key of level 0 and drags O towards +-4.

REFERENCE: ``cond_attn.reference64`` on q * (0.125 log2 e) (fp64), k, v per (group, head).  RESTATEMENT (``restate``): fp32 raw
scores, row maximum, exp2((s - mx) * fl32(0.125 * fl32(log2 e))), fp32 row sum, P rounded to bf16, fp32 P . V, one multiplication by
the reciprocal, one rounding.  Planted faults: cond_attn's p_trunc, o_trunc, drop_last, and leak_next (the first key of the next
group of the tile unmasked), leak_empty (one empty slot unmasked, with the k and v the kernel reads there).
BARS: cond_attn's (a), (b), (c) through ``cond_attn.check``, eps = eps_of(L, 64, S_abs, tiny=True).  (d) (``exact_mask``): bit
equality with bf16(o64) where a correct kernel cannot differ: L = 1 (O = v); flat rows at L a power of two (P = 1, l = L, O a sum of
at most 32 integers <= 7 over a power of two); peaked rows (the other keys sit 25 or more exp2 units down, and v_peak + 7 * 31 *
2^-25 rounds to v_peak).
CHAIN BAR (``chain_data``, ``chain_check``): y64 = x + bo + sum_d o64_d Wo[n, d], Wo = N(0, 1) / sqrt(512), bo = N(0, 0.2), bf16;
    |got - y64| <= (1 + eps_attn) 2^-8 sum_d |Wo[n, d]| (A_d + |o64_d|) + (0.5 + eps_gemm) ulp_bf16(y64),
eps_gemm = cond_gemm.eps_of at K = 512 with the two epilogue additions, S = sum_d |o64_d Wo[n, d]| + |bo| + |x|.  Nothing in it comes
from a kernel; it is loose (it catches a wrong row, head, column or residual), bit identity with the two launches is the sharp check.
"""
import functools
import math

import numpy as np
import torch

import cond_attn as C
import cond_gemm as CG
import exact_rowk as xr
from exact_rowk import BF, EPS_ATTN, K  # noqa: F401  (EPS_ATTN re-exported)

FAMS = C.families_of("tiny")
NF = len(FAMS)
FAM_ID = {f: C.FAMILIES.index(f) for f in FAMS}
SCALE = 0.125
SCALE_LOG2 = SCALE * math.log2(math.e)                                            # fp64: the definition
SCALE_LOG2_F32 = float(np.float32(SCALE) * np.float32(1.4426950408889634))        # what the host hands the kernel
HEADS, D = 8, 64
K_CONST, AMP, SPREAD_Q, SW = 5.5, 7.5, 2.0, 3.75                                  # SW (a + b) = AMP
Q_NOISE = 1.0                                                                     # q = Q_NOISE (e[a] - e[b]) on the noise features
STRUCT_MINUS = 0.18                                                               # 2 p (1 - p) = 0.3 of the noise features non-zero
PEAK_DROP = 25.0                                                                  # peaked rows: every other key at least this far down

# code bits of a row (indices into CODE_POS)
QC, QW1, QW2, QW3 = (0, 1), (2, 3), (4, 5), (6, 7)
QP = ((8, 9), (10, 11), (12, 13))
QN = tuple(range(14, 54))
KL = tuple(range(54, 70))                                                         # four levels x (4, 2, 1, 1/2)
KP = ((70, 71), (72, 73), (74, 75))
KN = tuple(range(76, 132))
NCODE = 132
CODE_POS = np.random.RandomState(7).permutation(K)[:NCODE]
LEVEL_W = (4.0, 2.0, 1.0, 0.5)
ON, OFF, NEG = (1, 1), (1, -1), (-1, -1)
assert 2 * SW == AMP and len(KN) + KN[0] == NCODE and sum(LEVEL_W) == AMP


def blocks_of(h):
    """Feature positions of head h -> dict: const [8], wide_a [8], wide_b [8], peaks [3][4], noise [28]."""
    f = [int(v) for v in np.random.RandomState(100 + h).permutation(D)]
    return dict(const=f[0:8], wide_a=f[8:16], wide_b=f[16:24], peaks=[f[24 + 4 * c:28 + 4 * c] for c in range(3)], noise=f[36:64])


def peaks_of(L):
    return (0, L // 2, L - 1)


def slots_of(L):
    """Key slots a query's tile row holds: the cell of the narrow kernel, the two tiles of the wide one."""
    return 32 if L > 16 else 16 if L > 8 else 1 << (L - 1).bit_length()


def groups_per_tile(L):
    return 1 if L > 8 else 16 // slots_of(L)


def patterns(M, rng, codes):
    """e [M, 512] int64 (+-1, sum 0) holding ``codes`` [M, NCODE] at CODE_POS (exact_rowk.patterns for more code positions)."""
    e = np.empty((M, K), np.int64)
    free = np.setdiff1d(np.arange(K), CODE_POS)
    plus = 256 - (codes == 1).sum(1)
    rank = rng.random((M, len(free))).argsort(1).argsort(1)
    e[:, free] = np.where(rank < plus[:, None], 1, -1)
    e[:, CODE_POS] = codes
    assert (e.sum(1) == 0).all() and ((e * e).sum(1) == K).all()
    return torch.from_numpy(e)


def weights(rng):
    """-> (Wg [1536, 512], c [1536]) fp64: the packed q | k | v Linear after the fold, on the grid of the module docstring."""
    wg = torch.zeros(3 * K, K, dtype=torch.float64)
    c = torch.zeros(3 * K, dtype=torch.float64)
    pos = lambda bits: [int(CODE_POS[b]) for b in bits]
    for h in range(HEADS):
        blk = blocks_of(h)
        q0, k0 = D * h, K + D * h
        for f in blk["const"]:
            wg[q0 + f, pos(QC)] = SW
            c[k0 + f] = K_CONST
        for f in blk["wide_a"]:
            wg[q0 + f, pos(QW1)] = SW
            wg[q0 + f, pos(QW2)] = SPREAD_Q / 2
            wg[k0 + f, pos(KL[4 * (h % 4):4 * (h % 4) + 4])] = torch.tensor(LEVEL_W, dtype=torch.float64)
        for f in blk["wide_b"]:
            wg[q0 + f, pos(QW3)] = SW
            lv = (h + 1) % 4
            wg[k0 + f, pos(KL[4 * lv:4 * lv + 4])] = torch.tensor(LEVEL_W, dtype=torch.float64)
        for pk in range(3):
            for f in blk["peaks"][pk]:
                wg[q0 + f, pos(QP[pk])] = SW
                wg[k0 + f, pos(KP[pk])] = SW
        for f in blk["noise"]:
            a, b = rng.choice(len(QN), 2, replace=False)
            wg[q0 + f, CODE_POS[QN[a]]], wg[q0 + f, CODE_POS[QN[b]]] = Q_NOISE, -Q_NOISE
            a, b = rng.choice(len(KN), 2, replace=False)
            wg[k0 + f, CODE_POS[KN[a]]], wg[k0 + f, CODE_POS[KN[b]]] = 1.0, 0.5
    wg[2 * K:] = xr.thin(K, rng, 3).double()
    sign = torch.from_numpy(rng.choice([-1.0, 1.0], (HEADS, D)))
    sign[:, :D // 2] = 1.0
    c[2 * K:] = 4.0 * sign.reshape(-1)
    return wg, c


def codes_of(M, rows, rng):
    """-> (codes [M, NCODE] +-1, fam [groups, L] (index into cond_attn.FAMILIES), peak [groups, L])."""
    G, L = rows.shape
    g, i = np.arange(G)[:, None], np.arange(L)[None, :]
    fam_local = (i + g) % NF
    peak = ((i + g) // NF + g) % 3
    fam = np.array([FAM_ID[f] for f in FAMS])[fam_local]
    codes = rng.choice([-1, 1], (M, NCODE))
    for bits in (QC, QW1, QW2, QW3, *QP, *KP):                                    # rows of no group: every switch off
        codes[:, list(bits)] = OFF
    cg = rng.choice([-1, 1], (G, L, NCODE))
    is_ = lambda name: (fam == FAM_ID[name])[..., None]

    def pair(bits, pos_on, neg_on=None):
        val = np.where(pos_on, ON, OFF)
        cg[..., list(bits)] = val if neg_on is None else np.where(neg_on, NEG, val)

    pair(QC, is_("shift-high"), is_("shift-low"))
    pair(QW1, is_("wide") | is_("large"))
    pair(QW2, is_("shift-low") | is_("shift-high"))
    pair(QW3, is_("large"))
    for pk in range(3):
        pair(QP[pk], is_("peaked") & (peak == pk)[..., None])
        pair(KP[pk], np.broadcast_to(i == peaks_of(L)[pk], (G, L))[..., None])
    pool = cg[..., list(QN)]
    structured = ~(is_("friendly") | is_("flat"))
    pool = np.where(is_("flat"), 1, np.where(structured, np.where(rng.random(pool.shape) < STRUCT_MINUS, -1, 1), pool))
    cg[..., list(QN)] = pool
    cg[:, 0, list(KL)] = 1
    if L > 1:
        cg[:, 1, list(KL)] = -1
    codes[rows.reshape(-1)] = cg.reshape(-1, NCODE)
    return codes, torch.from_numpy(fam), torch.from_numpy(peak)


def per_head(t, rows):
    """[M, 512] -> [groups * 8, L, 64] over ``rows`` [groups, L]."""
    G, L = rows.shape
    return t[rows].view(G, L, HEADS, D).transpose(1, 2).reshape(G * HEADS, L, D)


def per_row(t, G):
    """[groups * 8, L, 64] -> [groups * L, 512] (the order of rows.reshape(-1))."""
    L = t.shape[1]
    return t.view(G, HEADS, L, D).transpose(1, 2).reshape(G * L, HEADS * D)


def seed_of(geo, M):
    return C.seed_of("rowattn-" + "-".join(str(v) for v in (*geo, M)))


@functools.lru_cache(maxsize=3)
def data(L, n_outer, n_inner, outer_stride, seq_stride, M):
    """The data of a geometry on the CPU (cached: treat as read-only) -> dict: x, the un-folded packed Linear (w [1536, 512], b,
    gamma, beta), wg, c, e, mu, d, t = e . Wg^T, rows [groups, L], the designed q, k, v [M, 512] fp64, fam, peak [groups, L], and the
    reference: o64, A [groups * 8, L, 64], fam8 [groups * 8, L], s_abs, eps."""
    rng = np.random.RandomState(seed_of((L, n_outer, n_inner, outer_stride, seq_stride), M))
    rows = xr.group_rows(L, n_outer, n_inner, outer_stride, seq_stride)
    G = rows.shape[0]
    assert rows.max() < M and len(torch.unique(rows)) == rows.numel()
    codes, fam, peak = codes_of(M, rows.numpy(), rng)
    e = patterns(M, rng, codes)
    x, mu, d = xr.rows_of(e, rng)
    wg, c = weights(rng)
    w, b, gamma, beta = xr.fold(wg, c, rng, True)
    t = e.double() @ wg.T
    qkv = t + c
    q, k, v = qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:]
    qh, kh, vh = (per_head(z, rows) for z in (q, k, v))
    o64, A = C.reference64(qh * SCALE_LOG2, kh, vh)
    sabs = C.s_abs(qh * SCALE_LOG2, kh)
    fam8 = fam[:, None, :].expand(G, HEADS, L).reshape(G * HEADS, L)
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, wg=wg, c=c, e=e, mu=mu, d=d, t=t, rows=rows, q=q, k=k, v=v, fam=fam, peak=peak,
                fam8=fam8, L=L, M=M, o64=o64, A=A, s_abs=sabs, eps=C.eps_of(L, D, sabs, tiny=True))


def case_data(c):
    return data(*xr.geometry(c), c["M"])


def pack(ops, dat, dev):
    """ops.pack_rowgemm512 of the un-folded q | k | v Linear; its fold must be the exact one."""
    pk = ops.pack_rowgemm512(dat["w"].to(dev), dat["b"].to(dev), dat["gamma"].to(dev), dat["beta"].to(dev))
    assert torch.equal(pk["w"].cpu().double(), dat["wg"]) and torch.equal(pk["colsum"].cpu().double(), dat["wg"].sum(1))
    assert torch.equal(pk["cvec"].cpu().double(), dat["c"])
    return pk


def emulate(dat, ulp, fma):
    """exact_rowk.emulate_fold over the q | k | v columns of the rows of the groups -> bf16 [groups * L, 1536]."""
    r = dat["rows"].reshape(-1)
    return xr.emulate_fold(dict(d=dat["d"][r], t=dat["t"][r], c=dat["c"], gelu=False, r=None), ulp, fma)


# ------------------------------------------------------------------------------------------------------------ restatement
FAULTS = ("p_trunc", "o_trunc", "drop_last", "leak_next", "leak_empty")


def has_next(dat):
    """[groups] bool: the group has a successor in its tile (narrow kernel, more than one group per tile)."""
    G, gpt = dat["rows"].shape[0], groups_per_tile(dat["L"])
    g = torch.arange(G)
    return (g % gpt != gpt - 1) & (g + 1 < G)


def has_empty(dat):
    return dat["L"] < slots_of(dat["L"])


def restate(dat, fault=None):
    """The restatement of the module docstring on the designed q, k, v -> bf16 [groups * 8, L, 64]."""
    assert fault is None or fault in FAULTS
    rows, L = dat["rows"], dat["L"]
    G = rows.shape[0]
    q, k, v = (per_head(dat[n], rows).float() for n in "qkv")
    ck, cv = (dat["c"][a:a + K].view(1, HEADS, 1, D).expand(G, HEADS, 1, D).reshape(G * HEADS, 1, D).float() for a in (K, 2 * K))
    nxt = torch.cat([rows[1:, 0], rows[:1, 0]])                                    # first row of the next group
    kn, vn = (dat[n][nxt].view(G, HEADS, 1, D).reshape(G * HEADS, 1, D).float() for n in "kv")
    kk, vv = torch.cat([k, kn, ck], 1), torch.cat([v, vn, cv], 1)
    s = q @ kk.transpose(1, 2)                                                     # [G * 8, L, L + 2], exact
    leak_n = (has_next(dat) if fault == "leak_next" else torch.zeros(G, dtype=torch.bool))[:, None].expand(G, HEADS).reshape(-1)
    s[..., L] = torch.where(leak_n[:, None], s[..., L], -math.inf)
    if not (fault == "leak_empty" and has_empty(dat)):
        s[..., L + 1] = -math.inf
    if fault == "drop_last":
        s[..., L - 1] = -math.inf
    p = torch.exp2((s - s.amax(-1, keepdim=True)) * torch.tensor(SCALE_LOG2_F32, dtype=torch.float32))
    pb = C._trunc_bf16(p) if fault == "p_trunc" else p.to(BF).float()
    o = (pb @ vv) * (1.0 / p.sum(-1, keepdim=True))
    if fault == "o_trunc":
        o = C._trunc_bf16(o)
    return o.to(BF)


def exact_mask(dat):
    """Bar (d): [groups * 8, L] bool, the query rows whose output a correct kernel gives as bf16(o64) bit for bit."""
    L, fam = dat["L"], dat["fam8"]
    if L == 1:
        return torch.ones_like(fam, dtype=torch.bool)
    m = fam == FAM_ID["peaked"]
    if L & (L - 1) == 0:
        m = m | (fam == FAM_ID["flat"])
    return m


def assert_exact_rows(name, got, dat, plan=None):
    """Bar (d) on ``got`` bf16 [groups * 8, L, 64]."""
    m = exact_mask(dat)
    ref = dat["o64"].to(BF)
    bad = xr.bad_elements(got[m], ref.to(got.device)[m])
    assert not bool(bad.any()), f"{name} [plan {plan}] bar (d): {xr.describe(bad, got[m], ref.to(got.device)[m])}"


def check(name, got, dat, restated=None, plan=None, out=print):
    """Bars (a), (b), (c: finite) and (d) on ``got`` bf16 [groups * 8, L, 64] -> cond_attn.check's figures."""
    restated = restate(dat) if restated is None else restated
    dev = got.device
    fig = C.check(name, got, dat["o64"].to(dev), dat["A"].to(dev), restated, dat["fam8"], FAMS, dat["eps"], plan=plan, out=out)
    out(f"{name} | {int(xr.bad_elements(got, restated.to(dev)).sum())} of {got.numel()} elements differ from the restatement (a record)")
    assert_exact_rows(name, got, dat, plan)
    return fig


# ------------------------------------------------------------------------------------------------------------ chain
def chain_weights():
    gen = torch.Generator().manual_seed(C.seed_of("rowattn-out-projection"))
    wo = (torch.randn(K, K, generator=gen) / math.sqrt(K)).to(BF)
    bo = (torch.randn(K, generator=gen) * 0.2).to(BF).float()
    return wo, bo


@functools.lru_cache(maxsize=2)
def chain_data(L, n_outer, n_inner, outer_stride, seq_stride, M):
    """``data`` plus wo, bo, y64 and bar [groups * L, 512] (the chain bar of the module docstring, absolute)."""
    dat = dict(data(L, n_outer, n_inner, outer_stride, seq_stride, M))
    wo, bo = chain_weights()
    G = dat["rows"].shape[0]
    o, A = per_row(dat["o64"], G), per_row(dat["A"], G)
    xg = dat["x"].double()[dat["rows"].reshape(-1)]
    wd, wa = wo.double().T, wo.double().abs().T
    y64 = xg + bo.double() + o @ wd
    S = o.abs() @ wa + bo.double().abs() + xg.abs()
    ulp = CG._ulp(y64)
    bar = (1 + dat["eps"]) * C.UNIT * ((A + o.abs()) @ wa) + (0.5 + CG.eps_of(S, ulp, K, ops=2)) * ulp
    dat.update(wo=wo, bo=bo, y64=y64, bar=bar, ulp=ulp)
    return dat


def chain_case_data(c):
    return chain_data(*xr.geometry(c), c["M"])


def chain_restate(dat, a=None):
    """The restated ``a`` (bf16 [groups * 8, L, 64]), an fp32 out-projection accumulated in 32-blocks, + bo, + x, one rounding."""
    G = dat["rows"].shape[0]
    a = per_row(restate(dat) if a is None else a, G).float()
    wt = dat["wo"].float().T
    acc = torch.zeros(a.shape[0], K)
    for k0 in range(0, K, 32):
        acc = acc + a[:, k0:k0 + 32] @ wt[k0:k0 + 32]
    return ((acc + dat["bo"]) + dat["x"].float()[dat["rows"].reshape(-1)]).to(BF)


def chain_check(name, got, dat, plan=None, out=print):
    """The chain bar on ``got`` bf16 [groups * L, 512] -> (worst |got - y64| / bar, the median error and the median bar in ulps of y64)."""
    g = got.double().cpu()
    err = (g - dat["y64"]).abs()
    ratio = torch.nan_to_num(err / dat["bar"], nan=math.inf)
    fig = (float(ratio.max()), float(torch.nan_to_num(err / dat["ulp"], nan=math.inf).median()), float((dat["bar"] / dat["ulp"]).median()))
    out(f"{name} | chain bar: worst |got - y64| / bar {fig[0]:.3f}, median error {fig[1]:.2f} ulp, median bar {fig[2]:.1f} ulp")
    bad = ratio > 1
    assert not bool(bad.any()), (f"{name} [plan {plan}] chain bar: {int(bad.sum())} of {bad.numel()} elements outside; first (group row, "
                                 f"column) {tuple(int(v) for v in bad.nonzero()[0])}, worst ratio {fig[0]:.3f}")
    return fig


# ------------------------------------------------------------------------------------------------------------ the GPU matrix
def _c(geom, pad=128, tp0=None, multi=False):
    c = dict(geom, pad=pad, tp0=tp0, multi=multi)
    c["name"] = f"L{c['L']}-{c['geom']}" + ("-multi-unit" if multi else "") + ("" if tp0 is None else f"-tp{tp0}")
    return c


RAGGED17 = xr._geom("ragged+3", 17, 2, 101, 17 * 101, 101, extra=3)
NARROW_CASES = [
    _c(xr.multi_id(1, 1500)),                          # P = 1, 16 groups per tile, the last tile holds 12
    _c(xr.multi_id(2, 1111), pad=256),                 # P = 2, 8 per tile
    _c(xr.multi_id(3, 555)),                           # 4-slot cells, one empty slot
    _c(xr.temporal(4), pad=256),
    _c(xr.temporal(8, n_inner=55, n_outer=3)),         # 165 groups, two per tile
    _c(xr.temporal(13), pad=256),                      # 3 empty slots, 2 outer blocks
    _c(xr.trailing(16, n_outer=3)),                    # 5 rows of no group
    _c(xr.multi_id(3, 2251), pad=256, multi=True),     # 563 tiles: 288 (row block, head) units on 256 workgroups
]
WIDE_CASES = [
    _c(RAGGED17),
    _c(xr.temporal(25, n_inner=45), pad=256),
    _c(xr._geom("one-outer", 32, 1, 77, 0, 77)),
    _c(xr.multi_id(17, 290), pad=256, multi=True),     # 580 tiles: 296 units
]
GROUP_ATTN_CASES = NARROW_CASES + WIDE_CASES
ATTN_OUT_CASES = [
    _c(xr.multi_id(1, 1500), tp0=0), _c(xr.multi_id(2, 1111), tp0=1, pad=256), _c(xr.multi_id(3, 555), tp0=6),
    _c(xr.temporal(13), tp0=0, pad=256), _c(xr.trailing(16, n_outer=3), tp0=6),
    _c(xr.temporal(13), tp0=1),                        # 338 tiles on 256 workgroups: two passes
]
RAGGED13 = xr._geom("ragged+3", 13, 2, 101, 13 * 101, 101, extra=3)
NO_GROUP_CASES = [_c(xr.trailing(16, n_outer=3)), _c(RAGGED17, pad=256)]                 # the plain kernel
NO_GROUP_OUT_CASES = [_c(xr.trailing(16, n_outer=3), tp0=0, pad=256), _c(RAGGED13, tp0=0)]  # the chain (L <= 16)


def expected_plan(c):
    """What router_group_attn_plan must answer for the case (without "blocks")."""
    L, groups = c["L"], c["n_outer"] * c["n_inner"]
    gpt = groups_per_tile(L)
    return dict(P=min(slots_of(L), 16), G=16 // min(slots_of(L), 16), wide=L > 16, tiles=2 * groups if L > 16 else -(-groups // gpt))


def expected_chain_plan(c):
    """(tiles, tp0, passes) of router_group_attn_out_plan: rowchain.hip's auto_tp0 / grid_for / Passes restated (8 waves)."""
    tiles = -(-c["n_outer"] * c["n_inner"] // groups_per_tile(c["L"]))
    tp0 = c["tp0"] or min(max(-(-tiles // 256), 1), 8)
    grid = min(-(-tiles // tp0), 256)
    base, tpw, passes = 0, tp0, 1
    while base + grid * tpw < tiles:
        base += grid * tpw
        tpw = min(-(-(tiles - base) // grid), 8)
        passes += 1
    return tiles, tp0, passes
