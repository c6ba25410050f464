"""Exact-data checking of csrc/norm.hip (a plain helper module: no tests, no fixtures; the sibling of ``exact_gemm.py``,
``exact_attn.py`` and ``exact_rowk.py``, whose ``GuardedOut`` / ``bad_elements`` / ``patterns`` it reuses): layernorm_kernel<VEC, NV>
with its fp8 and MX outputs, layernorm_adaln_rows_kernel<NV, MOD> and qknorm_rope_kernel<STATS>.  The stand-alone q/k-norm kernel
is the reference of every fused home of qknorm_math.h, so comparing those with it cannot see a fault in it; a relative-Frobenius
bar of 1e-3 does not see a variance divided by D - 1, a dropped eps or an eps a hundred times too large (test_norm_exact_cpu.py
recomputes those scores).  Here every case has data for which a correct kernel's answer is a function of the data alone, the
check is bit equality with an fp64 reference rounded once, and a failure names the element, its row, its wave and its lane.
All data is made on the CPU from a seed (the CPU tests check the same tensors).

LAYERNORM (``ln_data``), D in {512, 768, 1024, 2048, 3072}.  Row m is x = mu + d e: mu an integer in [-4, 4], d in {1, 2, 4},
e an integer row with sum 0 and sum of squares exactly D -- D / 2 entries +1 and D / 2 entries -1 in a seeded order, or (every
other row of the pool, where the form has an additive term) D / 16 x +2, D / 16 x -2, D / 4 x +1, D / 4 x -1 and 3 D / 8 zeros:
``exact_rowk.patterns`` scaled to D.  |x| <= 12 is exact in bf16; sum x = D mu and sum (x - mu)^2 = D d^2 are sums of small
integers, exact in fp32 in any order; fl(fl(D mu) fl(1 / D)) == mu and fl(fl(D d^2) fl(1 / D)) == d^2 for all five widths, the
two whose 1 / D is no power of two included (``assert_mean_var_identities``).  So mean and variance are exact, x - mean = d e,
and LN(x) = e (d rstd).  The rows of a case come from a pool of at most 64 pattern rows (row m takes pool row (m + 3 (m / P)) mod
P: neighbours always differ) with mu and d of their own, so the per-element conditions of a 25-million-element case are
exhaustive on its distinct (pool row, d, parameter set) triples.
eps: the mixed-d cases use eps = 0 (true rstd 1 / d, LN(x) = e); the eps cases use d = 1 on every row and eps = 3: var + eps = 4,
the true rstd is 1 / 2 and LN(x) = e / 2 -- a kernel that drops, mis-scales or swaps eps is wrong by a factor, not by 1e-5.
Parameters: w a power of two per column (1/2, 1, 2); 1 + scale a power of two per column (scale in {-1/2, 0, 1, 3}); b an even
integer; shift an integer.  With A = w (1 + scale), B = b (1 + scale) + shift and k = d rstd (1 or 1/2) the true
y = e k A + B; B has alternating sign per column and magnitude  ceil(2 k |A|) + 2 .. + 8,  so |e k A| <= 2 k |A| never cancels
it: y != 0 on every element, y is a multiple of u = k |A| >= 1/8 with |y| / u <= 4 + 9 / u' < 2^8: at most 8 significant bits, a
bf16 number whose nearest rounding boundary is 2^-9 |y| away.  (Forms without an additive term -- no parameters, w alone -- use
the +-1 patterns only: y = e k A.)  The device's rsqrtf may be an ulp or two off and the two kernels' expressions differ (the
generic branch o w + b then (1 + sc) + sh, contracted or not; the single fma of the A / B form): both move the result by a few
2^-23 relative, which y != 0 makes harmless.  ``emulate_ln`` evaluates the expressions in fp32 with rstd up to two ulps either
side for every element and must give the fp64 result's bf16.  The modulation sets (batch entry z, side of the split) are
drawn so that y under any two of them differs on every element for every pattern value: a wrong set changes every element.

VARIANCE-SENSITIVE ROWS (``form = "sens"``, every width).  A relative fault of 1 / (2 D) in rstd -- the variance divided by
D - 1 -- cannot move a value of 8 significant bits across a bf16 rounding boundary 2^-9 |y| away: the grid that makes the answer
independent of the last bit of rsqrtf makes it independent of that fault too.  These rows put values NEAR a boundary instead:
modulation alone, scale = 0, shift = +-(2^-8 + delta) with alternating sign per column, delta = ``sens_delta(D)`` the power of two
below 1 / (4 D), on +-1 patterns at eps = 0.  Where e and the shift agree in sign |y| = 1 + 2^-8 + delta: exact in fp32, delta
above the boundary 1 + 2^-8 of the bf16 numbers 1 and 1 + 2^-7, so it rounds up; the kernels' noise (rstd two ulps off: 2^-22)
is at least 2^-14 / 2^-22 = 256 times smaller than delta, while 1 / (2 (D - 1)) > 2 delta takes the faulty value below the
boundary, which rounds to 1.  Where they disagree |y| = 1 - 2^-8 - delta, 2^-9 - delta from the nearest boundary.

FP8 / MX OUTPUT (``form = "quant"``, D = 3072, +-1 patterns): per set A = a 2^j and B = beta 2^j with a in {1, 2}, j in {0, 1} and
beta an integer with a < |beta| <= 7 - a, so y / 2^j is an integer of magnitude 1 .. 7.  Column 0 has a = 1, beta = +6 and every
pattern row has e[0] = +1 (a row with -1 there is negated; its sum stays 0): every row's maximum is 7 2^j, 448 / amax a power of
two and every scaled value an e4m3 number.  The first column of every 32-block has a = 1 and |beta| in {5, 6}: the block's
maximum is in [4, 8) 2^j, its MX scale 2^j (e2m3) or 2^(j - 6) (e4m3) and every scaled value an integer <= 7 (times 64): exact
in both element formats.  Expected bytes: the quantisers' DEFINITION (``quant_rows_fp8_ref`` here -- moved from
test_fp8_gpu.py -- and test_mx_cpu.quant_mx_ref) applied to the fp64 LayerNorm rounded to bf16, not to ops.layernorm.

Q/K-NORM + ROPE (``qk_data``).  A head row is mu + d e over 64 values, e = +-1 with sum 0 (1 / 64 is a power of two: mean and
variance exact).  w a power of two (1/2, 1, 2), b an integer of magnitude 3 .. 6 with alternating sign: n = e k w + b is a
multiple of 1/4 with 1 <= |n| <= 8.  The rotary tables are inputs: entries from {0, +-1/2, +-1, +-2}, independent per element
(cos[2i] != cos[2i+1] as a rule) and per token row, so any wrong row or element index changes the answer.  Every
n[e] c[e] - n[e+1] s[e] and n[e+1] c[e+1] + n[e] s[e+1] is a multiple of 1/8 of magnitude <= 32; a table entry whose output would be 0
for some (tensor, batch, head) is drawn again.  Every output is non-zero with at most 8 significant bits (asserted), times
k_scale in {1, 1/4} (an exponent shift).  ``emulate_qkn`` restates qknorm_math.h in fp32 with rstd +- 2 ulps (sequential sum of 8,
the tree 1, 2, 4, the explicit fmas).  stats: the squared norm of a finished row is a sum of 64 squares of multiples of 1/32
below 2^12 (1/8 below 2^16 for q): exact in fp32 in any order, so a table entry must EQUAL the fp64 maximum over the pairs whose
workgroup index maps to its slot (``qk_stats_table``).

Which kernel a case runs is asserted through ops.layernorm_plan / ops.qknorm_rope_plan before the launch; which waves of the rows
kernel cross the split or a batch boundary or are clipped (``rows_waves``), and which waves of the q/k kernel straddle a token
row, a batch entry or the q -> k boundary (``qk_waves``), are modelled here from the plan's rows_per_wave / pair enumeration.
"""
import numpy as np
import torch

import exact_rowk as xr
from exact_gemm import BF, POISON, SENTINEL, GuardedOut, assert_exact, bad_elements, describe, pow2, strided  # noqa: F401  (re-exported)
from test_mx_cpu import quant_mx_ref

WIDTHS = (512, 768, 1024, 2048, 3072)
VEC_NV = {512: (8, 1), 768: (4, 3), 1024: (8, 2), 2048: (8, 4), 3072: (8, 6)}
FORMS = ("none", "w", "wb", "mod", "wbmod")
EPS3 = 3.0
POOL = 64


def f32(v):
    """Round fp64 values to fp32 (kept in fp64)."""
    return v.float().double()


def fma32(a, b, c):
    """fmaf on fp32 values held in fp64: the product of two 24-bit significands is exact in fp64."""
    return f32(a * b + c)


def sig_bits(v):
    """Significant bits of each non-zero dyadic fp64 value."""
    m, _ = torch.frexp(v.abs())
    n = (m * 2.0 ** 53).long()
    low = n & -n                                                      # lowest set bit
    return 53 - torch.log2(low.double()).long()


def move_ulps(r, ulps):
    """fp32 tensor moved by ``ulps`` ulps (positive: up)."""
    r = r.float()
    for _ in range(abs(ulps)):
        r = torch.nextafter(r, torch.full_like(r, float("inf") if ulps > 0 else 0.0))
    return r


def quant_rows_fp8_ref(x):
    """include/bya.h, bya_quantize_rows_fp8, on the CPU: bf16 [.., K] -> (e4m3 bytes, fp32 row scales [..])."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True)
    # tensor / tensor: the correctly rounded quotient (torch evaluates `scalar / tensor` as reciprocal * scalar, which is
    # one ulp off for a third of the rows and flips 0.13 % of the bytes at exact ties)
    c448 = torch.full_like(amax, 448.0)
    inv = torch.where(amax > 0, c448 / amax, torch.zeros_like(amax))
    scale = torch.where(amax > 0, amax / c448, torch.ones_like(amax))
    q = (xf * inv).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale.squeeze(-1)


# ------------------------------------------------------------------------------------------------------------ LayerNorm data
def assert_mean_var_identities():
    """fl(fl(D mu) fl(1 / D)) == mu and fl(fl(D d^2) fl(1 / D)) == d^2 in fp32, for every width, |mu| <= 8, d in {1, 2, 4}."""
    for D in WIDTHS + (64,):
        inv = np.float32(1.0) / np.float32(D)
        for mu in range(-8, 9):
            assert np.float32(np.float32(D * mu) * inv) == np.float32(mu), (D, mu)
        for d in (1, 2, 4):
            assert np.float32(np.float32(D * d * d) * inv) == np.float32(d * d), (D, d)


def ln_patterns(P, D, rng, rich):
    """e [P, D] int64: rows with sum 0 and sum of squares D (``exact_rowk.patterns`` scaled to D)."""
    if D == xr.K:
        return xr.patterns(P, rng, rich=rich)
    rank = rng.random((P, D)).argsort(1).argsort(1)
    e = np.where(rank < D // 2, 1, -1).astype(np.int64)
    if rich:
        multiset = np.array([2] * (D // 16) + [-2] * (D // 16) + [1] * (D // 4) + [-1] * (D // 4) + [0] * (3 * D // 8))
        assert len(multiset) == D
        odd = np.arange(1, P, 2)
        e[odd] = multiset[rng.random((len(odd), D)).argsort(1)]
    assert (e.sum(1) == 0).all() and ((e * e).sum(1) == D).all()
    return torch.from_numpy(e)


def sens_delta(D):
    """2^-n with 2^-n < 1 / (4 D): the offset of the variance-sensitive values from a bf16 rounding boundary."""
    return 2.0 ** -(int(np.ceil(np.log2(2 * D))) + 1)


def boundary_distance(y):
    """Relative distance of each fp64 value to the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 numbers)."""
    _, ex = torch.frexp(y.abs())
    ulp = torch.ldexp(torch.ones_like(y), ex - 8)                    # |y| in [2^(ex-1), 2^ex): 8 significant bits
    frac = torch.remainder(y.abs() / ulp, 1.0)
    return (frac - 0.5).abs() * ulp / y.abs()


def _signs(D):
    return torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0).double()


def _draw_sets(nsets, D, k, draw):
    """Per-column (A, B) [nsets, D] of ``nsets`` parameter sets by ``draw(mask) -> (A, B) [nsets, mask.sum()]``, drawn again for
    the columns where two sets give the same y = e k A + B for some pattern value e in -2 .. 2."""
    A, B = draw(torch.ones(D, dtype=torch.bool))
    ev = torch.arange(-2, 3).double()[:, None, None] * k
    for _ in range(200):
        y = ev * A[None] + B[None]                                   # [5, nsets, D]
        same = torch.zeros(D, dtype=torch.bool)
        for s in range(nsets):
            for t in range(s + 1, nsets):
                same |= (y[:, s] == y[:, t]).any(0)
        if not bool(same.any()):
            return A, B
        A[:, same], B[:, same] = draw(same)
    raise AssertionError("parameter sets that differ everywhere were not found")


def ln_data(c):
    """The tensors of LayerNorm case ``c`` (``LN_CASES``) -> dict: x [B, M, D] bf16; w, b [D] bf16 or None; sh, sc [B, 2, D] bf16
    or None (set (z, 0) for rows < split, (z, 1) for the others; mod_batch_stride = 2 D); the pool e [P, D], idx / mu / d per
    row [B * M]; the closed form's A, Bc [B, 2, D] fp64 and k."""
    D, M, Bn, form, eps = c["D"], c["rows"], c["batch"], c["form"], c["eps"]
    rng = np.random.RandomState(seed_of(c))
    total = M * Bn
    P = min(total, POOL)
    additive = form in ("wb", "mod", "wbmod")
    e = ln_patterns(P, D, rng, rich=additive)
    if form == "quant":
        e = torch.where(e[:, :1] < 0, -e, e)                         # e[:, 0] = +1
    m = torch.arange(total)
    idx = (m + 3 * (m // P)) % P
    mu = torch.from_numpy(rng.randint(-4, 5, total))
    d = torch.ones(total, dtype=torch.int64) if eps else torch.from_numpy(rng.choice([1, 2, 4], total))
    k = 0.5 if eps else 1.0
    x = (mu[:, None].float() + d[:, None].float() * e.float()[idx]).to(BF).view(Bn, M, D)
    sign = _signs(D)
    pw = lambda n, vals: torch.from_numpy(rng.choice(vals, n)).double()
    w = b = sh = sc = None
    nsets = 2 * Bn
    if form == "quant":
        a = pw(D, [1.0, 2.0])
        first = torch.arange(D) % 32 == 0
        a[first] = 1.0
        wv = torch.where(a == 2, pw(D, [1.0, 2.0]), pw(D, [0.5, 1.0, 2.0]))
        j = torch.from_numpy(rng.permutation(np.arange(nsets) % 2)).double()[:, None]
        lo, hi = a + 1, 7 - a                                         # a < |beta| <= 7 - a
        beta = torch.stack([lo + torch.from_numpy(rng.randint(0, 100, D)).double() % (hi - lo + 1) for _ in range(nsets)])
        beta[:, first] = torch.from_numpy(rng.choice([5.0, 6.0], (nsets, int(first.sum()))))
        beta = beta * torch.from_numpy(rng.choice([-1.0, 1.0], (nsets, D)))
        beta[:, 0] = 6.0
        A, Bc = a[None] * 2.0 ** j, beta * 2.0 ** j
        bv = 2.0 * torch.from_numpy(rng.randint(-2, 3, D)).double()
        one_sc = A / wv
        w, b, sc, sh = wv, bv, one_sc - 1, Bc - bv * one_sc
    elif form == "sens":
        # modulation alone with scale = 0 and shift = +-(2^-8 + delta): y = e + shift (see the module docstring)
        sc = torch.zeros(nsets, D).double()
        sh = (sign * (2.0 ** -8 + sens_delta(D)))[None].repeat(nsets, 1)
        A, Bc = torch.ones(nsets, D).double(), sh.clone()
    else:
        wv = pw(D, [0.5, 1.0, 2.0]) if "w" in form else torch.ones(D).double()
        bv = 2.0 * torch.from_numpy(rng.randint(-2, 3, D)).double()

        if "mod" in form:
            def draw(mask):                                          # A = w (1 + scale), |B| = ceil(2 k |A|) + 2 .. 8
                n = int(mask.sum())
                A_ = wv[mask][None] * pw((nsets, n), [0.5, 1.0, 2.0, 4.0])
                return A_, sign[mask][None] * (torch.ceil(2 * k * A_) + torch.from_numpy(rng.randint(2, 9, (nsets, n))).double())

            A, Bc = _draw_sets(nsets, D, k, draw)
            one_sc = A / wv
            sc = one_sc - 1
            if form == "wbmod":
                w, b, sh = wv, bv, Bc - bv * one_sc
            else:
                sh = Bc
        else:
            A = wv[None].repeat(nsets, 1)
            if form == "wb":
                bv = sign * (torch.ceil(2 * k * wv) + torch.from_numpy(rng.randint(2, 9, D)).double())
                w, b, Bc = wv, bv, bv[None].repeat(nsets, 1)
            else:
                Bc = torch.zeros(nsets, D).double()
                w = wv if form == "w" else None
    tobf = lambda t: None if t is None else _exact_bf(t)
    out = dict(x=x, w=tobf(w), b=tobf(b), sh=None if sh is None else tobf(sh).view(Bn, 2, D), sc=None if sc is None else tobf(sc).view(Bn, 2, D),
               e=e, idx=idx, mu=mu, d=d, A=A.view(Bn, 2, D), Bc=Bc.view(Bn, 2, D), k=k, eps=float(eps))
    return out


def _exact_bf(t):
    r = t.to(BF)
    assert torch.equal(r.double(), t.double()), "a parameter is not a bf16 number"
    return r.contiguous()


def row_sets(c, dev="cpu"):
    """Set index 2 z + side of every row [B * M]."""
    z = torch.arange(c["batch"], device=dev).repeat_interleave(c["rows"])
    row = torch.arange(c["rows"], device=dev).repeat(c["batch"])
    return 2 * z + (row >= c["split"]).long()


def closed_form(c, dat, sets=None, rows=None):
    """y = e k A + B of rows ``rows`` (default: all) under parameter sets ``sets`` (default: their own) -> fp64 [n, D]."""
    rows = torch.arange(c["rows"] * c["batch"]) if rows is None else rows
    sets = row_sets(c)[rows] if sets is None else sets
    A, Bc = dat["A"].reshape(-1, c["D"]), dat["Bc"].reshape(-1, c["D"])
    return dat["e"].double()[dat["idx"][rows]] * dat["k"] * A[sets] + Bc[sets]


def distinct_rows(c, dat):
    """One row index per distinct (pool row, d, parameter set): the per-element conditions on these rows hold for every row."""
    key = torch.stack([dat["idx"], dat["d"], row_sets(c)], 1).numpy()
    _, first = np.unique(key, axis=0, return_index=True)
    return torch.from_numpy(np.sort(first))


def ln_reference64(x, eps, w=None, b=None, sh=None, sc=None, sets=None, var_div=None):
    """The LayerNorm's definition in fp64 on x [n, D] (any device): ((x - mean) / sqrt(var + eps) w + b) (1 + scale) + shift with
    row r's modulation vectors sh[sets[r]], sc[sets[r]] (sh, sc: [nsets, D]).  ``var_div``: the planted fault var / (D - 1)."""
    xd = x.double()
    D = xd.shape[-1]
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).sum(-1, keepdim=True) / (D if var_div is None else var_div)
    y = (xd - mean) / torch.sqrt(var + eps)
    if w is not None:
        y = y * w.double()
    if b is not None:
        y = y + b.double()
    if sh is not None:
        y = y * (1 + sc.double()[sets]) + sh.double()[sets]
    return y


def ln_reference_case(c, dat, dev="cpu", rows=None, **fault):
    """fp64 reference of case ``c`` -> [B, M, D] (or the rows ``rows`` -> [n, D]) on ``dev``."""
    D = c["D"]
    x = dat["x"].view(-1, D)
    sets = row_sets(c)
    if rows is not None:
        x, sets = x[rows], sets[rows]
    if fault.pop("side_only", False):
        sets = sets % 2                                              # the planted fault: the set keyed by the side alone
    eps = fault.pop("eps", dat["eps"])
    mv = lambda t: None if t is None else t.to(dev)
    sh, sc = (None if dat[n] is None else dat[n].view(-1, D).to(dev) for n in ("sh", "sc"))
    y = ln_reference64(x.to(dev), eps, mv(dat["w"]), mv(dat["b"]), sh, sc, sets.to(dev), **fault)
    return y if rows is not None else y.view(c["batch"], c["rows"], D)


def assert_ln_conditions(c, dat):
    """Every element of the case: x exact, y != 0, at most 8 significant bits, the fp64 LayerNorm rounds to the closed form, the
    kernels' fp32 expressions with rstd +- 2 ulps give its bf16 (``emulate_ln``); quantised cases: the fp8 / MX conditions."""
    D = c["D"]
    x = dat["x"].view(-1, D).double()
    assert float(x.abs().max()) <= 12 and torch.equal(x.sum(1), D * dat["mu"].double())
    assert torch.equal(((x - dat["mu"][:, None]) ** 2).sum(1), D * (dat["d"] ** 2).double())
    assert not c["eps"] or bool((dat["d"] == 1).all())
    rows = distinct_rows(c, dat)
    y = closed_form(c, dat, rows=rows)
    assert bool((y != 0).all()), "a true result is 0"
    want = y.to(BF)
    if c["form"] == "sens":
        # half the elements sit delta above a rounding boundary (|y| = 1 + 2^-8 + delta), the others far from one; the fp32 noise
        # of a few 2^-23 is far below delta, the fault var / (D - 1) moves e by 1 / (2 (D - 1)) > 2 delta
        dist = boundary_distance(y)
        near = y.abs() > 1
        assert float(dist.min()) >= 2.0 ** -16 and 0.4 < float(near.double().mean()) < 0.6
        assert bool((dist[near] < 1.0 / (4 * c["D"])).all()) and bool((dist[~near] > 2.0 ** -10).all())
    else:
        assert int(sig_bits(y).max()) <= 8, int(sig_bits(y).max())
        assert torch.equal(want.double(), y)
    ref = ln_reference_case(c, dat, rows=rows)
    assert float(((ref - y).abs() / y.abs()).max()) < 2.0 ** -40
    assert torch.equal(ref.to(BF), want)
    for ulps in (-2, -1, 0, 1, 2):
        for got in emulate_ln(c, dat, rows, ulps):
            bad = bad_elements(got, want)
            assert not bool(bad.any()), f"{c['name']} rstd {ulps:+d} ulps: {describe(bad, got, want)}"
    if c["form"] == "quant":
        yq = closed_form(c, dat)
        j = torch.log2(yq.abs().amax(1) / 7)
        assert torch.equal(j, j.round()), "a row's maximum is not 7 * 2^j"
        v = yq / (2.0 ** j)[:, None]
        assert torch.equal(v, v.round()) and float(v.abs().max()) == 7 and float(v.abs().min()) >= 1
        blk = v.abs().view(v.shape[0], -1, 32).amax(-1)
        assert float(blk.min()) >= 4
        s8 = v * 64
        assert torch.equal(s8.float().to(torch.float8_e4m3fn).double(), s8)           # e4m3 numbers after the row scale 448 / amax


def emulate_ln(c, dat, rows, ulps):
    """The kernels' expressions in fp32 on the rows ``rows``, rstd = the true one moved by ``ulps`` ulps -> list of bf16 [n, D]:
    the generic branch (o w + b, then (1 + sc) + sh; each contracted to an fma and not) and the single fma of the A / B form
    where a kernel evaluates it (w and b present)."""
    D = c["D"]
    sets = row_sets(c)[rows]
    cen = (dat["d"][rows, None] * dat["e"][dat["idx"][rows]]).double()                 # x - mean, exact
    var = (dat["d"][rows, None] ** 2).double()
    true_rstd = (1.0 / torch.sqrt(var + dat["eps"])).float()
    assert torch.equal(true_rstd.double() ** 2 * (var + dat["eps"]), torch.ones_like(var)), "the true rstd is not an fp32 number"
    o = f32(cen * move_ulps(true_rstd, ulps).double())
    w, b = (None if dat[n] is None else dat[n].double() for n in ("w", "b"))
    sh, sc = (None if dat[n] is None else dat[n].view(-1, D).double()[sets] for n in ("sh", "sc"))
    outs = []
    for fma in (True, False):
        t = o
        if w is not None:
            bb = b if b is not None else torch.zeros(D).double()
            t = fma32(t, w, bb) if fma else f32(f32(t * w) + bb)
        if sh is not None:
            one = f32(1.0 + sc)
            t = fma32(t, one, sh) if fma else f32(f32(t * one) + sh)
        outs.append(t.to(BF))
    if w is not None and b is not None:
        if sh is not None:
            one = f32(1.0 + sc)
            A, Bc = f32(w * one), fma32(b.expand_as(one), one, sh)
        else:
            A, Bc = w.expand_as(o), b.expand_as(o)
        outs.append(fma32(o, A, Bc).to(BF))
    return outs


def quant_expected(c, dat):
    """Bytes and scales of the fp8 / MX forms of case ``c`` from the quantisers' definitions on the fp64 LayerNorm rounded to bf16
    -> (codes uint8 [B, M, row bytes], scales [B, M] fp32 or [B, M, D / 32] uint8)."""
    y = ln_reference_case(c, dat).to(BF)
    if c["out"] == "fp8":
        return quant_rows_fp8_ref(y)
    return quant_mx_ref(y, c["out"])


# ------------------------------------------------------------------------------------------------------------ rows-kernel model
def rows_waves(rows_per_batch, batch, split, rpw):
    """layernorm_adaln_rows_kernel's ranges: per wave (r0, r1, crosses_split, crosses_batch, clipped) over the batch-major row
    enumeration; crosses_split: the side changes inside one batch entry; clipped: r0 + rpw > total."""
    total = rows_per_batch * batch
    out = []
    for gw in range((total + rpw - 1) // rpw):
        r0, r1 = gw * rpw, min(gw * rpw + rpw, total)
        zs = [r // rows_per_batch for r in range(r0, r1)]
        sides = [(r % rows_per_batch) >= split for r in range(r0, r1)]
        cs = any(zs[i] == zs[i + 1] and sides[i] != sides[i + 1] for i in range(len(zs) - 1))
        out.append((r0, r1, cs, zs[0] != zs[-1], gw * rpw + rpw > total))
    return out


def ln_events(c, plan):
    """What the rows kernel's waves of case ``c`` meet: a set of names."""
    if plan["kernel"] != "rows":
        return set()
    ev = set()
    for r0, r1, cs, cb, cl in rows_waves(c["rows"], c["batch"], c["split"], plan["rows_per_wave"]):
        sides = {(r % c["rows"]) >= c["split"] for r in range(r0, r1)}
        ev |= {"crosses_split"} if cs else set()
        ev |= {"crosses_batch"} if cb else set()
        ev |= {"crosses_batch_same_side"} if cb and len(sides) == 1 else set()
        ev |= {"clipped"} if cl else set()
    return ev


def describe_ln(c, plan, bad, got, ref):
    """Failure text: the first bad element with its batch entry, row, wave, lane and vector, and how many differ."""
    idx = bad.reshape(-1, c["D"]).nonzero()
    if idx.numel() == 0:
        return "no bad elements"
    r, col = int(idx[0, 0]), int(idx[0, 1])
    vec = plan["vec"]
    g, w = got.reshape(-1, c["D"]), ref.reshape(-1, c["D"])
    return (f"{idx.shape[0]} of {bad.numel()} elements differ; first: batch entry {r // c['rows']} row {r % c['rows']} column {col} "
            f"(wave {r // plan['rows_per_wave']}, lane {(col // vec) % 64}, vector {col // (64 * vec)}): got {float(g[r, col]):g}, "
            f"want {float(w[r, col]):g}; rows {int(idx[:, 0].min())}..{int(idx[:, 0].max())}")


def assert_ln_exact(c, plan, got, ref64, what=""):
    ref = ref64.to(BF)
    bad = bad_elements(got, ref)
    assert not bool(bad.any()), f"{c['name']} {what} [plan {plan}]: {describe_ln(c, plan, bad, got, ref)}"


# ------------------------------------------------------------------------------------------------------------ q/k-norm + RoPE
TABLE_VALUES = [0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0]


def qk_data(c):
    """The tensors of q/k case ``c`` (``QK_CASES``) -> dict: q, k [B, S, H * 64] bf16 inputs; qw, qb, kw, kb [64] bf16; cos, sin
    fp32 [S - text_rows, 64] or None; ref [2, B, S, H * 64] fp64 (q, k), n (before the rotation) and the pieces of ``emulate_qkn``."""
    Bn, S, H, T, eps = c["batch"], c["S"], c["heads"], c["text_rows"], c["eps"]
    rng = np.random.RandomState(seed_of(c))
    R = 2 * Bn * S * H
    rank = rng.random((R, 64)).argsort(1).argsort(1)
    e = torch.from_numpy(np.where(rank < 32, 1, -1)).view(2, Bn, S, H, 64)
    mu = torch.from_numpy(rng.randint(-4, 5, (2, Bn, S, H, 1)))
    d = torch.ones(2, Bn, S, H, 1, dtype=torch.int64) if eps else torch.from_numpy(rng.choice([1, 2, 4], (2, Bn, S, H, 1)))
    k = 0.5 if eps else 1.0
    x = mu + d * e
    w = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], (2, 64))).double()
    b = _signs(64)[None] * torch.from_numpy(rng.randint(3, 7, (2, 64))).double()
    n = e.double() * k * w[:, None, None, None] + b[:, None, None, None]                # [2, B, S, H, 64]
    ks = torch.tensor([1.0, c["k_scale"]]).double().view(2, 1, 1, 1, 1)
    cos = sin = None
    ref = n.clone()
    if T < S:
        N = S - T
        draw = lambda shape: torch.from_numpy(rng.choice(TABLE_VALUES, shape)).double()
        cos, sin = draw((N, 64)), draw((N, 64))
        nv = n[:, :, T:]                                                                    # [2, B, N, H, 64]
        rot = torch.stack([-nv[..., 1::2], nv[..., 0::2]], -1).flatten(-2)                  # rot[2i] = -n[2i+1], rot[2i+1] = n[2i]
        for _ in range(200):
            o = nv * cos[None, None, :, None] + rot * sin[None, None, :, None]
            zero = (o == 0).any(0).any(0).any(1)                                            # [N, 64]
            if not bool(zero.any()):
                break
            cnt = int(zero.sum())
            cos[zero], sin[zero] = draw(cnt), draw(cnt)
        else:
            raise AssertionError("rotary entries without a cancellation were not found")
        ref[:, :, T:] = o
    ref = ref * ks
    flat = lambda t: t.reshape(2, Bn, S, H * 64)
    xb = flat(x).to(BF)
    assert torch.equal(xb.double(), flat(x).double())
    return dict(q=xb[0].contiguous(), k=xb[1].contiguous(), qw=_exact_bf(w[0]), kw=_exact_bf(w[1]), qb=_exact_bf(b[0]), kb=_exact_bf(b[1]),
                cos=None if cos is None else cos.float().contiguous(), sin=None if sin is None else sin.float().contiguous(),
                ref=flat(ref), n=n, x=x, d=d, mu=mu, w=w, b=b, kk=k, eps=float(eps))


def qk_reference64(x, w, b, cos, sin, text_rows, eps, k_scale=1.0, **fault):
    """The definition in fp64: per-head LayerNorm(64) of x [B, S, H * 64], interleaved-pair RoPE on rows >= text_rows, * k_scale.
    Planted faults: ``var_div`` (variance divisor), ``cos_shift`` (cos[e] read for element e + 1)."""
    Bn, S, W = x.shape
    xd = x.double().view(Bn, S, W // 64, 64)
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).sum(-1, keepdim=True) / fault.get("var_div", 64)
    y = (xd - mean) / torch.sqrt(var + eps) * w.double() + b.double()
    if text_rows < S:
        c_, s_ = cos.double(), sin.double()
        if fault.get("cos_shift"):
            c_ = torch.roll(c_, 1, -1)
        v = y[:, text_rows:]
        rot = torch.stack([-v[..., 1::2], v[..., 0::2]], -1).flatten(-2)
        y = torch.cat([y[:, :text_rows], v * c_[None, :, None] + rot * s_[None, :, None]], 1)
    return (y * k_scale).reshape(Bn, S, W)


def qk_reference_case(c, dat, **fault):
    """-> (q_ref, k_ref) fp64 [B, S, H * 64] from the definition (not from the closed form)."""
    eps = fault.pop("eps", dat["eps"])
    q_scale = fault.pop("q_scale", 1.0)                               # the planted fault: k_scale applied to q
    args = (dat["cos"], dat["sin"], c["text_rows"], eps)
    return (qk_reference64(dat["q"], dat["qw"], dat["qb"], *args, q_scale, **fault),
            qk_reference64(dat["k"], dat["kw"], dat["kb"], *args, c["k_scale"], **fault))


def assert_qk_conditions(c, dat):
    ref = dat["ref"]
    assert bool((ref != 0).all()), "a true result is 0"
    assert int(sig_bits(ref).max()) <= 8
    assert torch.equal(ref.to(BF).double(), ref)
    q64, k64 = qk_reference_case(c, dat)
    for which, r64 in enumerate((q64, k64)):
        assert float(((r64 - ref[which]).abs() / ref[which].abs()).max()) < 2.0 ** -40
        assert torch.equal(r64.to(BF), ref[which].to(BF))
    T, S = c["text_rows"], c["S"]
    if 0 < S - T:
        cs, sn = dat["cos"], dat["sin"]
        assert float((cs[:, 0::2] != cs[:, 1::2]).float().mean()) > 0.5 and float((sn[:, 0::2] != sn[:, 1::2]).float().mean()) > 0.5
    want = ref.to(BF)
    for ulps in (-2, -1, 0, 1, 2):
        got = emulate_qkn(c, dat, ulps)
        bad = bad_elements(got, want)
        assert not bool(bad.any()), f"{c['name']} rstd {ulps:+d} ulps: {describe(bad, got, want)}"
    n2 = (ref ** 2).view(*ref.shape[:-1], -1, 64).sum(-1)
    assert float(n2.max()) * 2 ** 10 < 2 ** 24 and torch.equal(n2 * 2 ** 10, (n2 * 2 ** 10).round())


def emulate_qkn(c, dat, ulps):
    """qknorm_math.h in fp32 for every element: sequential sum of 8, the tree 1, 2, 4, fma-accumulated squares, rstd moved by
    ``ulps`` ulps, the explicit fmas of qkn_finish8 -> bf16 [2, B, S, H * 64]."""
    Bn, S, H, T = c["batch"], c["S"], c["heads"], c["text_rows"]
    x = dat["x"].double()                                              # [2, B, S, H, 64]
    g = x.view(*x.shape[:-1], 8, 8)

    def tree(s):                                                        # [.., 8] lane values -> every lane's total, (g ^ 1), (g ^ 2), (g ^ 4)
        for m in (1, 2, 4):
            s = f32(s + s[..., torch.arange(8) ^ m])
        return s

    s = g[..., 0]
    for i in range(1, 8):
        s = f32(s + g[..., i])
    mean = f32(tree(s) * (1.0 / 64))
    v = f32(g - mean[..., None])
    sq = torch.zeros_like(s)
    for i in range(8):
        sq = fma32(v[..., i], v[..., i], sq)
    var = f32(tree(sq) * (1.0 / 64))
    assert torch.equal(var[..., 0:1], (dat["d"] ** 2).double()) and torch.equal(mean[..., 0:1], dat["mu"].double())
    true_rstd = (1.0 / torch.sqrt(f32(var + dat["eps"]))).float()
    rstd = move_ulps(true_rstd, ulps).double()[..., None]
    w = dat["w"].view(2, 1, 1, 1, 8, 8)
    b = dat["b"].view(2, 1, 1, 1, 8, 8)
    n = fma32(f32(v * rstd), w, b).view(*x.shape)
    out = n.clone()
    if T < S:
        cc = dat["cos"].double()[None, None, :, None]
        ss = dat["sin"].double()[None, None, :, None]
        nv = n[:, :, T:]
        ev, od = nv[..., 0::2], nv[..., 1::2]
        o_ev = fma32(ev, cc[..., 0::2], -f32(od * ss[..., 0::2]))
        o_od = fma32(od, cc[..., 1::2], f32(ev * ss[..., 1::2]))
        out[:, :, T:] = torch.stack([o_ev, o_od], -1).flatten(-2)
    ks = torch.tensor([1.0, c["k_scale"]]).double().view(2, 1, 1, 1, 1)
    out = f32(out * ks)
    return out.reshape(2, Bn, S, H * 64).to(BF)


def qk_pairs(c):
    """The kernel's pair enumeration for case ``c``: (which, z, s, head) int64 arrays over all pairs, and pairs per tensor."""
    ppt = c["batch"] * c["S"] * c["heads"]
    only = c["only"]
    pair = np.arange(ppt * (1 if only else 2))
    which = np.full_like(pair, only - 1) if only else (pair >= ppt).astype(np.int64)
    rest = pair if only else pair - which * ppt
    head, rest = rest % c["heads"], rest // c["heads"]
    return which, rest // c["S"], rest % c["S"], head, ppt


def qk_waves(c):
    """What the waves of eight pairs of case ``c`` meet -> set of names (straddles a token row / a batch entry / the q -> k
    boundary within one wave; the last wave / the last workgroup partial)."""
    which, z, s, head, ppt = qk_pairs(c)
    n = len(which)
    ev = set()
    wave = np.arange(n) // 8
    for name, key in (("straddles_row", z * c["S"] + s + which * 10 ** 9), ("straddles_batch", z + which * 10 ** 6), ("straddles_qk", which)):
        lo = np.full(wave[-1] + 1, np.iinfo(np.int64).max)
        hi = np.full(wave[-1] + 1, -1)
        np.minimum.at(lo, wave, key)
        np.maximum.at(hi, wave, key)
        if name == "straddles_row":                                  # two token rows of one tensor and batch entry
            same = np.zeros(wave[-1] + 1, bool)
            for wv in np.nonzero(lo != hi)[0]:
                sl = slice(wv * 8, min(wv * 8 + 8, n))
                zz, ww, sv = z[sl], which[sl], s[sl]
                same[wv] = any(zz[i] == zz[i + 1] and ww[i] == ww[i + 1] and sv[i] != sv[i + 1] for i in range(len(zz) - 1))
            hit = bool(same.any())
        elif name == "straddles_batch":
            hit = any(which[w8 * 8] == which[min(w8 * 8 + 7, n - 1)] and z[w8 * 8] != z[min(w8 * 8 + 7, n - 1)] for w8 in range(wave[-1] + 1))
        else:
            hit = bool((lo != hi).any())
        if hit:
            ev.add(name)
    if n % 8:
        ev.add("last_wave_partial")
    if ((n + 7) // 8) % 4:
        ev.add("last_workgroup_partial")
    return ev


def qk_stats_table(c, ref):
    """The statistics table the kernel must write: [slots, 2, B * H] fp64, entry = max squared norm of the finished rows over
    the pairs whose workgroup (32 pairs) maps to the slot; 0 where no pair does.  ``ref`` [2, B, S, H * 64] fp64 (bf16 numbers)."""
    which, z, s, head, _ = qk_pairs(c)
    n2 = (ref ** 2).view(2, c["batch"], c["S"], c["heads"], 64).sum(-1).numpy()
    slot = (np.arange(len(which)) // 32) % c["slots"]
    table = np.zeros((c["slots"], 2, c["batch"] * c["heads"]))
    np.maximum.at(table, (slot, which, z * c["heads"] + head), n2[which, z, s, head])
    return torch.from_numpy(table)


def describe_qk(c, bad, got, ref, which):
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "no bad elements"
    z, s, col = (int(v) for v in idx[0])
    head, el = col // 64, col % 64
    ppt = c["batch"] * c["S"] * c["heads"]
    pair = (z * c["S"] + s) * c["heads"] + head + (ppt if which == 1 and not c["only"] else 0)
    return (f"{idx.shape[0]} of {bad.numel()} elements of {'qk'[which]} differ; first: batch entry {z} token row {s} head {head} element {el} "
            f"(pair {pair}, wave {pair // 8}, group {pair % 8}, lane {(pair % 8) * 8 + el // 8}): got {float(got[z, s, col]):g}, "
            f"want {float(ref[z, s, col]):g}")


# ------------------------------------------------------------------------------------------------------------ the case lists
def seed_of(c):
    return sum(ord(ch) for ch in c["name"])


def _ln(D, rows, batch, split, form, eps=0, generic_form=False, out="bf16", kernel="generic", rpw=1, events=()):
    name = f"D{D}-{batch}x{rows}-s{split}-{form}" + ("-eps3" if eps else "") + ("-lngeneric" if generic_form else "") + ("" if out == "bf16" else f"-{out}")
    return dict(name=name, D=D, rows=rows, batch=batch, split=split, form=form, eps=EPS3 if eps else 0.0, generic_form=generic_form,
                out=out, kernel=kernel, rpw=rpw, events=set(events))


ROW_COUNTS = (1, 3, 4, 5, 333)


def _generic_cases():
    out = []
    for i, D in enumerate(WIDTHS):
        for j, form in enumerate(FORMS):
            rows = ROW_COUNTS[(i + j) % 5]
            batch = 2 if (i + j) % 2 or "mod" in form else 1
            split = (rows + 1) // 2 if "mod" in form else 0
            if D == 3072 and form in ("wb", "wbmod"):
                out.append(_ln(D, rows, batch, split, form, generic_form=True))          # <8, 6> with w + b: the reference form only
            else:
                out.append(_ln(D, rows, batch, split, form))
        out.append(_ln(D, ROW_COUNTS[(i + 3) % 5], 2, 1, "mod" if D == 3072 else "wbmod", eps=1))
        out.append(_ln(D, 5, 1, 2, "sens"))
    out.append(_ln(3072, 333, 2, 100, "wbmod", eps=1, generic_form=True))
    return out


ROWS_CASES = [
    _ln(3072, 4, 1, 0, "wb", kernel="rows", rpw=2),
    _ln(3072, 4, 1, 3, "wbmod", kernel="rows", rpw=2, events=["crosses_split"]),
    _ln(3072, 333, 1, 0, "wb", kernel="rows", rpw=2, events=["clipped"]),
    _ln(3072, 333, 1, 101, "wbmod", kernel="rows", rpw=2, events=["crosses_split", "clipped"]),
    _ln(3072, 333, 1, 100, "wbmod", eps=1, kernel="rows", rpw=2, events=["clipped"]),
    # the workload's situation: rows_per_wave 3, 4099 mod 3 = 1 -- a wave crosses the batch boundary, one crosses the split in
    # each batch entry, the last range is clipped
    _ln(3072, 4099, 2, 226, "wbmod", kernel="rows", rpw=3, events=["crosses_split", "crosses_batch", "clipped"]),
    _ln(3072, 4099, 2, 226, "wb", kernel="rows", rpw=3, events=["crosses_batch", "clipped"]),
    _ln(3072, 12291, 1, 5001, "wbmod", kernel="rows", rpw=4, events=["crosses_split", "clipped"]),
    # a batch boundary without a change of side: all rows on one side of the split
    _ln(3072, 5, 2, 0, "wbmod", kernel="rows", rpw=2, events=["crosses_batch", "crosses_batch_same_side"]),
    _ln(3072, 5, 2, 5, "wbmod", kernel="rows", rpw=2, events=["crosses_batch", "crosses_batch_same_side"]),
]
QUANT_CASES = [_ln(3072, rows, batch, split, "quant", out=out) for out in ("fp8", "mxfp8", "mxfp6")
               for rows, batch, split in ((333, 2, 100), (1, 1, 0))]
GENERIC_CASES = _generic_cases()
LN_CASES = GENERIC_CASES + ROWS_CASES + QUANT_CASES


def modulated(c):
    return c["form"] in ("mod", "wbmod", "sens", "quant")


def ln_instance(c, plan=None):
    """The template instance of norm.hip case ``c`` runs, as a string."""
    vec, nv = VEC_NV[c["D"]]
    if c["kernel"] == "rows":
        return f"rows<{nv},{'mod' if 'mod' in c['form'] else 'plain'}>"
    return f"generic<{vec},{nv},{c['out']}>"


LN_INSTANCES = {f"generic<{v},{n},bf16>" for v, n in VEC_NV.values()} | {"generic<8,6,fp8>", "generic<8,6,mxfp8>", "generic<8,6,mxfp6>",
                                                                          "rows<6,mod>", "rows<6,plain>"}


def _qk(heads, batch, S, text_rows, only=0, k_scale=1.0, eps=0, slots=0, events=()):
    name = f"H{heads}-{batch}x{S}-t{text_rows}-{('qk', 'q', 'k')[only]}-ks{k_scale:g}" + ("-eps3" if eps else "") + (f"-stats{slots}" if slots else "")
    return dict(name=name, heads=heads, batch=batch, S=S, text_rows=text_rows, only=only, k_scale=k_scale, eps=EPS3 if eps else 0.0,
                slots=slots, events=set(events))


_ALL3 = ["straddles_row", "straddles_batch", "straddles_qk"]
QK_CASES = [
    _qk(1, 1, 5, 0, events=["last_wave_partial", "last_workgroup_partial"]),
    _qk(1, 2, 19, 4, k_scale=0.25, slots=64),
    _qk(3, 2, 35, 7, k_scale=0.25, events=_ALL3 + ["last_wave_partial", "last_workgroup_partial"]),
    _qk(3, 2, 35, 0, only=1, k_scale=0.25, events=["straddles_row", "straddles_batch", "last_wave_partial"]),
    _qk(3, 1, 35, 35, only=2, k_scale=0.25, events=["straddles_row", "last_wave_partial"]),
    _qk(3, 2, 35, 7, k_scale=0.25, slots=8, events=_ALL3),
    _qk(6, 2, 37, 5, events=_ALL3 + ["last_workgroup_partial"]),
    _qk(6, 2, 37, 5, only=1, k_scale=0.25, events=["straddles_row", "straddles_batch", "last_wave_partial"]),
    _qk(6, 2, 37, 36, only=2, k_scale=0.25, slots=8, events=["straddles_row", "straddles_batch"]),
    _qk(6, 1, 35, 3, eps=1, k_scale=0.25, events=["straddles_row", "straddles_qk", "last_wave_partial"]),
    _qk(6, 2, 37, 0, slots=1, events=_ALL3),
    _qk(8, 2, 9, 9),
    _qk(8, 1, 7, 2, k_scale=0.25, only=2),
    _qk(48, 1, 11, 3, k_scale=0.25),
    _qk(48, 2, 5, 0, eps=1),
]
