"""Conditioning of the attention kernels (a plain helper module: no tests, no fixtures; the sibling of ``cond_norm.py``).
The exact-data suite (exact_attn.py) draws probabilities that are powers of two and outputs of 8 significant bits, so it cannot see
how a kernel rounds P or O, what the lazy-rescale threshold does to a row whose maximum creeps up, or what a constant under a row's
scores does to its sum; the random-data tests see those through one relative Frobenius norm over N(0, 1) data, where none of it
matters.  Here every (batch, head) holds rows of every SCORE FAMILY below and every output element is held to the fp64 softmax of
the bf16 values the kernel reads.

DATA (``build``).  One K and one V per (batch, head) and key/value variant (level-2 batch, identity); the family is chosen by the
QUERY ROW.  K carries eight structured coordinates and gaussian noise (sd 1/4) in the other D - 8; a q row switches coordinates on:
    0  const    k = 1                                  q = -60 / +60: a constant under every score of the row
    1  wide     k = w_j, uniform in [-1, 1], +-1 hit   q = 80 (wide), 20 (the spread of the shifted rows), LARGE (large)
    2  rise-3   k grows by 3 / amplitude per 64-key tile, 3  rise-7 by 7,  4  fall: falls by FALL_RATE per tile
    5..7 peaks  k = 1 at ONE key each: in the first tile, in the interior, the last key (the ragged tail);  q = 40
Everything is rounded to bf16 before anything is computed from it.  Scores are in exp2 units (the kernels that scale themselves
get exact_attn.UNIT_SCALE; attn_tiny gets ln 2).
    friendly     gaussian, sd 3                                             the control
    flat         q = 0: every score 0, P = 1 everywhere, l = Skv
    peaked       one key 40 above gaussian scores of sd 3/4; the key cycles over first tile / interior / last key
    shift-low/-high   -60 / +60 under every score, spread +-20              the static kernels' range; padding keys counted at P = 1
    rising-3 / -7     the tile maximum grows by 3 / 7 per tile              under / over RESCALE_THR = 6
    falling      maximum in the first tile, then down by >= 2 per tile to -160: P underflows harmlessly
    wide         uniform over +-80                                          the whole range of a static bound in one row
    large        uniform over +-LARGE (300 at D = 64, 180 at D = 128)       running-maximum kernels: the two-term bf16 split of m_run
The static and device-bound kernels promise |s| <= bound <= 90 (include/bya.h), so ``large`` is not given to them and their rising
and falling rows run from -80 to +80 and stop there (with the noise: inside +-85).  The running-maximum kernels get 0 .. CAP (252
at D = 64, 160 at D = 128) and 0 .. -160.  |s| ~ 1000 would put the analytic bar below out of reach: the fp32 accumulation of a
score of magnitude S_abs is itself uncertain by (D + 2) u32 S_abs, which at 1000 is 0.7 of the unit; LARGE and CAP are the largest
round amplitudes that keep eps <= 0.5 at 4133 keys.  One-tile paths (kv-mix, attn_tiny: at most 64 / 32 keys) drop the three
families that need a second tile.  Nothing else is left out.
The device-bound kind takes B = sqrt(max |q|^2 max |k|^2) per head, a Cauchy-Schwarz bound that is several times the largest
score of rows built from eight coordinates; ``scale_for_device_bound`` scales q per head so that B is 85 (even heads: static kernel)
or 100 (odd heads: flagged, running-maximum kernel), and the families keep their shape at about a third of the amplitude (the
peak coordinates are raised to 80 x 1.5 there, which moves neither largest norm and leaves the peak 40 above the rest).
V: the first D / 2 columns are |N(0, 1)| + 1, the rest N(0, 1).
ROW LAYOUT.  Interleaved: the family changes every row.  Cases with Sq >= 32 * (number of families) hold on their odd (batch, head)s
the blocked layout, the family changing every 32 rows: a whole wave then sits on one family (else a neighbour's row trips the
wave-uniform rescale branch for ``rising-3``).

MEASURE.  From fp64 on the bf16 inputs:  o64 = sum_j p_j v_j / l,  A = sum_j p_j |v_j| / l,  and per element
    e = |got - o64| / (2^-8 (A + |o64|)).
A is what the errors of P scale with; an output near zero by cancellation is not held to its own ulp.

BAR (a): e <= 1 + eps for every element.  Derivation: write P~_j = p_j (1 + d_j), |d_j| <= u = 2^-8 for the rounding of P to bf16
(the row sum l is taken from the unrounded P in every kernel), so O~ = sum_j P~_j v_j / l differs from o64 by at most u A; the final
rounding to bf16 adds at most u |O~| <= u (|o64| + u A).  Together |got - o64| <= u (A + |o64|) (1 + u), i.e. e <= 1 apart from the
fp32 terms, which are eps:
    eps = 2^8 u32 (2 Skv + ln 2 (D + 2) S_abs) + 1/16,   u32 = 2^-24,  S_abs = max_ij sum_d |q_id k_jd|
  * 2 Skv u32: the fp32 row sum and the fp32 accumulation of P . V over Skv terms of one sign pattern, worst case, each;
  * ln 2 (D + 2) S_abs u32: a score is an fp32 sum of D exact products and the two terms of -m_run, in any order, off by at most
    (D + 2) u32 S_abs; through exp2 that is a relative ln 2 times as much in P;
  * 1/16 for v_exp_f32 and v_rcp_f32 (1 ulp each of fp32 is 2^-15 of the unit; the sixteenth is generous on purpose).
kv-mix adds n_id u32 2^8 for its fp32 mix and attn_tiny 2 S_abs u32 ln 2 2^8 for q * scale and the argument of __expf; neither is
visible.  No term comes from a kernel's output.  attn_tiny keeps P in fp32: it sits near 0.5.
kv-mix: z = sum_id w_id O_id with unit 2^-8 (sum_id w_id A_id + |z|).  attn_mix32.h and attn_mix_body accumulate w_id / l_id * O_id
in fp32 and round z once, so there is no term for a rounded per-identity O.

BAR (b): bias.  Over the positive-V columns, per family (flat excluded: P = 1 is exact),  b = mean((got - o64) / A) / 2^-9; the bar
is |b| <= |b of the RESTATEMENT| + 0.25.  The restatement (``restate``) is computed at test time on the same inputs: fp32 scores,
row maximum, exp2, fp32 row sum, P rounded to bf16, fp32 P . V, one division, one rounding to bf16.  Correct variants measure at
most 0.1, a truncation of P or of O at least 0.5 (test_attn_cond_cpu.py asserts both at the suite's shapes).
BAR (c): every output finite, the guard band intact, no poison left.
"""
import functools
import math

import torch

import exact_attn as X
from exact_attn import BF

U32 = 2.0 ** -24
UNIT = 2.0 ** -8
BIAS_UNIT = 2.0 ** -9
BIAS_MARGIN = 0.25
EPS_MAX = 0.5
FAMILIES = ("friendly", "flat", "peaked", "shift-low", "shift-high", "rising-3", "rising-7", "falling", "wide", "large")
MULTI_TILE = ("rising-3", "rising-7", "falling")
STATIC_KINDS = ("w4", "dev")
NCOORD = 8
K_NOISE = 0.25
NOISE_SD = {"friendly": 3.0, "flat": 0.0}
STRUCT_SD = 0.75
PEAK = 40.0
DEV_PEAK = (80.0, 1.5)                     # (q, k) of the peak coordinates under the device bound: 120, about 40 once q is scaled
SHIFT, SPREAD, WIDE = 60.0, 20.0, 80.0
STATIC_AMP = 80.0                          # rising / falling rows of the static kinds run over [-80, 80]
CAP = {64: 252.0, 128: 160.0}              # where the rising rows of the running-maximum kinds stop
LARGE = {64: 300.0, 128: 180.0}
FALL = 160.0
BOUND_LOW, BOUND_HIGH = 85.0, 100.0        # the two targets of the device bound; BYA_ATTN_BOUND_LIMIT = 90 lies between
RESCALE_THR = 6.0


def families_of(path):
    """The families a path admits.  path: an attention kind (run, pre, d128, w4, dev), "mix" or "tiny"."""
    if path in STATIC_KINDS:
        return tuple(f for f in FAMILIES if f != "large")
    if path in ("mix", "tiny"):
        return tuple(f for f in FAMILIES if f not in MULTI_TILE)
    return FAMILIES


def fall_rate(nt):
    """Per-tile fall of ``falling``: 2 where that reaches -152 by the last tile, else as steep as it takes."""
    return 0 if nt < 2 else max(2, -(-152 // (nt - 1)))


def seed_of(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def build(Sq, Skv, D, nbh, fams, static, seed, nkv=1, heads=None, peak_qk=(PEAK, 1.0)):
    """-> dict: q [nbh, Sq, D], k, v [nbh, nkv, Skv, D] (fp32 holding bf16 values), fam [nbh, Sq] (index into FAMILIES), peak [nbh,
    Sq] (which of ``peaks`` a peaked row selects), peaks (the three key positions), blocked [nbh] bool, factor [nbh] (1: see
    ``scale_for_device_bound``), static."""
    gen = torch.Generator().manual_seed(seed)
    heads = heads or nbh
    NF, Dn = len(fams), D - NCOORD
    nt = -(-Skv // 64)
    t = (torch.arange(Skv) // 64).float()
    rate = fall_rate(nt)
    if static:
        a_rise = a_fall = STATIC_AMP
        f3, f7 = (torch.clamp(3 * t, max=160.0) - 80) / 80, (torch.clamp(7 * t, max=160.0) - 80) / 80
        ff = (80 - torch.clamp(rate * t, max=160.0)) / 80
    else:
        a_rise, a_fall = CAP[D], FALL
        f3, f7 = torch.clamp(3 * t, max=a_rise) / a_rise, torch.clamp(7 * t, max=a_rise) / a_rise
        ff = -torch.clamp(rate * t, max=FALL) / FALL
    peaks = (min(5, Skv - 1), Skv // 2, Skv - 1)
    k = torch.zeros(nbh, nkv, Skv, D)
    k[..., 0] = 1.0
    w = torch.rand(nbh, nkv, Skv, generator=gen) * 2 - 1
    j_hi = (3 + 5 * torch.arange(nbh * nkv).view(nbh, nkv, 1)) % Skv
    w.scatter_(2, j_hi, 1.0)
    if Skv > 1:
        w.scatter_(2, (j_hi + 1) % Skv, -1.0)
    k[..., 1], k[..., 2], k[..., 3], k[..., 4] = w, f3, f7, ff
    for c, p in enumerate(peaks):
        k[:, :, p, 5 + c] = peak_qk[1]
    k[..., NCOORD:] = torch.randn(nbh, nkv, Skv, Dn, generator=gen) * K_NOISE
    v = torch.randn(nbh, nkv, Skv, D, generator=gen)
    v[..., :D // 2] = v[..., :D // 2].abs() + 1

    bh, i = torch.arange(nbh)[:, None], torch.arange(Sq)[None, :]
    blocked = (torch.arange(nbh) % 2 == 1) & (Sq >= 32 * NF)
    local = torch.where(blocked[:, None], (i // 32 + bh) % NF, (i + bh) % NF)
    peak = torch.where(blocked[:, None], (i % 3).expand(nbh, Sq), ((i // NF) % 3).expand(nbh, Sq))
    fam = torch.tensor([FAMILIES.index(f) for f in fams])[local]
    amp = torch.zeros(len(FAMILIES), 5)
    sd = torch.full((len(FAMILIES),), STRUCT_SD)
    for f, s in NOISE_SD.items():
        sd[FAMILIES.index(f)] = s
    ix = FAMILIES.index
    amp[ix("shift-low"), 0], amp[ix("shift-low"), 1] = -SHIFT, SPREAD
    amp[ix("shift-high"), 0], amp[ix("shift-high"), 1] = SHIFT, SPREAD
    amp[ix("rising-3"), 2], amp[ix("rising-7"), 3], amp[ix("falling"), 4] = a_rise, a_rise, a_fall
    amp[ix("wide"), 1], amp[ix("large"), 1] = WIDE, LARGE[D]
    q = torch.zeros(nbh, Sq, D)
    q[..., :5] = amp[fam]
    is_peak = fam == ix("peaked")
    q[..., 5:8] = torch.where(is_peak[..., None] & (peak[..., None] == torch.arange(3)), peak_qk[0], 0.0)
    q[..., NCOORD:] = torch.randn(nbh, Sq, Dn, generator=gen) * (sd[fam] / (K_NOISE * math.sqrt(Dn)))[..., None]
    r = lambda x: x.to(BF).float()
    return dict(q=r(q), k=r(k), v=r(v), fam=fam, peak=peak, peaks=peaks, blocked=blocked, factor=torch.ones(nbh, dtype=torch.float64),
                static=static, fams=tuple(fams))


def scale_for_device_bound(d, heads):
    """Scale q of every (batch, head) so that the bound the device-bound kernel derives, B = sqrt(max |q|^2) sqrt(max |k|^2), is
    BOUND_LOW on even heads and BOUND_HIGH on odd ones for every key/value variant of the head (at most on the even, at least on
    the odd ones; the variants' largest key norms differ by a few per cent)."""
    qn = d["q"].double().norm(dim=-1).amax(1)
    kn = d["k"].double().norm(dim=-1).amax(2)
    high = (torch.arange(qn.numel()) % heads) % 2 == 1
    factor = torch.where(high, BOUND_HIGH / (qn * kn.amin(1)) * (1 + 2.0 ** -7), BOUND_LOW / (qn * kn.amax(1)))
    factor = torch.where(qn > 0, factor, 1.0)                     # (a head whose only row is the flat one: B = 0)
    d["q"] = (d["q"] * factor[:, None, None].float()).to(BF).float()
    d["factor"] = factor
    return d


def device_bound_stats(d, B, H, dev, bh0=2):
    """The statistics table as bya_qknorm_rope would leave it -> (stats fp32 [2, 2, n + 5] with column bh0 + (b L2 + l2) H + h, the
    two slots holding the largest squared row norms of the first and of the second half of the rows; B fp32 [n] in that order,
    computed as the kernel does: sqrtf(max q2) * sqrtf(max k2))."""
    nbh, nkv = d["k"].shape[:2]
    q2, k2 = d["q"].pow(2).sum(-1), d["k"].pow(2).sum(-1)                     # [nbh, Sq], [nbh, nkv, Skv]
    Sq, Skv = q2.shape[-1], k2.shape[-1]
    qs = torch.stack([q2[:, :(Sq + 1) // 2].amax(-1), q2[:, Sq // 2:].amax(-1)])                          # [2, nbh]
    ks = torch.stack([k2[..., :(Skv + 1) // 2].amax(-1), k2[..., Skv // 2:].amax(-1)])                    # [2, nbh, nkv]
    order = lambda x: x.view(2, B, H, nkv).permute(0, 1, 3, 2).reshape(2, -1)                               # (b, h, l2) -> (b, l2, h)
    qs, ks = order(qs[:, :, None].expand(2, nbh, nkv)), order(ks)
    n = qs.shape[1]
    stats = torch.zeros(2, 2, n + 5)
    stats[:, 0, bh0:bh0 + n], stats[:, 1, bh0:bh0 + n] = qs, ks
    bound = torch.sqrt(qs.amax(0)) * torch.sqrt(ks.amax(0))
    return stats.to(dev), bound


# ------------------------------------------------------------------------------------------------------------ reference and restatement
def _row_chunks(n, Sq, Skv, limit=1 << 24):
    """(head range, row range)s with at most ``limit`` scores each."""
    if Sq * Skv <= limit:
        g = max(1, limit // (Sq * Skv))
        return [(a, min(a + g, n), 0, Sq) for a in range(0, n, g)]
    rows = max(32, limit // Skv // 32 * 32)
    return [(a, a + 1, r0, min(r0 + rows, Sq)) for a in range(n) for r0 in range(0, Sq, rows)]


def reference64(q, k, v):
    """fp64 softmax attention, scores in exp2 units: q [n, Sq, D], k, v [n, Skv, D] -> (o64, A) fp64 [n, Sq, D]."""
    n, Sq, D = q.shape
    o = torch.empty(n, Sq, D, dtype=torch.float64, device=q.device)
    A = torch.empty_like(o)
    for a, b, r0, r1 in _row_chunks(n, Sq, k.shape[1]):
        s = q[a:b, r0:r1].double() @ k[a:b].double().transpose(1, 2)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        vd = v[a:b].double()
        ov = (p @ torch.cat([vd, vd.abs()], -1)) / p.sum(-1, keepdim=True)
        o[a:b, r0:r1], A[a:b, r0:r1] = ov[..., :D], ov[..., D:]
    return o, A


def s_abs(q, k):
    """max_ij sum_d |q_id k_jd| over q [n, Sq, D], k [n, Skv, D] (fp32 is plenty for a bound's coefficient: 1 + 2^-17)."""
    worst = 0.0
    qa, ka = q.float().abs(), k.float().abs()
    for a, b, r0, r1 in _row_chunks(q.shape[0], q.shape[1], k.shape[1]):
        worst = max(worst, float((qa[a:b, r0:r1] @ ka[a:b].transpose(1, 2)).max()))
    return worst * (1 + 2.0 ** -17)


def eps_of(Skv, D, sabs, n_id=0, tiny=False):
    """The fp32 terms of bar (a): the module docstring."""
    return 2.0 ** 8 * U32 * (2 * Skv + math.log(2.0) * (D + 2 + (2 if tiny else 0)) * sabs + n_id) + 1.0 / 16


def _trunc_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _two_term(m):
    hi = m.to(BF).float()
    return hi + (m - hi).to(BF).float()


def restate(q, k, v, form="rowmax", fault=None, rows=None, rounded=True):
    """The attention of q [n, Sq, D], k, v [n, Skv, D] in fp32 torch with P rounded to bf16 for P . V, one division, one rounding
    (``rounded`` False: the fp32 quotient, for kv-mix).
    form  "rowmax": the RESTATEMENT -- row maximum, exp2, fp32 row sum.
          "static": no offset at all, P = exp2(s)  (the static-bound kernels; for rows with |s| <= 90).
          "tiled":  64-key tiles, online softmax as attn_tile runs it: a reference point kept as a two-term bf16 value, moved (and O,
                    l rescaled) only when some row of the 32-row block grows past it by more than RESCALE_THR; the first tile sets it.
    fault (planted, on the rows of the bool mask ``rows`` [n, Sq], all rows if None):
          "p_trunc" / "o_trunc": P / the output truncated to bf16 instead of rounded;
          "drop_last": the last key is never added;  "pad_zero": one padding key counted at score 0 with V = 0."""
    n, Sq, D = q.shape
    Skv = k.shape[1]
    out = torch.empty(n, Sq, D, dtype=torch.float32, device=q.device)
    hit = torch.ones(n, Sq, dtype=torch.bool, device=q.device) if rows is None else rows.to(q.device)
    p_bf = (lambda p: _trunc_bf16(p)) if fault == "p_trunc" else (lambda p: p.to(BF).float())
    for a, b, r0, r1 in _row_chunks(n, Sq, Skv):
        s = q[a:b, r0:r1].float() @ k[a:b].float().transpose(1, 2)
        vf = v[a:b].float()
        h = hit[a:b, r0:r1]
        if fault == "pad_zero":                                     # a key of score 0 and V = 0 behind the last one
            s = torch.cat([s, torch.where(h, 0.0, -math.inf)[..., None]], -1)
            vf = torch.cat([vf, torch.zeros_like(vf[:, :1])], 1)
        if fault == "drop_last":
            s[..., Skv - 1] = torch.where(h, -math.inf, s[..., Skv - 1])
        if form in ("rowmax", "static"):
            p = torch.exp2(s if form == "static" else s - s.amax(-1, keepdim=True))
            O, l = p_bf(p) @ vf, p.sum(-1)
        else:
            R = s.shape[1]
            O, l = torch.zeros(b - a, R, D, device=q.device), torch.zeros(b - a, R, device=q.device)
            m = torch.zeros(b - a, R, device=q.device)
            for t0 in range(0, s.shape[-1], 64):
                st = s[..., t0:t0 + 64]
                mx = st.amax(-1) - m
                if t0 == 0:
                    m_new = _two_term(mx)
                else:
                    pad = (-R) % 32                                   # the branch is uniform over a wave's 32 rows
                    trip = torch.nn.functional.pad(mx > RESCALE_THR, (0, pad)).view(b - a, -1, 32).any(-1, keepdim=True)
                    trip = trip.expand(-1, -1, 32).reshape(b - a, -1)[:, :R]
                    m_new = torch.where(trip, _two_term(m + mx.clamp_min(0.0)), m)
                    alpha = torch.exp2(m - m_new)
                    O, l = O * alpha[..., None], l * alpha
                m = m_new
                p = torch.exp2(st - m[..., None])
                l = l + p.sum(-1)
                O = O + p_bf(p) @ vf[:, t0:t0 + 64]
        o = O / l[..., None]
        if fault == "o_trunc":
            o = _trunc_bf16(o)
        out[a:b, r0:r1] = o
    return out.to(BF) if rounded else out


# ------------------------------------------------------------------------------------------------------------ measure and bars
def figures(got, o64, A, fam):
    """Per family present: (worst e, bias b in units of 2^-9 over the positive-V columns, all finite).  got, o64, A [..., rows, D];
    fam [..., rows] (index into FAMILIES)."""
    D = got.shape[-1]
    g = got.double()
    e = torch.nan_to_num((g - o64).abs() / (UNIT * (A + o64.abs())), nan=math.inf)
    r = ((g - o64) / A)[..., :D // 2]
    fam = fam.to(got.device)
    out = {}
    for i, name in enumerate(FAMILIES):
        m = fam == i
        if bool(m.any()):
            out[name] = (float(e[m].max()), float(r[m].mean()) / BIAS_UNIT, bool(torch.isfinite(g[m]).all()))
    return out


def check(name, got, o64, A, restated, fam, fams, eps, plan=None, out=print):
    """Print worst e, eps and b of ``got`` and of the restatement per family, then assert the three bars of the module docstring.
    -> {family: (worst e, b, the restatement's worst e, its b)}."""
    assert eps <= EPS_MAX, f"{name}: eps {eps:.3f} leaves bar (a) without meaning"
    mine, rest = figures(got, o64, A, fam), figures(restated.to(got.device), o64, A, fam)
    assert set(mine) == set(fams), f"{name}: the case does not hold exactly its path's families: {sorted(mine)}"
    failed = []
    for f in fams:
        (w, b, finite), (rw, rb, _) = mine[f], rest[f]
        out(f"{name} | {f:10s} | worst e {w:6.3f} (bar {1 + eps:.3f}, eps {eps:.3f}), b {b:+6.3f} | restatement: worst e {rw:5.3f}, b {rb:+6.3f}"
            + ("" if f == "flat" else f" (bar {abs(rb) + BIAS_MARGIN:.3f})"))
        if not finite:
            failed.append(f"{f}: a result is not finite")
        elif not w <= 1 + eps:
            failed.append(f"{f}: worst e {w:.3f} > 1 + eps = {1 + eps:.3f}")
        elif f != "flat" and not abs(b) <= abs(rb) + BIAS_MARGIN:
            failed.append(f"{f}: bias {b:+.3f} x 2^-9 against the restatement's {rb:+.3f} + {BIAS_MARGIN}")
    assert not failed, f"{name} [plan {plan}]: " + "; ".join(failed)
    return {f: (mine[f][0], mine[f][1], rest[f][0], rest[f][1]) for f in fams}


# ------------------------------------------------------------------------------------------------------------ the GPU matrix
def _kind_cases(kind):
    """The small shapes carry many (batch, head)s: the bias of a family is a mean over its rows, a row's P errors are shared by
    its columns (sd about 0.4 x 2^-9 per row), and the correct variants stay within 0.1 only from about 150 rows per family."""
    a = X._a
    return [
        a(f"{kind}-40x40", kind, 40, 40, 8, B=8),
        a(f"{kind}-64x64", kind, 64, 64, 8, B=3),
        a(f"{kind}-200x200", kind, 200, 200, 4, B=2),
        a(f"{kind}-1350x1350", kind, 1350, 1350, 4, pad=24),
        a(f"{kind}-513x4133", kind, 513, 4133, 4),
        a(f"{kind}-1031x4133-narrow", kind, 1031, 4133, 3, col0=4),
        a(f"{kind}-127x32-cross", kind, 127, 32, 6, B=2, L2=2, narrow=True),
        a(f"{kind}-1x8", kind, 1, 8, 40, B=40),          # one row per head: the family changes with the head
    ]


ATTN_CASES = sum((_kind_cases(kd) for kd in ("run", "pre", "d128", "w4", "dev")), []) + [
    X._a("w4-streamk-5056x32", "w4", 5056, 5056, 32, sk=True),
    X._a("w4-streamk-5056x32-narrow", "w4", 5056, 5056, 32, sk=True, col0=4),
    X._a("w4-streamk-off-5056x32", "w4", 5056, 5056, 32, sk_opt=0),
    X._a("dev-streamk-5056x32", "dev", 5056, 5056, 32, sk=True),
    X._a("dev-streamk-off-5056x32", "dev", 5056, 5056, 32, sk_opt=0),
]
POISON_SHAPES = ("40x40", "200x200", "513x4133")         # ragged last tiles: under one tile, four, sixty-five


@functools.lru_cache(maxsize=2)                  # (cases that differ only in the grid or the store width share their data)
def _attn_data(kind, B, H, L2, Sq, Skv, D):
    static = kind in STATIC_KINDS
    d = build(Sq, Skv, D, B * H, families_of(kind), static, seed_of(f"{kind}-{B}x{H}x{L2}-{Sq}x{Skv}"), nkv=L2, heads=H,
              peak_qk=DEV_PEAK if kind == "dev" else (PEAK, 1.0))
    return scale_for_device_bound(d, H) if kind == "dev" else d


def attn_case_data(c):
    """The case's data on the CPU (cached: treat as read-only)."""
    return _attn_data(c["kind"], c["B"], c["H"], c["L2"], c["Sq"], c["Skv"], c["D"])


def per_variant(d, dev="cpu"):
    """q expanded over the key/value variants -> (q [nbh * nkv, Sq, D], k, v [nbh * nkv, Skv, D], fam [nbh * nkv, Sq]) on ``dev``."""
    nbh, nkv, Skv, D = d["k"].shape
    Sq = d["q"].shape[1]
    q = d["q"].to(dev)[:, None].expand(nbh, nkv, Sq, D).reshape(nbh * nkv, Sq, D)
    fam = d["fam"][:, None].expand(nbh, nkv, Sq).reshape(nbh * nkv, Sq)
    return q, d["k"].to(dev).reshape(nbh * nkv, Skv, D), d["v"].to(dev).reshape(nbh * nkv, Skv, D), fam


def case_eps(c, q, k):
    return eps_of(c["Skv"], c["D"], s_abs(q, k))


MIX_NAMES = ("audio-d64-3id-kv20", "audio-d64-4id", "face-d128-2id", "face-d128-4id-big-lds", "face-d64-kv33", "audio-d64-kv64",
             "audio-d64-generic", "face-d128-misaligned-z", "face-d128-kv64")
MIX_CASES = [c for c in X.MIX_CASES if c["name"] in MIX_NAMES]
assert len(MIX_CASES) == len(MIX_NAMES) and {c["Skv"] for c in MIX_CASES} == {20, 32, 33, 64}
MIX_POISON = ("audio-d64-3id-kv20", "face-d64-kv33")


def mix_case_data(c, dev="cpu"):
    """build's dict for the case (K / V variants = identities) plus r, af, w [grp * Sq, n_id], wsum of exact_attn.mix_weights."""
    d = dict(build(c["Sq"], c["Skv"], c["D"], c["grp"] * c["H"], families_of("mix"), False, seed_of("mix-" + c["name"]), nkv=c["n_id"],
                   heads=c["H"]))
    r, af, w = X.mix_weights(c["grp"] * c["Sq"], c["n_id"], c["audio"], dev, seed=seed_of(c["name"]) % 1000)
    d.update(r=r, af=af, w=w, wsum=w.sum(1))
    return d


def mix_reference(c, d, dev="cpu", form="rowmax", fault=None):
    """-> (z64, sum_id w_id A_id, the restatement's z bf16, fam), all [grp * H, Sq, D] / [grp * H, Sq]: the fp64 mix of the fp64
    per-identity attentions, and the fp32 mix of the un-rounded fp32 restatements, rounded once."""
    G, H, n_id, Sq, D = c["grp"], c["H"], c["n_id"], c["Sq"], c["D"]
    q, k, v, _ = per_variant(d, dev)
    o64, A = reference64(q, k, v)
    o32 = restate(q, k, v, form, fault, rounded=False)
    w = d["w"].to(dev).view(G, 1, Sq, n_id).expand(G, H, Sq, n_id).reshape(G * H, Sq, n_id)
    mix = lambda t, wt: torch.einsum("bisd,bsi->bsd", t.view(G * H, n_id, Sq, D), wt)
    return mix(o64, w.double()), mix(A, w.double()), mix(o32, w.float()).to(BF), d["fam"]


TINY_NAMES = ("L2-h8-1x203-multi-id", "L3-h16-2x9", "L13-h8-2x45", "L25-h8-2x15", "L2-h6-1x11-multi-id", "L4-h6-2x5", "L16-h6-1x3",
              "L32-h6-1x2", "L13-h8-1x9-unaligned")
TINY_CASES = [c for c in X.TINY_CASES if c["name"] in TINY_NAMES]
assert len(TINY_CASES) == len(TINY_NAMES)
TINY_POISON = ("L13-h8-2x45", "L13-h8-1x9-unaligned")


def tiny_case_data(c):
    """-> (build's dict with nbh = groups * H and Sq = Skv = L, rows of the q | k | v matrix, row ids [groups, L])."""
    L, H, no, ni = c["L"], c["H"], c["n_outer"], c["n_inner"]
    groups = no * ni
    d = build(L, L, 64, groups * H, families_of("tiny"), False, seed_of("tiny-" + c["name"]), heads=H)
    rows = no * L * ni if c["temporal"] else L * ni
    idx = (torch.arange(no)[:, None, None] * (L * ni if c["temporal"] else 0) + torch.arange(L)[None, None, :] * ni
           + torch.arange(ni)[None, :, None]).reshape(groups, L)
    return d, rows, idx
