"""Exact-data checking of the small kernels of the denoise step (a plain helper module: no tests, no fixtures; the sibling of
``exact_gemm.py``, ``exact_attn.py``, ``exact_rowk.py``, ``exact_norm.py`` and ``exact_vae.py``, whose ``GuardedOut`` / ``bad_elements`` /
``describe`` / ``assert_exact`` / ``pow2`` / ``POISON`` / ``SENTINEL``, +-1 pattern rows and ``SILU_WINDOW`` it reuses): csrc/misc.hip
(bya_linear_small_m, bya_timestep_features, bya_masked_combine, bya_routed_mix, bya_forcing_max_over_frames, bya_patchify /
bya_unpatchify, bya_act_add, bya_cfg_scheduler_step) and csrc/router.hip (bya_router_scores, bya_router_head).  Every case has data
for which a correct kernel's answer is a function of the data alone; the check is bit equality with an fp64 reference of the
DEFINITION rounded once (+0 and -0 equal), the few inexact functions have DERIVED bounds, outputs sit inside a sentinel buffer and a
failure names the element with its row, workgroup, wave and lane.  The case tables are module constants: test_step_exact_cpu.py
checks their conditions and plans without a GPU and plants faults.

SMALL-M LINEAR (``LIN_CASES``).  Operands of ``exact_gemm.exact_operands`` / ``exact_epilogue``: every product is a multiple of 2^-2
of at most 36, any partial sum of K <= 3072 of them is below 3072 * 36 * 4 < 2^19 units, + bias (b 2^-2, |b| <= 16): exact in fp32
in every order of the 64 lanes' pieces and of the wave reduction (``lin_bound``, ``lin_units``).  M in {1, 2} is the 2-row
instantiation, M in {3, 5, 8} the 8-row one (the face mapper's); N in {5, 1027}: a last workgroup with idle waves; K in {8, 504, 520, 1280, 3072}: one
lane only / lanes 63 idle / lane 0 with two pieces / the production K (lanes 0..31 three pieces, the others two) / six pieces.
``silu_in``: x in {0, 32, 64, -128}, where x / (1 + __expf(-x)) is x, x, x and -0 exactly (fp32 1 + exp(-32) = 1; __expf(128) = inf)
and so is bf16(fp64 SiLU(x)) (|SiLU(32) - 32| = 4e-13; SiLU(-128) = -3e-54 rounds to -0); W = b 2^rw, b in [-3, 3], rw in {-1, 0,
1}: products are multiples of 16 of at most 768, sums below 3072 * 768 < 2^22 are, with the bias, multiples of 2^-2 below 2^24
units.  ``act_out`` = SiLU: a 2^-6 scales the pre-activation p to |p| <= 32 (asserted), still exact; the output follows the WINDOW
RULE.

WINDOW RULE (SiLU, sigmoid).  ``SILU_WINDOW`` = 2^-16 relative and its 2 % cap are exact_vae.py's: an element whose fp64 value lies
farther than the window from a bf16 rounding boundary must match bit for bit, an element inside may be either neighbour, and the
builders take the first seed whose data keeps at most 2 % of a case inside.  Noise of p / (1 + __expf(-p)), __expf(v) = v_exp_f32(v
log2 e): for |p| <= 32 the argument t = p log2 e is below 64, its fp32 rounding costs 2^-19 absolute, the constant's own rounding
46 * 2^-25 = 2^-19.5, i.e. (times ln 2) 2^-19.5 + 2^-20 relative in the exponential, v_exp_f32 and the division an ulp (2^-23) each:
about 2^-18.6 in all, the result's sensitivity to the exponential being e / (1 + e) <= 1; the window is five times that.  SIGMOID 1 /
(1 + __expf(-z)) at |z| <= 8: |t| < 16, 2^-21 absolute + 2^-21.5, i.e. 2^-21.5 + 2^-22 relative, + 2^-23 + 2^-24 + 2^-24: about
2^-20.3; the window is twenty times that, so the derivation needs no wider one.

TIMESTEP FEATURES.  Exact part: t = 0 makes the angle 0 * expf(..) = 0, so sin = 0 and cos = 1 bit for bit: this pins the layout
([cos | sin] with flip, [sin | cos] without).  Bounded part, element by element against fp64 sin / cos of a = t exp(-ln(10000) j /
(half - shift)): the kernel computes expo = fl(fl(-L j) / (half - shift)) with L = logf(10000) (one rounding + at most 1 ulp: 3 half
ulps), a product and an IEEE division (a half ulp each; half - shift is exact): |d expo| <= 5 * 2^-24 |expo|; expf (1 ulp) turns
that into a RELATIVE error of 5 * 2^-24 |expo| + 2 * 2^-24, the product with t adds 2^-24: |d a| <= a (5 |expo| + 3) 2^-24
(``angle_budget``; at most 2.0e-4, at t = 999 and expo = -0.4); sinf / cosf: 2 ulps of a value below 1 (4 * 2^-24 absolute) and |d
sin| <= |d a|.  The bound is half a bf16 ulp of (|reference| + budget) + budget: at most 2^-9 + 2.0e-4 = 2.2e-3, five times tighter
than the older test's 1.2e-2.  Nothing in it is measured.

ROUTER SCORES (``SCORES_CASES``).  Every key row kr[id, tok, h, :] is ONE-HOT: a single 1 at perm_h[32 id + tok], perm_h a seeded
permutation of the head's 128 dims, so the positions of different identities are disjoint and, with four identities, partition
the head.  Feature f = 16 tok + h of token n is then the ENTRY qr[n, 128 h + perm_h[32 id + tok]] (one non-zero product per MFMA
accumulator: exact), and the entries are mu + d e: e a +-1 row with 256 of each sign (``exact_rowk.patterns``), (mu, d), mu an
integer in [-4, 4], d in {1, 2, 4}, different per token and identity; dims no identity reads hold +-48.  So sum = 512 mu and the
squared deviations 512 d^2, all partial sums integers below 2^13: mean = mu, var = d^2 exactly, and the true normalised value is e.
ln_w is a power of two per feature (1/2, 1, 2), ln_b an integer of alternating sign and magnitude 3 .. 6 (never cancelled by |e w| <=
2), pos integers |p| <= 32 that differ between neighbouring tokens and features: the LayerNorm output e w + b is a multiple of 1/2
of at most 8 (5 significant bits: its nearest bf16 rounding boundary is 2^-9 |y| away, the two ulps of rsqrtf 2^-22), + pos a
multiple of 1/2 of at most 40 (7 bits; with eps = 3 multiples of 1/4: 6 and 8 bits): ``emulate_scores`` restates the kernel's fp32
expression with rstd +- 2 ulps and must give the same bf16.  eps = 0 (rstd = 1 / d), or eps = 3 with d = 1 (rstd = 1/2: a wrong eps is wrong by a factor).  With the one-hot keys
every (face token, head, K-step) of the operand map and every 16-byte chunk of the LDS stage's XOR swizzle carries an entry whose
(e, w, b, pos) identify it (``scores_key_steps``: all four K-steps and all sixteen swizzle rows are hit).

ROUTER HEAD (``HEAD_CASES``).  x integers, w = +-q (q = 1, or 1/4), b = 3 q: every product is a multiple of q of at most 64 q, sums
below 1024 * 64 q: exact; z = x . w + b is a bf16 number.  "classes": z in {0} u [17, 200] u [-200, -100], where the kernel returns
0.5, 1 (fp32 1 + exp(-17) = 1) and 0 (__expf(100) = inf) and so does bf16(fp64 sigmoid): 1 - 4e-8 rounds to 1 and 4e-44 to 0 (bf16's
smallest subnormal is 9e-41; -92 would still hold one); the class of (n, id) is a seeded function of both, all three appear for
every identity.  "quarters": z multiples of 1/4 in [-8, 8] under the window rule.

MASKED COMBINE / ROUTED MIX (``MIX_CASES``).  r in {0, 1/4, 1/2, 1}; af entries in {0, 1/2, 1} with row sums <= 1, a different
matrix per sample; feat integers in [-8, 8]; x integers in [-16, 16]; alpha in {1, 1/2}.  av = af r is a multiple of 1/8 of at most
1, 1 - av too; the product chain of the three- and four-stream audio weights is exact where it stays a multiple of 1/8: tokens
where it does not are drawn again from r in {0, 1/2, 1}, then {0, 1} (av a multiple of 1/2: every product a power of two).  With
all weights multiples of 1/8 the mix is a multiple of 1/8 of at most 4 * 8 = 32: at most 256 units, a bf16 number, and so are alpha
times it and (routed_mix) the fp32 weight sum.  ``mix_weights`` asserts all of it; the fp64 definition, rounded once at the end, is
therefore the reference whatever the kernel's rounding points.

FORCING MAXIMUM, PATCHIFY: pure selection / data movement; the patch elements are a running int16 counter seen as bf16.

ACTIVATION + ADD (``ACT_*``).  x = k 2^-4, |k| <= 160; none / relu / leaky_relu: the fp32 expression rounded once; SiLU: the window
rule (|x| <= 10); both GELUs: ``ACT_ULPS`` of test_gemm_exact_gpu.py under that test's rule (same device functions).  With a residual
the result must equal bf16(bf16(act) + r) of the kernel's own activation-only output, bit for bit.

CFG + SCHEDULER STEP: oracle.scheduler's expression-by-expression restatement, bit for bit, at a size that takes the grid-stride
loop round twice.
"""
import math

import numpy as np
import torch

import exact_norm as xn
import exact_rowk as xr
from exact_gemm import BF, POISON, SENTINEL, GuardedOut, assert_exact, bad_elements, describe, exact_epilogue, exact_operands, pow2  # noqa: F401  (re-exported)
from exact_vae import SILU_WINDOW, is_sentinel, sentinel, silu64, ulp_distance  # noqa: F401  (re-exported)

WINDOW_CAP = 0.02


def seed_of(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def exact_bf(t):
    r = t.to(BF)
    assert torch.equal(r.double(), t.double()), "a value is not a bf16 number"
    return r.contiguous()


def guarded(shape, dev, dtype=BF, before=24, after=40):
    """A contiguous, poisoned output of ``shape`` in the middle of a 1-D sentinel buffer -> (view, buffer, mask of the rest).
    bf16 / int16: POISON inside, SENTINEL outside; fp32: NaN inside, -7777.0 outside.  (``before`` * itemsize is a multiple of 16.)"""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        buf = torch.full((before + n + after,), -7777.0, dtype=dtype, device=dev)
        buf[before:before + n] = float("nan")
    else:
        buf = torch.full((before + n + after,), SENTINEL, dtype=torch.int16, device=dev)
        buf[before:before + n] = POISON
        buf = buf.view(dtype)
    rest = torch.ones(buf.shape, dtype=torch.bool, device=dev)
    rest[before:before + n] = False
    return buf[before:before + n].view(shape), buf, rest


def guard_intact(buf, rest):
    if buf.dtype == torch.float32:
        return bool((buf[rest] == -7777.0).all())
    return bool((buf.view(torch.int16)[rest] == SENTINEL).all())


def first_bad(bad):
    """Index tuple of the first bad element (``bad`` must have one)."""
    return tuple(int(v) for v in bad.nonzero()[0])


def window_share(ref64):
    """Share of the elements whose fp64 value lies within ``SILU_WINDOW`` relative of a bf16 rounding boundary."""
    return float((xn.boundary_distance(ref64) < SILU_WINDOW).double().mean())


def window_check(got, ref64):
    """The window rule -> (mask of the elements that break it, share inside the window, worst distance in ulps)."""
    ref = ref64.to(BF)
    ulps = ulp_distance(got, ref)
    ulps = torch.where(bad_elements(got, ref), ulps, torch.zeros_like(ulps))          # +0 and -0 are equal
    inside = xn.boundary_distance(ref64) < SILU_WINDOW
    wrong = (ulps > 1) | ((ulps != 0) & ~inside)
    return wrong, float(inside.double().mean()), int(ulps.max())


def sigmoid64(z):
    return 1.0 / (1.0 + torch.exp(-z))


# ------------------------------------------------------------------------------------------------------------ small-M linear
LIN_MS, LIN_NS, LIN_KS = (1, 2, 3, 5, 8), (5, 1027), (8, 504, 520, 1280, 3072)


def _lin(M, N, K, bias, kind="plain"):
    return dict(name=f"{kind}-m{M}-n{N}-k{K}-{'bias' if bias else 'nobias'}", M=M, N=N, K=K, bias=bias, kind=kind)


# the full product of rows, columns and K; the bias alternates so that each instantiation meets each K with and without one
LIN_CASES = [_lin(M, N, K, bool((im + jn + kk) % 2)) for im, M in enumerate(LIN_MS) for jn, N in enumerate(LIN_NS) for kk, K in enumerate(LIN_KS)]
LIN_SILU_IN_CASES = [_lin(2, 5, 1280, True, "siluin"), _lin(5, 1027, 3072, True, "siluin"), _lin(8, 5, 520, False, "siluin")]
LIN_SILU_OUT_CASES = [_lin(1, 1027, 1280, True, "siluout"), _lin(8, 1027, 1280, False, "siluout"), _lin(5, 5, 3072, True, "siluout")]
ALL_LIN_CASES = LIN_CASES + LIN_SILU_IN_CASES + LIN_SILU_OUT_CASES
SILU_OUT_SCALE = 2.0 ** -6


def lin_plan(c):
    """The plan bya_linear_small_m_plan must return for case ``c``."""
    return dict(kernel=2 if c["M"] <= 2 else 8, grid=(c["N"] + 3) // 4, rounds=(c["K"] + 511) // 512, items=c["N"], items_per_round=512)


def lin_lanes(K):
    """(lanes with work, pieces of lane 0, lanes that hold the largest piece count)."""
    pieces = [len(range(8 * lane, K, 512)) for lane in range(64)]
    return sum(p > 0 for p in pieces), pieces[0], sum(p == pieces[0] for p in pieces)


def _lin_draw(c, seed):
    M, N, K = c["M"], c["N"], c["K"]
    if c["kind"] == "siluin":
        g = torch.Generator().manual_seed(seed)
        x = torch.tensor([0.0, 32.0, 64.0, -128.0])[torch.randint(0, 4, (M, K), generator=g)].to(BF)
        _, w = exact_operands(M, N, K, "cpu", seed=seed + 1)
    else:
        x, w = exact_operands(M, N, K, "cpu", seed=seed)
        if c["kind"] == "siluout":
            x = exact_bf(x.double() * SILU_OUT_SCALE)
    bias = exact_epilogue(w, "cpu", seed + 7, bias=True)["bias"] if c["bias"] else None
    if bias is not None and c["kind"] == "siluout":
        bias = exact_bf(bias.double() * SILU_OUT_SCALE)
    return dict(x=x.contiguous(), w=w.contiguous(), bias=bias, seed=seed)


def lin_pre(c, dat, dev="cpu", fault=None):
    """The definition in fp64: f(x) @ w.T + bias, f = bf16(SiLU) for the silu_in cases, before any output activation.  ``fault`` = (m,
    n, lane): that lane's LAST 16-byte piece is lost for output (m, n)."""
    x = dat["x"].to(dev).double()
    if c["kind"] == "siluin":
        x = silu64(x).to(BF).double()
    w = dat["w"].to(dev).double()
    y = x @ w.T
    if fault is not None:
        m, n, lane = fault
        k0 = list(range(8 * lane, c["K"], 512))[-1]
        y[m, n] -= (x[m, k0:k0 + 8] * w[n, k0:k0 + 8]).sum()
    if dat["bias"] is not None:
        y = y + dat["bias"].to(dev).double()
    return y


def lin_data(c):
    """The tensors of linear case ``c`` (CPU) -> dict(x [M, K], w [N, K], bias [N] or None).  act_out = SiLU: the first seed with at
    most 2 % of the outputs in the rounding-boundary window."""
    for attempt in range(50):
        dat = _lin_draw(c, seed_of(c["name"]) + 1009 * attempt)
        if c["kind"] != "siluout" or window_share(silu64(lin_pre(c, dat))) <= WINDOW_CAP:
            return dat
    raise AssertionError(f"{c['name']}: no data with at most 2 % of its outputs in the SiLU window")


def lin_units(c):
    """(unit of x after f, unit of w, unit of the bias): the grids the operands are built on."""
    if c["kind"] == "siluin":
        return 32.0, 0.5, 0.25
    scale = SILU_OUT_SCALE if c["kind"] == "siluout" else 1.0
    return 0.5 * scale, 0.5, 0.25 * scale


def lin_bound(c, dat):
    """(largest |partial sum| in units of the product grid, largest |value before the rounding| in units of the finer of that grid and
    the bias's): both must be < 2^24.  Asserts that every operand is on its grid."""
    x = dat["x"].double()
    if c["kind"] == "siluin":
        x = silu64(x).to(BF).double()
    w = dat["w"].double()
    ux, uw, ub = lin_units(c)
    for t, u in ((x, ux), (w, uw)) + (((dat["bias"].double(), ub),) if dat["bias"] is not None else ()):
        assert torch.equal(t / u, torch.round(t / u)), "an operand is off its grid"
    acc = c["K"] * float(x.abs().max()) * float(w.abs().max()) / (ux * uw)
    total = acc
    if dat["bias"] is not None:
        fine = min(ux * uw, ub)
        total = (acc * ux * uw + float(dat["bias"].double().abs().max())) / fine
    return acc, total


def describe_lin(c, bad, got, ref):
    m, n = first_bad(bad)
    lanes, p0, full = lin_lanes(c["K"])
    return (f"{c['name']}: {int(bad.sum())} of {bad.numel()} outputs differ; first: row {m}, column {n} (workgroup {n // 4}, wave {n % 4}; {lanes} lanes "
            f"with work, lanes 0..{full - 1} take {p0} pieces): got {float(got[m, n])!r}, want {float(ref[m, n])!r}")


# ------------------------------------------------------------------------------------------------------------ timestep features
TS_EXACT_CASES = [(flip, dim) for flip in (0, 1) for dim in (6, 3072)]                      # t = 0, batch 3
TS_BOUND_CASES = [(1, 0.0, 3072), (0, 0.0, 3072), (1, 1.0, 3072), (0, 1.0, 3072), (1, 1.0, 6), (0, 0.0, 6)]      # (flip, shift, dim)
TS_VALUES = (1, 500, 999)
TS_OLD_BAR = 1.2e-2


def ts_reference(t, dim, flip, shift):
    """fp64 sin / cos of t exp(-ln(10000) j / (half - shift)) -> (reference [B, dim], angle [B, half], exponent [half])."""
    half = dim // 2
    expo = -math.log(10000.0) * torch.arange(half, dtype=torch.float64) / (half - shift)
    ang = t.double()[:, None] * torch.exp(expo)[None]
    s, c = torch.sin(ang), torch.cos(ang)
    return (torch.cat([c, s], 1) if flip else torch.cat([s, c], 1)), ang, expo


def angle_budget(ang, expo):
    """|d angle| <= angle (5 |expo| + 3) 2^-24 (module docstring), fp64 [B, half]."""
    return ang.abs() * (5.0 * expo.abs()[None] + 3.0) * 2.0 ** -24


def ts_bound(ref, ang, expo):
    """The derived bound per element [B, dim]: half a bf16 ulp of (|ref| + budget) + budget, budget = angle budget + 4 * 2^-24."""
    bud = angle_budget(ang, expo) + 4.0 * 2.0 ** -24
    bud = torch.cat([bud, bud], 1)
    mag = (ref.abs() + bud).clamp(2.0 ** -126, 1.0 - 2.0 ** -30)                 # |sinf|, |cosf| <= 1: the binade below 1 at most
    half_ulp = torch.exp2(torch.floor(torch.log2(mag)) - 8)
    return half_ulp + bud


# ------------------------------------------------------------------------------------------------------------ router scores
R_HEADS, R_TOK, R_HD = 16, 32, 128
R_QK, R_FEAT = R_HEADS * R_HD, R_HEADS * R_TOK
JUNK = 48.0


def _scores(name, n_id, N, kernel, eps=0.0, wave_form=False):
    return dict(name=name, n_id=n_id, N=N, kernel=kernel, eps=eps, wave_form=wave_form)


# (3, 4090): the last N of the wave kernel; (3, 4099) / (4, 4112): 255 / 256 workgroups of the LDS kernel, ragged / whole last tile
SCORES_CASES = [
    _scores("wave-2x150", 2, 150, "wave"),
    _scores("wave-2x150-eps3", 2, 150, "wave", eps=3.0),
    _scores("wave-3x4090", 3, 4090, "wave"),
    _scores("lds-3x4099", 3, 4099, "lds"),
    _scores("lds-4x4112", 4, 4112, "lds"),
    _scores("waveform-3x4099", 3, 4099, "wave", wave_form=True),
]
SCORES_OLD_BAR = 2e-3


def scores_plan(c):
    """The plan bya_router_scores_plan must return for case ``c``."""
    tiles = (c["N"] + 15) // 16
    if c["kernel"] == "lds":
        grid = 256 // c["n_id"] * c["n_id"]
        per = grid // c["n_id"] * 8
        return dict(kernel="lds", grid=grid, rounds=(tiles + per - 1) // per, items=tiles, items_per_round=per)
    return dict(kernel="wave", grid=(tiles * c["n_id"] + 3) // 4, rounds=1, items=tiles, items_per_round=tiles)


def scores_data(c):
    """The tensors of scores case ``c`` (CPU) -> dict: qr [N, 2048], kr [n_id, 32, 2048], ln_w, ln_b [512], pos [N, 512] bf16; the
    closed form's e [n_id, N, 512] (int8), mu, d [n_id, N], perm [16, 128] and the dims read ``src`` [n_id, 512] (feature order)."""
    n_id, N = c["n_id"], c["N"]
    rng = np.random.RandomState(seed_of(c["name"].replace("waveform", "lds")))       # the reference form runs the LDS case's data
    perm = np.stack([rng.permutation(R_HD) for _ in range(R_HEADS)])                # [h, 128]
    f = np.arange(R_FEAT)
    tok, h = f // R_HEADS, f % R_HEADS
    src = np.stack([h * R_HD + perm[h, R_TOK * i + tok] for i in range(n_id)])       # [n_id, 512]: column of qr behind feature f
    kr = torch.zeros(n_id, R_TOK, R_QK)
    for i in range(n_id):
        kr[i, torch.from_numpy(tok), torch.from_numpy(src[i])] = 1.0
    pool = xr.patterns(64, rng).numpy().astype(np.int8)                               # [64, 512]: sum 0, 256 of each sign
    n = np.arange(N)
    idx = (n[None] * 5 + 17 * np.arange(n_id)[:, None] + n[None] // 64) % 64          # [n_id, N]
    e = pool[idx]                                                                     # [n_id, N, 512]
    pairs = np.array([(m, dd) for m in range(-4, 5) for dd in (1, 2, 4)])
    pick = np.stack([rng.permutation(len(pairs))[:n_id] for _ in range(N)], 1)        # different pairs for one token's identities
    mu, d = pairs[pick, 0], pairs[pick, 1]
    if c["eps"]:
        d = np.ones_like(d)
    qr = rng.choice([-JUNK, JUNK], (N, R_QK))
    for i in range(n_id):
        qr[:, src[i]] = mu[i][:, None] + d[i][:, None] * e[i]
    sign = np.where(f % 2 == 0, 1.0, -1.0)
    ln_w = rng.choice([0.5, 1.0, 2.0], R_FEAT)
    ln_b = sign * rng.randint(3, 7, R_FEAT)
    pos = rng.randint(-32, 33, (N, R_FEAT)).astype(np.float64)
    same = (pos[1:] == pos[:-1])
    pos[1:][same] += np.where(pos[1:][same] < 32, 1, -1)                              # neighbouring tokens differ
    tb = lambda a: exact_bf(torch.from_numpy(np.ascontiguousarray(a)).double())
    return dict(qr=tb(qr), kr=exact_bf(kr), ln_w=tb(ln_w), ln_b=tb(ln_b), pos=tb(pos), e=torch.from_numpy(e), mu=torch.from_numpy(mu),
                d=torch.from_numpy(d), perm=perm, src=src, k=0.5 if c["eps"] else 1.0)


def scores_closed_form(dat):
    """e k w + b + pos, fp64 [n_id, N, 512]: what the definition gives on this data."""
    return dat["e"].double() * dat["k"] * dat["ln_w"].double() + dat["ln_b"].double() + dat["pos"].double()[None]


def scores_raw(dat, dev="cpu"):
    """s[id, n, 16 tok + h] = sum_d qr[n, 128 h + d] kr[id, tok, 128 h + d] in fp64 (the definition, by matrix products)."""
    N = dat["qr"].shape[0]
    n_id = dat["kr"].shape[0]
    qh = dat["qr"].to(dev).double().view(N, R_HEADS, R_HD).transpose(0, 1)                       # [16, N, 128]
    kh = dat["kr"].to(dev).double().view(n_id, R_TOK, R_HEADS, R_HD).permute(0, 2, 3, 1)          # [id, 16, 128, 32]
    s = qh[None] @ kh                                                                            # [id, 16, N, 32]
    return s.permute(0, 2, 3, 1).reshape(n_id, N, R_FEAT)


def scores_finish(s, dat, eps, dev="cpu"):
    """LayerNorm(512) in fp64, rounded to bf16 (the LayerNorm's output dtype), + pos -> fp64 [n_id, N, 512] (round with .to(bf16))."""
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    y = (s - mean) / torch.sqrt(var + eps) * dat["ln_w"].to(dev).double() + dat["ln_b"].to(dev).double()
    return y.to(BF).double() + dat["pos"].to(dev).double()[None]


def scores_reference(c, dat, dev="cpu", eps=None):
    return scores_finish(scores_raw(dat, dev), dat, c["eps"] if eps is None else eps, dev)


def scores_key_steps(dat):
    """For every identity: the set of (K-step, swizzle row r & 15, LDS chunk) its one-hot entries fall into -> (K-steps hit per
    (identity, head), swizzle rows hit, distinct 16-byte chunks hit per identity)."""
    n_id = dat["src"].shape[0]
    f = np.arange(R_FEAT)
    tok, h = f // R_HEADS, f % R_HEADS
    steps, rows, chunks = set(), set(), []
    for i in range(n_id):
        p = dat["src"][i] - h * R_HD                                  # position inside the head
        ks, grp = p // 32, p % 32 // 8
        steps |= {(i, int(a), int(b)) for a, b in zip(h, ks)}
        rows |= {(i, int(t) & 15, int(b)) for t, b in zip(tok, ks)}
        chunks.append(len({(int(t), int(16 * hh + 4 * a + g)) for t, hh, a, g in zip(tok, h, ks, grp)}))
    return steps, rows, chunks


def emulate_scores(dat, ulps):
    """The kernel's fp32 expression (acc - mean) * rstd * w + b, rstd = the true one moved by ``ulps`` ulps, on every (d, e, feature)
    -> (bf16 [3, 2, 512], the closed form's bf16 [3, 2, 512]); then + pos is exact (asserted by the caller)."""
    d = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64)[:, None, None]
    e = torch.tensor([-1.0, 1.0], dtype=torch.float64)[None, :, None]
    k = dat["k"]
    if k != 1.0:
        d = d[:1]
    true_rstd = (k / d).float()
    w, b = dat["ln_w"].double()[None, None], dat["ln_b"].double()[None, None]
    t = xn.f32(xn.f32((d * e) * xn.move_ulps(true_rstd, ulps).double()) * w)            # (w is a power of two: exact)
    return xn.f32(t + b).to(BF), (e * k * w + b).expand(d.shape[0], 2, R_FEAT).to(BF)


def scores_fault_swap(s, tile, ident, head, tok_a, tok_b):
    """Planted: the wave of ``tile`` of identity ``ident`` swaps face tokens a and b inside one head."""
    s = s.clone()
    rows = slice(16 * tile, 16 * tile + 16)
    fa, fb = 16 * tok_a + head, 16 * tok_b + head
    s[ident, rows, fa], s[ident, rows, fb] = s[ident, rows, fb].clone(), s[ident, rows, fa].clone()
    return s


def scores_fault_kstep(s, dat, tile, ident, head, kstep):
    """Planted: the wave of ``tile`` of identity ``ident`` drops K-step ``kstep`` of one head (those products never reach the sum)."""
    s = s.clone()
    f = np.arange(R_FEAT)
    p = dat["src"][ident] - (f % R_HEADS) * R_HD
    hit = torch.from_numpy((f % R_HEADS == head) & (p // 32 == kstep))
    assert int(hit.sum()) > 0
    s[ident, 16 * tile:16 * tile + 16][:, hit] = 0.0
    return s


def describe_scores(c, bad, got, ref):
    i, n, f = first_bad(bad)
    tok, h, tile = f // 16, f % 16, n // 16
    where = f"wave-kernel wave {i * ((c['N'] + 15) // 16) + tile}"
    if c["kernel"] == "lds":
        per = 256 // c["n_id"]
        where = f"LDS-kernel workgroup {(tile // 8) % per * c['n_id'] + i} wave {tile % 8} round {tile // (8 * per)}"
    return (f"{c['name']}: {int(bad.sum())} of {bad.numel()} elements differ; first: identity {i}, token {n}, feature {f} = face token {tok} head {h} "
            f"(tile {tile}, {where}, lane {n % 16 + 16 * (tok % 16 // 4)}, accumulator [{h}][{tok // 16}][{tok % 4}]): got {float(got[i, n, f])!r}, "
            f"want {float(ref[i, n, f])!r}")


# ------------------------------------------------------------------------------------------------------------ router head
def _head(kind, n_id, N, D):
    return dict(name=f"{kind}-{n_id}x{N}x{D}", kind=kind, n_id=n_id, N=N, D=D)


HEAD_SHAPES = [(2, 701, 512), (3, 333, 1024), (4, 5, 512)]       # D = 1024: the second trip of the K loop; rows % 4 != 0
HEAD_CASES = [_head(kind, *s) for kind in ("classes", "quarters") for s in HEAD_SHAPES]
HEAD_OLD_BAR = 2e-3


def _head_draw(c, seed):
    n_id, N, D = c["n_id"], c["N"], c["D"]
    rng = np.random.RandomState(seed)
    q = 1.0 if c["kind"] == "classes" else 0.25
    w = rng.choice([-1, 1], D)
    n, i = np.meshgrid(np.arange(N), np.arange(n_id))                                  # [n_id, N]
    if c["kind"] == "classes":
        cls = (n * 7 + i * 5 + n // 3 + (n * i) % 4) % 3
        if N * n_id >= 3 * n_id:
            cls[:, :3] = (np.arange(3)[None] + np.arange(n_id)[:, None]) % 3          # all three classes for every identity
        z = np.where(cls == 0, 0, np.where(cls == 1, rng.randint(17, 201, (n_id, N)), -rng.randint(100, 201, (n_id, N))))
    else:
        cls = None
        z = rng.randint(-32, 33, (n_id, N))                                           # in units of 1/4
    target = z - 3                                                                    # b = 3 q
    x = rng.randint(-2, 3, (n_id, N, D))
    corr = target - (x * w).sum(-1)                                                   # spread over eight seeded columns
    cols = np.stack([rng.permutation(D)[:8] for _ in range(n_id * N)]).reshape(n_id, N, 8)
    share = corr[..., None] // 8 + (np.arange(8) < (corr[..., None] % 8))
    np.put_along_axis(x, cols, np.take_along_axis(x, cols, -1) + share * w[cols], -1)
    assert ((x * w).sum(-1) == target).all() and np.abs(x).max() <= 64
    return dict(x=exact_bf(torch.from_numpy(x).double()), w=exact_bf(torch.from_numpy(w * q).double()), b=exact_bf(torch.tensor([3 * q]).double()),
                z=torch.from_numpy(z * q).double(), cls=cls, seed=seed)


def head_data(c):
    """The tensors of head case ``c`` (CPU) -> dict: x [n_id, N, D], w [D], b [1] bf16, the exact z [n_id, N], cls (classes)."""
    for attempt in range(50):
        dat = _head_draw(c, seed_of(c["name"]) + 1009 * attempt)
        if c["kind"] == "classes" or window_share(sigmoid64(dat["z"])) <= WINDOW_CAP:
            return dat
    raise AssertionError(f"{c['name']}: no data with at most 2 % of its outputs in the window")


def head_reference(dat, dev="cpu"):
    """sigmoid(bf16(x . w + b)) in fp64, in the [N, n_id] layout."""
    z = dat["x"].to(dev).double() @ dat["w"].to(dev).double() + dat["b"].to(dev).double()
    return sigmoid64(z.to(BF).double()).T.contiguous()


def describe_head(c, bad, got, ref):
    n, i = first_bad(bad)
    row = i * c["N"] + n
    return (f"{c['name']}: {int(bad.sum())} of {bad.numel()} elements differ; first: token {n}, identity {i} (input row {row}: workgroup {row // 4}, wave "
            f"{row % 4}; {c['D'] // 512} trip(s) of the K loop): got {float(got[n, i])!r}, want {float(ref[n, i])!r}")


# ------------------------------------------------------------------------------------------------------------ masked combine / routed mix
def _mix(mode, n_id, D, N, bcast, alpha=1.0):
    return dict(name=f"{mode}-id{n_id}-d{D}-n{N}-{'shared' if bcast else 'persample'}-a{alpha:g}", mode=mode, n_id=n_id, D=D, N=N, bcast=bcast,
                alpha=alpha, B=2)


# B N D / 8 = 666 and 4810 threads: no multiple of 256, three and nineteen workgroups
MIX_CASES = ([_mix(mode, n_id, *((8, 333, True) if (n_id + k) % 2 else (520, 37, False)), alpha=(1.0, 0.5)[k])
              for mode, ids in (("face", (1, 2, 3, 4)), ("audio", (2, 3, 4))) for n_id in ids for k in (0, 1)]
             + [_mix("audio", 2, 8, 333, False), _mix("audio", 4, 520, 37, True, 0.5), _mix("face", 3, 8, 333, False, 0.5)])
R_TIERS = ([0.0, 0.25, 0.5, 1.0], [0.0, 0.5, 1.0], [0.0, 1.0])


def mix_weights(mode, r, af, check=True):
    """The routing weights of the DEFINITION in fp64 (include/bya.h): face w = r; audio av = af r, w[a] = prod_{b != a} (1 - av[b]).
    r [B, N, n_id], af [B, n_id, n_id] -> w [B, N, n_id].  ``check``: every intermediate is a bf16 number and every weight a
    multiple of 1/8 (so no rounding point of the kernel rounds)."""
    if mode == "face":
        return r.clone()
    n_id = r.shape[-1]
    av = torch.einsum("bai,bni->bna", af, r)
    om = 1.0 - av
    w = torch.ones_like(r)
    for a in range(n_id):
        for b in range(n_id):
            if b != a:
                w[..., a] = w[..., a] * om[..., b]
                if check:
                    exact_bf(w[..., a])
    if check:
        exact_bf(av), exact_bf(om)
        assert torch.equal(w * 8, torch.round(w * 8)), "a weight is no multiple of 1/8"
    return w


def mix_data(c):
    """The tensors of mix case ``c`` (CPU) -> dict: feat [B, n_id, N, D], r [B or 1, N, n_id], af [B, n_id, n_id] or None, x [B, N, D]
    bf16, and the share of tokens drawn again per tier."""
    B, n_id, N, D = c["B"], c["n_id"], c["N"], c["D"]
    rng = np.random.RandomState(seed_of(c["name"]))
    Br = 1 if c["bcast"] else B
    af = None
    if c["mode"] == "audio":
        rows = [v for v in np.stack(np.meshgrid(*[[0.0, 0.5, 1.0]] * n_id), -1).reshape(-1, n_id) if 0 < v.sum() <= 1]
        for _ in range(100):
            af = np.stack([[rows[rng.randint(len(rows))] for _ in range(n_id)] for _ in range(B)])
            if not (af[0] == af[1]).all() and (af == 0.5).any():
                break
        af = torch.from_numpy(af).double()
    r = torch.from_numpy(rng.choice(R_TIERS[0], (Br, N, n_id))).double()
    redrawn = []
    if c["mode"] == "audio":
        for tier in R_TIERS[1:]:
            w = mix_weights("audio", r.expand(B, N, n_id), af, check=False)
            ok = (w.to(BF).double() == w) & (w * 8 == torch.round(w * 8))
            # (intermediates of the chain: checked in full by mix_weights(check=True) once the draw is final)
            bad = ~ok.all(-1).all(0) if c["bcast"] else ~ok.all(-1)
            bad = bad.reshape(Br, N)
            redrawn.append(float(bad.double().mean()))
            r[bad] = torch.from_numpy(rng.choice(tier, (int(bad.sum()), n_id))).double()
    feat = torch.from_numpy(rng.randint(-8, 9, (B, n_id, N, D))).double()
    x = torch.from_numpy(rng.randint(-16, 17, (B, N, D))).double()
    return dict(feat=exact_bf(feat), r=exact_bf(r), af=None if af is None else exact_bf(af), x=exact_bf(x), redrawn=redrawn)


def mix_reference(c, dat, dev="cpu", af_of_sample0=False):
    """-> (z fp64 [B, N, D] = sum_id w feat, wsum fp64 [B, N], combined fp64 [B, N, D] = x + alpha z).  ``af_of_sample0``: the planted
    fault -- every sample takes sample 0's af."""
    B, N, n_id = c["B"], c["N"], c["n_id"]
    r = dat["r"].to(dev).double().expand(B, N, n_id)
    af = None if dat["af"] is None else dat["af"].to(dev).double()
    if af is not None and af_of_sample0:
        af = af[:1].expand(B, n_id, n_id)
    w = mix_weights(c["mode"], r, af, check=not af_of_sample0)
    z = torch.einsum("bni,bind->bnd", w, dat["feat"].to(dev).double())
    return z, w.sum(-1), dat["x"].to(dev).double() + c["alpha"] * z


def describe_mix(c, bad, got, ref):
    b, n, ch = first_bad(bad)
    gid = (b * c["N"] + n) * (c["D"] // 8) + ch // 8
    return (f"{c['name']}: {int(bad.sum())} of {bad.numel()} elements differ; first: sample {b}, token {n}, channel {ch} (thread {gid}: workgroup "
            f"{gid // 256}, wave {gid % 256 // 64}, lane {gid % 64}): got {float(got[b, n, ch])!r}, want {float(ref[b, n, ch])!r}")


# ------------------------------------------------------------------------------------------------------------ forcing maximum
FORCING_CASES = [(1, 100, 3), (13, 171, 3), (13, 54, 2), (13, 300, 4)]          # (frames, per_frame, n_id): 300, 513, 108, 1200 columns
FORCING_VALUES = [-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, 2.5]


def forcing_data(frames, per_frame, n_id):
    """-> (f [frames, per_frame, n_id] bf16 with ties, the frame of the maximum per column int64 [per_frame, n_id])."""
    g = torch.Generator().manual_seed(frames * 1000 + per_frame * 10 + n_id)
    f = torch.tensor(FORCING_VALUES)[torch.randint(0, len(FORCING_VALUES), (frames, per_frame, n_id), generator=g)]
    col = torch.arange(per_frame * n_id).view(per_frame, n_id)
    at = torch.tensor([0, frames // 2, frames - 1])[col % 3]
    top = torch.tensor([2.5, 3.0, 7.0])[(col // 3) % 3]                        # 2.5 ties with the background: the first one must win
    if frames > 1:
        f.scatter_(0, at[None], top[None])
    return f.to(BF), at


# ------------------------------------------------------------------------------------------------------------ patchify
PATCH_SHAPES = [(3, 1, 1, 2, 2), (2, 3, 5, 6, 10)]                              # (B, T, C, H, W)


def counter(shape, start):
    """A running int16 counter (every element distinct; NaN and infinity patterns included: these kernels only move bits)."""
    n = int(np.prod(shape))
    assert n < 65536
    return ((torch.arange(n, dtype=torch.int32) * 37 + start) % 65536 - 32768).to(torch.int16).view(shape)


def patchify_reference(x):
    B, T, C, H, W = x.shape
    return x.view(B, T, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, T * (H // 2) * (W // 2), C * 4)


def unpatchify_reference(y, shape):
    B, T, C, H, W = shape
    return y.reshape(B, T, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, T, C, H, W)


# ------------------------------------------------------------------------------------------------------------ activation + add
ACTS = ("none", "gelu_tanh", "gelu_erf", "relu", "silu", "leaky_relu")
ACT_SMALL_N = 8 * (3 * 256 + 5)                               # four workgroups, the last one ragged
ACT_LARGE_N = 3 * 4096 * 256 * 8 // 2 + 808                   # 1.5 rounds of the 4096-workgroup grid and a ragged remainder
ACT_LARGE_CASES = [("silu", True, True), ("gelu_erf", False, False), ("none", True, False), ("leaky_relu", False, True)]      # (act, residual, in place)


def act_plan(n):
    nvec = n // 8
    grid = min(4096, (nvec + 255) // 256)
    return dict(kernel="act_add", grid=grid, rounds=(nvec + grid * 256 - 1) // (grid * 256), items=nvec, items_per_round=grid * 256)


def act_data(n, dev, seed=3):
    """x = k 2^-4, |k| <= 160; r = j 2^-2, |j| <= 64 (bf16, on ``dev``)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randint(-160, 161, (n,), generator=g, device=dev).float() * 2.0 ** -4
    r = torch.randint(-64, 65, (n,), generator=g, device=dev).float() * 2.0 ** -2
    return x.to(BF), r.to(BF)


def act_fp32(act, x):
    """none / relu / leaky_relu: the kernel's fp32 expression (torch's fp32 arithmetic is the same IEEE arithmetic)."""
    t = x.float()
    if act == "relu":
        return torch.where(t > 0, t, torch.zeros_like(t))
    if act == "leaky_relu":
        return torch.where(t > 0, t, torch.tensor(0.01, dtype=torch.float32, device=t.device) * t)
    return t


def describe_act(n, bad, got, ref):
    i = first_bad(bad)[0]
    p = act_plan(n)
    v = i // 8
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; first: element {i} (piece {v}: round {v // p['items_per_round']}, workgroup "
            f"{v % p['items_per_round'] // 256}, wave {v % 256 // 64}, lane {v % 64}): got {float(got[i])!r}, want {float(ref[i])!r}")


# ------------------------------------------------------------------------------------------------------------ CFG + scheduler step
SCHED_N = 8192 * 256 + 1000
SCHED_PAD = 64                                                 # pred_stride = n + 64: the two predictions are rows of a wider buffer
SCHED_CASES = ["ddim-cfg-strided", "dpm-second-cfg-strided", "dpm-first-nocfg"]


def sched_plan(n):
    grid = min(8192, (n + 255) // 256)
    return dict(kernel="cfg_scheduler_step", grid=grid, rounds=(n + grid * 256 - 1) // (grid * 256), items=n, items_per_round=grid * 256)


def describe_sched(n, bad, got, ref):
    i = first_bad(bad)[0]
    p = sched_plan(n)
    return (f"{int(bad.sum())} of {bad.numel()} elements differ; first: element {i} (round {i // p['items_per_round']}, workgroup "
            f"{i % p['items_per_round'] // 256}, wave {i % 256 // 64}, lane {i % 64}): got {float(got[i])!r}, want {float(ref[i])!r}")
