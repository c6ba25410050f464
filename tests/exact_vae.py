"""Exact-data checking of the video VAE's kernels (a plain helper module: no tests, no fixtures; the sibling of ``exact_gemm.py``,
``exact_attn.py``, ``exact_rowk.py`` and ``exact_norm.py``, whose ``GuardedOut`` / ``bad_elements`` / ``describe`` / ``assert_exact`` /
``pow2`` / ``POISON`` / ``SENTINEL`` and +-1 pattern rows it reuses): bya_vae_conv3d (the CONV instance of gemm_v4.hip with its
epilogue branch of gemm_wide_epilogue.h), bya_vae_upsample_pad, bya_vae_groupnorm_stats, bya_vae_norm_act and bya_vae_patches
(csrc/vae.hip).  Every case has data for which a correct kernel's answer is a function of the data alone; the check is bit equality
with an fp64 reference of the unpadded DEFINITION rounded once (SiLU, which is not exact, has a derived one-ulp bound), outputs
sit inside a sentinel buffer, and a failure names the element, its pixel, its tile and its wave fragment.  The case tables are
module constants: test_vae_exact_cpu.py reasons about them without a GPU.

CONVOLUTION (``conv_data`` / ``conv_reference``).  x[t, h, w, c] = a 2^ra[t, h, w], w[n, tap, c] = b 2^rw[n], a and b integers in
[-3, 3], ra and rw in {-1, 0, 1}; the two context frames are drawn independently of x.  Every product is a multiple of 2^-2 of
magnitude <= 9 * 4 = 36; the longest K here is 27 * 512 = 13824 (above the 12288 exact_gemm.py derived for): 13824 * 36 = 497664
< 2^19, so every partial sum, in any order, is a multiple of 2^-2 below 2^21 units: exact in fp32.  Bias (b 2^-2, |b| <= 16) and
residual (r 2^-3, |r| <= 64) are on ``exact_gemm.exact_epilogue``'s grid: acc + bias is a multiple of 2^-2 below 2^19 + 4, + res a
multiple of 2^-3 below 2^19 + 12 < 2^23 units -- every value before the one rounding to bf16 is exact (``conv_bound``).  The
reference is 27 (or 9) shifted-slice matmuls in fp64 on the device: causal time (the two context frames, or the first frame
twice), zero space padding.  It never touches bya_vae_patches.

GROUPNORM STATISTICS (``stats_data``).  Group g of a chunk [rows, C] is mu_g + d_g e: e = +-1 with exactly half (count odd: one
more than half) of the group's rows * cg entries positive in a seeded order over the WHOLE group -- not balanced per row or per
channel, so a lost row or channel changes both sums; (mu_g, d_g), mu_g an integer in [-8, 8] and d_g in {1, 2}, is a different
pair for every group.  With count even sums[2g] = count mu_g and sums[2g + 1] = count (mu_g^2 + d_g^2).  Every partial sum is an
integer of magnitude <= count * 100 < 2^24 (``stats_bound``; the one large case has C = 32, so count = rows): exact in fp32 in any
order, partials included.

NORM + ACTIVATION (``norm_data``).  ``sums`` is an input, so it holds the exact count mu_g, count (mu_g^2 + d_g^2) of data built the
same way; the correctly rounded fp32 quotients are mu_g and mu_g^2 + d_g^2 (``assert_mean_var``: the library is
built without fast-math, so its fp32 division is IEEE), var = d_g^2 exactly and x - mean = d_g e.  eps = 0 with mixed d (rstd = 1 /
d) or eps = 3 with d = 1 (rstd = 1 / 2: a wrong eps is wrong by a factor).  gamma is a power of two (1/2, 1, 2), beta an integer
of alternating sign per channel and magnitude ceil(k gamma) + 1 .. + 4 (k = d rstd), which e k gamma never cancels.  With
modulation zy is a power of two (1/2, 1, 2) and zb an integer 1 .. 6 with beta's sign, both per (latent row, channel):
y = (e k gamma + beta) zy + zb is a non-zero multiple of 1/8 of at most 22: at most 8 significant bits (asserted), its nearest bf16
rounding boundary 2^-9 |y| away, so the last bits of the device's rsqrtf cannot matter: ``emulate_norm`` restates the kernel in
fp32 with rstd +- 2 ulps and must give the same bf16.  ``sens`` cases (the manner of exact_norm.py): gamma = 1, beta =
+-(2^-8 + delta), delta = ``exact_norm.sens_delta(count)`` < 1 / (4 count): where e and beta agree |y| = 1 + 2^-8 + delta sits delta
above a rounding boundary, the fp32 noise is 256 times smaller, and a variance over count - 1 moves the value below it.
SiLU: the pre-activation p is exact as above (|p| <= 22); the kernel evaluates p / (1 + __expf(-p)) in fp32 and rounds once, so it
may differ from bf16(fp64 SiLU(p)) by at most one bf16 ulp, and only where the fp64 value lies within ``SILU_WINDOW`` = 2^-16
relative of a rounding boundary (about eight times the fp32 noise: x log2(e) rounded at |x| <= 22 costs 2^-20.5 relative, the
division an ulp); at most 2 % of a case's elements may lie in that window, else the grid is drawn again (``norm_data`` takes
the first seed that passes; the CPU test asserts it).
INDEX MAP (``index_data``): gamma = 0, beta = 1, mean 0 and variance 1 make the normalised value exactly 1, so
y = zy[zr] + zb[zr]: zy[r, c] = 1 + r (at most 63 latent rows), zb[r, c] = ((3 r + c) mod 4) / 4: the sum is a bf16 number, different
for neighbouring latent rows and channels.  ``latent_rows`` is nearest resizing in integer arithmetic.

PATCH GATHER (``PATCH_CASES``): pure data movement against torch's unfold, inside a sentinel buffer.
"""
import numpy as np
import torch
import torch.nn.functional as F

import exact_norm as xn
from exact_gemm import BF, POISON, SENTINEL, GuardedOut, assert_exact, bad_elements, describe, exact_epilogue, pow2  # noqa: F401  (re-exported)

GRID = 256                       # workgroups of a full persistent launch (persistent_grid, csrc/gemm_persistent.h)
GN_ROWS = 512                    # rows per block of bya_vae_groupnorm_stats's first pass
GROUPS = 32
SILU_WINDOW = 2.0 ** -16


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def seed_of(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def sentinel(shape, dev):
    """A bf16 tensor filled with ``SENTINEL`` (a NaN payload no arithmetic produces)."""
    t = torch.empty(shape, dtype=torch.int16, device=dev)
    t.fill_(SENTINEL)
    return t.view(BF)


def is_sentinel(t):
    return t.contiguous().view(torch.int16) == SENTINEL


# ------------------------------------------------------------------------------------------------------------ convolution
def _conv(name, C, Cout, KT, To, H, W, cache=False, res=None, up=None):
    return dict(name=name, C=C, Cout=Cout, KT=KT, To=To, H=H, W=W, cache=cache, res=res, up=up)


# res: None / "separate" (its own tensor, ldres != ldc) / "alias" (the output itself).  bias always.
CONV_CASES = [
    # To = 1 without a cache (the first frame is its own context); 289 padded rows: 33 of them in the second tile; conv_out's
    # Cout = 8 with w of exactly 8 rows: the W descriptor clips the other 248 rows of the tile
    _conv("c128-kt3-cout8-m289", 128, 8, 3, 1, 15, 15),
    # 242 padded rows: below one tile; two N tiles, the second 8 wide
    _conv("c256-kt3-cout264-m242", 256, 264, 3, 2, 9, 9, cache=True, res="separate"),
    _conv("c256-kt3-cout128", 256, 128, 3, 3, 5, 21, cache=True, res="alias"),
    _conv("c512-kt3-cout512", 512, 512, 3, 2, 7, 12, cache=True, res="alias"),
    _conv("c512-kt3-cout256-single", 512, 256, 3, 1, 6, 7, res="separate"),
    _conv("c128-kt3-cout128", 128, 128, 3, 2, 13, 10, cache=True),
    _conv("c512-kt1-cout512", 512, 512, 1, 2, 6, 9, res="separate"),
    # 42 row tiles of K = 13824; the last one holds four pixels (10680 mod 256 = 2 Wp + 2 + 4)
    _conv("c512-kt3-cout8-lasttile4", 512, 8, 3, 2, 58, 87, cache=True),
]
# more output tiles than the persistent grid and not a multiple of it: 190 x 2 = 380 tiles on 256 workgroups (XCDs 0-3: 48 tiles,
# workgroups 0-15 of each take two; XCDs 4-7: 47 tiles, workgroups 0-14 take two): the tile walk, the next tile's prefetch under
# the epilogue and the clipped last tiles all happen behind a full round.  48387 mod 256 = 3: the last row tile is all padding.
CONV_MULTI_ROUND = _conv("c128-kt3-cout512-multiround", 128, 512, 3, 3, 125, 125, cache=True, res="alias")
# the up-sampler form: bya_vae_upsample_pad then bya_vae_conv3d(KT = 1); x is [T, H, W, C] before the up-sampling
UP_CASES = [
    _conv("up-c512-tmode0", 512, 512, 1, 2, 4, 5, up=0),
    _conv("up-c256-tmode1", 256, 256, 1, 2, 5, 3, up=1),
    _conv("up-c128-tmode2", 128, 264, 1, 3, 3, 4, up=2),
]
ALL_CONV_CASES = CONV_CASES + [CONV_MULTI_ROUND] + UP_CASES


def conv_bound(c):
    """(largest |partial sum| in units of 2^-2, largest |value before the rounding| in units of 2^-3): both must be < 2^24."""
    K = 9 * c["KT"] * c["C"]
    acc_units = K * 36 * 4
    return acc_units, (acc_units + 16) * 2 + 64


def up_frames(c):
    T, tm = c["To"], c["up"]
    return T if tm == 0 else (2 * T if tm == 1 else 2 * T - 1)


def conv_geometry(c):
    """-> dict(To, H, W of the OUTPUT grid, Hp, Wp, M padded rows, tiles_m, tiles_n, tiles)."""
    To, H, W = (up_frames(c), 2 * c["H"], 2 * c["W"]) if c["up"] is not None else (c["To"], c["H"], c["W"])
    M = To * (H + 2) * (W + 2)
    tm, tn = (M + 255) // 256, (c["Cout"] + 255) // 256
    return dict(To=To, H=H, W=W, Hp=H + 2, Wp=W + 2, M=M, tiles_m=tm, tiles_n=tn, tiles=tm * tn)


def persistent_walk(tiles):
    """Tiles per workgroup under persistent_grid's rule (csrc/gemm_persistent.h: a launch of min(256, tiles rounded up to 8)
    workgroups; XCD x = workgroup % 8 owns a contiguous eighth of the tile order, its workgroups take every (grid / 8)-th tile of
    it) -> (grid, list of tile counts per workgroup)."""
    grid = (tiles + 7) // 8 * 8 if tiles < GRID else GRID
    slots = grid // 8
    counts = []
    for wg in range(grid):
        xcd, slot = wg % 8, wg // 8
        n_x = tiles // 8 + (1 if xcd < tiles % 8 else 0)
        counts.append(max(0, (n_x - slot + slots - 1) // slots))
    assert sum(counts) == tiles
    return grid, counts


def conv_data(c, dev):
    """The tensors of convolution case ``c`` on ``dev`` -> dict: x [T, H, W, C], ctx [2, H, W, C] or None (KT = 3: the cache, or
    None: the first frame twice), w [Cout, 9 KT C], bias [Cout], res fp32 [rows, Cout] or None."""
    seed = seed_of(c["name"])
    T, H, W, C, KT, Cout = c["To"], c["H"], c["W"], c["C"], c["KT"], c["Cout"]

    def pixels(n, s):
        a = torch.randint(-3, 4, (n, H, W, C), generator=_gen(dev, s), device=dev).float()
        return (a * pow2((n, H, W, 1), dev, s + 1)).to(BF)

    x = pixels(T, seed)
    ctx = pixels(2, seed + 2) if c["cache"] else None
    K = 9 * KT * C
    w = (torch.randint(-3, 4, (Cout, K), generator=_gen(dev, seed + 4), device=dev).float() * pow2((Cout, 1), dev, seed + 5)).to(BF)
    g = conv_geometry(c)
    rows = g["To"] * g["H"] * g["W"]
    ep = exact_epilogue(w, dev, seed + 6, bias=True, res_rows=rows if c["res"] else None)
    return dict(x=x, ctx=ctx, w=w, bias=ep["bias"], res=None if ep["res"] is None else ep["res"][0].to(BF))


def upsample_reference(x, tmode):
    """Nearest up-sampling by ``repeat_interleave``: space x 2; time: 0 as it is, 1 every frame doubled, 2 the first frame single."""
    t = x if tmode == 0 else (x.repeat_interleave(2, 0) if tmode == 1 else torch.cat([x[:1], x[1:].repeat_interleave(2, 0)], 0))
    return t.repeat_interleave(2, 1).repeat_interleave(2, 2)


def conv_reference(x, ctx, w, bias, res, KT, fault=None):
    """The definition in fp64 on x's device: y[t, h, w, n] = bias[n] + res + sum over taps (dt, dh, dw) and c of
    xe[t + dt, h + dh - 1, w + dw - 1, c] w[n, tap, c], xe = [context | x] in time (KT = 3: ``ctx``, or the first frame twice), zero
    outside the frame.  -> fp64 [To * H * W, Cout].  ``fault`` = (tap, channel group of 64, mask of pixels [To, H, W]): the planted
    fault -- those pixels read that tap's channel group one pixel to the right (dw + 1)."""
    To, H, W, C = x.shape
    if KT == 3:
        xe = torch.cat([ctx if ctx is not None else x[:1].expand(2, H, W, C), x], 0)
    else:
        xe = x
    xp = F.pad(xe.double(), (0, 0, 1, 2, 1, 1))                       # [To + KT - 1, H + 2, W + 3, C] (one spare column: the fault)
    w3 = w.double().view(w.shape[0], 9 * KT, C)
    y = torch.zeros(To * H * W, w.shape[0], dtype=torch.float64, device=x.device)
    for tap in range(9 * KT):
        dt, dh, dw = tap // 9, (tap % 9) // 3, tap % 3
        sl = xp[dt:dt + To, dh:dh + H, dw:dw + W].reshape(-1, C)
        if fault is not None and fault[0] == tap:
            cg, mask = fault[1], fault[2].reshape(-1, 1).to(x.device)
            sh = xp[dt:dt + To, dh:dh + H, dw + 1:dw + 1 + W].reshape(-1, C)
            sl = sl.clone()
            sl[:, cg * 64:cg * 64 + 64] = torch.where(mask, sh[:, cg * 64:cg * 64 + 64], sl[:, cg * 64:cg * 64 + 64])
        y += sl @ w3[:, tap].T
    y += bias.double()
    if res is not None:
        y += res.double()
    return y


def last_tile_pixels(g):
    """Mask [To, H, W] of the pixels whose padded row lies in the last row tile that stores any."""
    t, h, w = torch.meshgrid(torch.arange(g["To"]), torch.arange(g["H"]), torch.arange(g["W"]), indexing="ij")
    tile = ((t * g["Hp"] + h) * g["Wp"] + w) // 256
    return tile == tile.max()


def describe_conv(c, bad, got, ref):
    """Failure text for got / ref [rows, Cout]: ``describe``'s count and tile boxes plus the first bad element's pixel, the tile
    of its PADDED row and its wave fragment (gemm_wide_epilogue.h: wave (wm, wn) owns 128 x 128, row block j, lane fr + 16 fq,
    accumulator register e, value i)."""
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "no bad elements"
    g = conv_geometry(c)
    r, n = int(idx[0, 0]), int(idx[0, 1])
    t, h, w = r // (g["H"] * g["W"]), r // g["W"] % g["H"], r % g["W"]
    m = (t * g["Hp"] + h) * g["Wp"] + w
    mi, ni = m % 256, n % 256
    return (f"{describe(bad, got, ref)}; first bad element: pixel (t, h, w) = ({t}, {h}, {w}) channel {n}: padded row {m}, tile (m {m // 256} of "
            f"{g['tiles_m']}, n {n // 256} of {g['tiles_n']}), wave (wm {mi // 128}, wn {ni // 128}), row block j {mi % 128 // 16}, lane fr {mi % 16} "
            f"fq {ni % 32 // 8}, register e {ni % 128 // 32}, value i {ni % 8}")


def assert_conv_exact(c, got, ref64, what=""):
    ref = ref64.to(BF)
    bad = bad_elements(got, ref)
    assert not bool(bad.any()), f"{c['name']} {what}: {describe_conv(c, bad, got, ref)}"


# ------------------------------------------------------------------------------------------------------------ GroupNorm statistics
# (C, rows): cg = C / 32 of 1, 2, 4, 8, 16; rows of 1, 511, 513; rows no multiple of rstep = 2048 / C (64, 32, 16, 8, 4); three blocks
STATS_CASES = [(32, 1), (64, 511), (128, 513), (256, 1), (512, 511), (512, 513), (32, 513), (64, 130), (128, 511), (256, 1027), (512, 7)]
# rows > 512 * 256 and rows % 512 != 0: 258 blocks -- the second trip of pass 2's strided loop, a ragged last block of 188 rows
STATS_LARGE = (32, 131072 + 700)


def group_pairs(rng, lo=-8, hi=8):
    """(mu_g, d_g) for the 32 groups: 32 different pairs of an integer in [lo, hi] and 1 or 2."""
    pairs = [(m, d) for m in range(lo, hi + 1) for d in (1, 2)]
    pick = rng.permutation(len(pairs))[:GROUPS]
    return np.array([pairs[i][0] for i in pick]), np.array([pairs[i][1] for i in pick])


def group_chunk(rng, rows, C, mu, d):
    """x [rows, C] int64 = mu_g + d_g e, e = +-1 with ceil(count / 2) entries of each group positive, in a seeded order over the
    whole group -> (x, e)."""
    cg = C // GROUPS
    count = rows * cg
    rank = rng.random((GROUPS, count)).argsort(1).argsort(1)
    e = np.where(rank < (count + 1) // 2, 1, -1).astype(np.int64)                       # [groups, rows * cg]
    e = np.ascontiguousarray(e.reshape(GROUPS, rows, cg).transpose(1, 0, 2)).reshape(rows, C)      # (row-major: cg = 1 would give a view)
    x = np.repeat(mu, cg)[None] + np.repeat(d, cg)[None] * e
    return torch.from_numpy(x), torch.from_numpy(e)


def stats_data(C, rows):
    """-> dict: x [rows, C] bf16 (CPU), mu, d [32], sums [64] int64 (exact), partial [blocks, 32, 2] int64 (exact)."""
    rng = np.random.RandomState(C * 7919 + rows)
    mu, d = group_pairs(rng)
    x, _ = group_chunk(rng, rows, C, mu, d)
    cg = C // GROUPS
    blocks = (rows + GN_ROWS - 1) // GN_ROWS
    xp = torch.zeros(blocks * GN_ROWS, C, dtype=torch.int64)
    xp[:rows] = x
    xg = xp.view(blocks, GN_ROWS, GROUPS, cg)
    partial = torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1)                  # [blocks, groups, 2]
    xb = x.to(BF)
    assert torch.equal(xb.double(), x.double())
    return dict(x=xb, mu=mu, d=d, sums=partial.sum(0).reshape(-1), partial=partial, count=rows * cg)


def stats_bound(dat):
    """The largest magnitude any partial sum can reach: count * max x^2 (must be < 2^24)."""
    return dat["count"] * int(dat["x"].double().abs().max()) ** 2


# ------------------------------------------------------------------------------------------------------------ norm + activation
def _norm(name, C, T, H, W, groups=GROUPS, eps=0.0, form="plain", lat=None, tmode=1, out_pad=False, act="none"):
    return dict(name=name, C=C, T=T, H=H, W=W, groups=groups, eps=eps, form=form, lat=lat, tmode=tmode, out_pad=out_pad, act=act)


# form: "plain" (GroupNorm alone: the encoder), "mod" (spatial modulation: the decoder), "sens" (variance-sensitive, plain).
# lat = (Tz, hz, wz).  C = 128: cg = 4, the per-element group lookup; 256 / 512: cg = 8 / 16, one lookup per piece; C = 96 with 32
# groups: cg = 3 and C / 8 = 12, no power of two: the cpr_shift = -1 division path
NORM_CASES = [
    _norm("c128-plain", 128, 2, 5, 6),
    _norm("c128-mod-eps3-pad", 128, 5, 4, 6, eps=3.0, form="mod", lat=(3, 2, 3), tmode=2, out_pad=True),
    _norm("c256-mod", 256, 4, 4, 8, form="mod", lat=(2, 1, 2), tmode=1),
    _norm("c512-plain-eps3-pad", 512, 1, 3, 5, eps=3.0, out_pad=True),
    _norm("c512-mod-pad", 512, 3, 2, 4, form="mod", lat=(3, 2, 4), tmode=0, out_pad=True),
    _norm("c96-mod-eps3", 96, 3, 4, 4, eps=3.0, form="mod", lat=(2, 2, 2), tmode=2),
    _norm("c96-plain-pad", 96, 2, 3, 7, out_pad=True),
    _norm("c64-plain", 64, 2, 4, 8),
    _norm("c128-sens", 128, 1, 8, 16, form="sens"),
    _norm("c256-sens-pad", 256, 2, 4, 8, form="sens", out_pad=True),
    _norm("c96-sens", 96, 1, 8, 16, form="sens"),
]
SILU_CASES = [
    _norm("silu-c128-mod", 128, 5, 4, 6, form="mod", lat=(3, 2, 3), tmode=2, act="silu"),
    _norm("silu-c256-plain-eps3", 256, 2, 4, 8, eps=3.0, act="silu"),
    _norm("silu-c512-mod-pad", 512, 4, 2, 4, form="mod", lat=(2, 2, 4), tmode=1, out_pad=True, act="silu"),
    _norm("silu-c96-mod-eps3", 96, 3, 4, 4, eps=3.0, form="mod", lat=(2, 2, 2), tmode=2, act="silu"),
]
# (T, Tz, tmode, shift): T / Tz of 5 / 3, 9 / 3, 4 / 2, 1 / 1 and an equal count; every shift with every tmode
INDEX_CASES = [(5, 3, 2, 1), (9, 3, 2, 0), (9, 3, 2, 2), (4, 2, 1, 2), (4, 2, 1, 0), (1, 1, 1, 1), (3, 3, 0, 0), (3, 3, 0, 1), (2, 2, 0, 2)]
INDEX_LATENT = (3, 4)            # hz, wz: at most 3 * 3 * 4 = 36 latent rows


def latent_rows(T, H, W, Tz, hz, wz, tmode, frame_of=None):
    """Nearest resizing in integer arithmetic: the latent row of every pixel of [T, H, W] -> int64 [T * H * W].  Space: h * hz // H
    (H = hz << shift).  Time: tmode 0 the same frame; 1 t * Tz // T; 2 the first frame apart: 0, then 1 + (t - 1) * (Tz - 1) // (T - 1).
    ``frame_of``: a planted replacement of the time rule."""
    t = torch.arange(T)
    if frame_of is not None:
        tz = frame_of(t)
    elif tmode == 0:
        tz = t
    elif tmode == 1:
        tz = t * Tz // T
    else:
        tz = torch.where(t == 0, torch.zeros_like(t), 1 + (t - 1) * (Tz - 1) // max(T - 1, 1))
    hh, ww = torch.arange(H) * hz // H, torch.arange(W) * wz // W
    return ((tz[:, None, None] * hz + hh[None, :, None]) * wz + ww[None, None, :]).reshape(-1)


def assert_mean_var(count, mus, ds):
    """fl(fl(count mu) / count) == mu and the same for mu^2 + d^2, in IEEE fp32."""
    cf = np.float32(count)
    for mu in mus:
        assert np.float32(count * mu) == count * mu and np.float32(count * mu) / cf == np.float32(mu), (count, mu)
        for d in ds:
            m2 = int(mu) ** 2 + int(d) ** 2
            assert np.float32(count * m2) == count * m2 and np.float32(count * m2) / cf == np.float32(m2), (count, mu, d)


def _norm_draw(c, seed):
    C, T, H, W, G = c["C"], c["T"], c["H"], c["W"], c["groups"]
    rows, cg = T * H * W, C // G
    count = rows * cg
    assert count % 2 == 0
    rng = np.random.RandomState(seed)
    mu, d = group_pairs(rng)
    if c["eps"] or c["form"] == "sens":
        d = np.ones_like(d)
    x, e = group_chunk(rng, rows, C, mu, d)
    k = 0.5 if c["eps"] else 1.0
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    if c["form"] == "sens":
        gamma = torch.ones(C).double()
        beta = sign * (2.0 ** -8 + xn.sens_delta(count))
    else:
        gamma = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], C)).double()
        beta = sign * (torch.ceil(k * gamma) + torch.from_numpy(rng.randint(1, 5, C)).double())
    sums = torch.zeros(2 * G, dtype=torch.float64)
    sums[0::2] = torch.from_numpy(count * mu).double()
    sums[1::2] = torch.from_numpy(count * (mu * mu + d * d)).double()
    pre = e.double() * k * gamma + beta                                               # the closed form [rows, C]
    zyb = zr = None
    if c["form"] == "mod":
        Tz, hz, wz = c["lat"]
        n = Tz * hz * wz
        zy = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], (n, C))).double()
        zb = sign[None] * torch.from_numpy(rng.randint(1, 7, (n, C))).double()
        zyb = torch.cat([zy, zb], 1)                                                  # the two halves of one buffer: ldz = 2 C
        zr = latent_rows(T, H, W, Tz, hz, wz, c["tmode"])
        pre = pre * zy[zr] + zb[zr]
    tobf = xn._exact_bf
    return dict(x=tobf(x.double()).view(T, H, W, C), e=e, mu=mu, d=d, k=k, count=count, sums=sums.float(), gamma=tobf(gamma), beta=tobf(beta),
                zyb=None if zyb is None else tobf(zyb), zr=zr, pre=pre, seed=seed)


def silu64(p):
    return p / (1.0 + torch.exp(-p))


def silu_window_share(pre):
    """Share of the elements whose fp64 SiLU lies within ``SILU_WINDOW`` relative of a bf16 rounding boundary."""
    return float((xn.boundary_distance(silu64(pre)) < SILU_WINDOW).double().mean())


def norm_data(c):
    """The tensors of norm case ``c`` (CPU) -> dict: x [T, H, W, C], sums fp32 [2 G] (hand-made, exact), gamma, beta [C], zyb
    [Tz hz wz, 2 C] or None, zr (latent row per pixel), pre = the exact value before the activation fp64 [rows, C].  SiLU cases: the
    first seed whose grid has at most 2 % of its elements in the rounding-boundary window."""
    for attempt in range(50):
        dat = _norm_draw(c, seed_of(c["name"]) + 1009 * attempt)
        if c["act"] != "silu" or silu_window_share(dat["pre"]) <= 0.02:
            return dat
    raise AssertionError(f"{c['name']}: no grid with at most 2 % of its elements in the SiLU window")


def norm_reference(c, dat, dev="cpu", eps=None, var_scale=1.0, zr=None):
    """The definition in fp64 from the DATA (statistics recomputed from x, not read from ``sums``): GroupNorm over the chunk's
    groups, * zy[zr] + zb[zr], before the activation -> fp64 [rows, C].  Planted faults: ``eps``, ``var_scale`` (count / (count - 1)),
    ``zr`` (another index map)."""
    C, G = c["C"], c["groups"]
    x = dat["x"].to(dev).double().view(-1, C)
    xg = x.view(x.shape[0], G, C // G)
    mean = xg.mean((0, 2), keepdim=True)
    var = ((xg - mean) ** 2).mean((0, 2), keepdim=True) * var_scale
    y = ((xg - mean) / torch.sqrt(var + (c["eps"] if eps is None else eps))).reshape(-1, C)
    y = y * dat["gamma"].to(dev).double() + dat["beta"].to(dev).double()
    if dat["zyb"] is not None:
        zyb = dat["zyb"].to(dev).double()
        r = (dat["zr"] if zr is None else zr).to(dev)
        y = y * zyb[r, :C] + zyb[r, C:]
    return y


def emulate_norm(c, dat, ulps):
    """vae_norm_act_kernel's expression in fp32, rstd = the true one moved by ``ulps`` ulps, each multiply-add contracted to an fma
    and not -> list of bf16 [rows, C] (before the activation)."""
    C, cg = c["C"], c["C"] // c["groups"]
    cen = (torch.from_numpy(np.repeat(dat["d"], cg))[None] * dat["e"]).double()       # x - mean, exact
    var = torch.from_numpy(np.repeat(dat["d"] ** 2, cg)).double()[None]
    true_rstd = (1.0 / torch.sqrt(var + c["eps"])).float()
    assert torch.equal(true_rstd.double() ** 2 * (var + c["eps"]), torch.ones_like(var)), "the true rstd is not an fp32 number"
    t = xn.f32(xn.f32(cen * xn.move_ulps(true_rstd, ulps).double()) * dat["gamma"].double())
    outs = []
    for fma in (True, False):
        y = xn.f32(t + dat["beta"].double())                                          # (gamma is a power of two: t is exact either way)
        if dat["zyb"] is not None:
            zyb = dat["zyb"].double()
            zy, zb = zyb[dat["zr"], :C], zyb[dat["zr"], C:]
            y = xn.fma32(y, zy, zb) if fma else xn.f32(xn.f32(y * zy) + zb)
        outs.append(y.to(BF))
    return outs


def assert_norm_conditions(c, dat):
    """x exact with the sums the case hands to the kernel; the quotients exact; y != 0 with at most 8 significant bits (sens: half
    the elements delta above a boundary); the fp64 definition rounds to the closed form; the fp32 restatement with rstd +- 2 ulps
    gives its bf16."""
    C, G = c["C"], c["groups"]
    cg = C // G
    x = dat["x"].double().view(-1, C)
    xg = x.view(-1, G, cg)
    assert torch.equal(xg.sum((0, 2)), dat["sums"][0::2].double()) and torch.equal((xg * xg).sum((0, 2)), dat["sums"][1::2].double())
    assert_mean_var(dat["count"], dat["mu"], set(dat["d"]))
    assert not c["eps"] or bool((dat["d"] == 1).all())
    y = dat["pre"]
    assert bool((y != 0).all()), "a true result is 0"
    want = y.to(BF)
    if c["form"] == "sens":
        dist, near = xn.boundary_distance(y), y.abs() > 1
        assert float(dist.min()) >= 2.0 ** -16 and 0.4 < float(near.double().mean()) < 0.6
        assert bool((dist[near] < 1.0 / (4 * dat["count"])).all()) and bool((dist[~near] > 2.0 ** -10).all())
    else:
        assert int(xn.sig_bits(y).max()) <= 8, int(xn.sig_bits(y).max())
        assert torch.equal(want.double(), y)
        assert float(y.abs().max()) <= 22
    ref = norm_reference(c, dat)
    assert float(((ref - y).abs() / y.abs()).max()) < 2.0 ** -40
    assert torch.equal(ref.to(BF), want)
    for ulps in (-2, -1, 0, 1, 2):
        for got in emulate_norm(c, dat, ulps):
            bad = bad_elements(got, want)
            assert not bool(bad.any()), f"{c['name']} rstd {ulps:+d} ulps: {describe(bad, got, want)}"


def index_data(T, Tz, tmode, shift, C=128):
    """Index-map case -> dict: x [T, H, W, C] (any finite data), sums (mean 0, variance 1), gamma = 0, beta = 1, zyb [rows_z, 2 C],
    zr, want bf16 [rows, C] = zy[zr] + zb[zr]."""
    hz, wz = INDEX_LATENT
    H, W = hz << shift, wz << shift
    n = Tz * hz * wz
    assert n <= 63
    g = torch.Generator().manual_seed(T * 100 + Tz * 10 + shift)
    x = torch.randint(-3, 4, (T, H, W, C), generator=g).to(BF)
    count = T * H * W * (C // GROUPS)
    sums = torch.zeros(2 * GROUPS)
    sums[1::2] = float(count)
    r, ch = torch.arange(n)[:, None], torch.arange(C)[None]
    zy = (1.0 + r).expand(n, C).double()
    zb = ((3 * r + ch) % 4).double() / 4
    zr = latent_rows(T, H, W, Tz, hz, wz, tmode)
    want = (zy + zb)[zr]
    assert torch.equal(want.to(BF).double(), want)
    return dict(x=x, sums=sums, gamma=torch.zeros(C, dtype=BF), beta=torch.ones(C, dtype=BF), zyb=torch.cat([zy, zb], 1).to(BF).contiguous(),
                zr=zr, want=want.to(BF), lat=(Tz, hz, wz), shape=(T, H, W, C))


def padded_interior(ypad):
    """The part of a zero-padded conv input [T + 2, H + 2, W + 2, C] the norm kernel owns: frames 2.., one pixel in."""
    return ypad[2:, 1:-1, 1:-1]


def pad_rest_mask(ypad):
    m = torch.ones(ypad.shape, dtype=torch.bool, device=ypad.device)
    m[2:, 1:-1, 1:-1] = False
    return m


def describe_norm(c_or_shape, bad, got, ref):
    shape = c_or_shape if isinstance(c_or_shape, tuple) else (c_or_shape["T"], c_or_shape["H"], c_or_shape["W"], c_or_shape["C"])
    idx = bad.reshape(-1, shape[3]).nonzero()
    if idx.numel() == 0:
        return "no bad elements"
    r, ch = int(idx[0, 0]), int(idx[0, 1])
    g, w = got.reshape(-1, shape[3]), ref.reshape(-1, shape[3])
    return (f"{idx.shape[0]} of {bad.numel()} elements differ; first: pixel (t, h, w) = ({r // (shape[1] * shape[2])}, {r // shape[2] % shape[1]}, "
            f"{r % shape[2]}) channel {ch} (piece {ch // 8}): got {float(g[r, ch])!r}, want {float(w[r, ch])!r}")


def ulp_distance(got, ref):
    """|bits(got) - bits(ref)| of bf16 tensors of one sign pattern (int64; a large number where the signs differ)."""
    g, r = got.contiguous().view(torch.int16).long(), ref.contiguous().view(torch.int16).long()
    return torch.where((g < 0) == (r < 0), (g - r).abs(), torch.full_like(g, 1 << 20))


# ------------------------------------------------------------------------------------------------------------ patch gather
def _patch(name, C, KT, stride, T, H, W, Kpad, cache=False, slab=None):
    return dict(name=name, C=C, KT=KT, stride=stride, T=T, H=H, W=W, Kpad=Kpad, cache=cache, slab=slab)


# slab = (t0, nt): frames [t0, t0 + nt) only.  C = 3 is vae_patches_small_kernel: KT = 3 has 81 columns, Kpad = 128 gives 43 slots of
# which 16 are zero and the last holds two columns; KT = 1 at stride 2 has 27 columns, Kpad = 64: 22 slots, the last of one column
PATCH_CASES = [
    _patch("c3-kt3", 3, 3, 1, 3, 5, 7, 128),
    _patch("c3-kt3-cache", 3, 3, 1, 3, 5, 7, 128, cache=True),
    _patch("c3-kt3-slab", 3, 3, 1, 3, 5, 7, 128, slab=(1, 2)),
    _patch("c3-kt3-cache-slab", 3, 3, 1, 3, 5, 7, 128, cache=True, slab=(1, 2)),
    _patch("c3-stride2-odd", 3, 1, 2, 2, 7, 9, 64),
    _patch("c8-kt3-kpad256", 8, 3, 1, 2, 4, 5, 256, cache=True),
    _patch("c16-kt3-kpad512", 16, 3, 1, 2, 3, 5, 512, slab=(1, 1)),
    _patch("c128-stride2-odd", 128, 1, 2, 2, 7, 9, 1152),
    _patch("c256-stride2-odd-kpad", 256, 1, 2, 1, 5, 7, 2304 + 64),
    _patch("c512-kt3", 512, 3, 1, 1, 3, 4, 13824),
]


def patch_out_shape(c):
    if c["stride"] == 2:
        return (c["H"] + 1 - 3) // 2 + 1, (c["W"] + 1 - 3) // 2 + 1
    return c["H"], c["W"]


def patch_reference(x, cache, KT, stride):
    """torch's unfold on [front | x] (front: the cache or the first frame twice), zero space padding (1, 1) at stride 1 and (0, 1)
    at stride 2 -> bf16 [To * Ho * Wo, KT * 9 * C], columns (kt, kh, kw, c)."""
    C = x.shape[-1]
    xs = x
    if KT == 3:
        xs = torch.cat([cache if cache is not None else x[:1].repeat(2, 1, 1, 1), x], 0)
    lo, hi = (1, 1) if stride == 1 else (0, 1)
    xp = F.pad(xs.permute(3, 0, 1, 2)[None].float(), (lo, hi, lo, hi))
    u = xp.unfold(2, KT, 1).unfold(3, 3, stride).unfold(4, 3, stride)
    return u.permute(0, 2, 3, 4, 5, 6, 7, 1).reshape(-1, KT * 9 * C).to(BF)
