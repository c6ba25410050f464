"""GPU: csrc/vae.hip and the CONV instance of csrc/gemm_v4.hip on exact data (tests/exact_vae.py).  Every output sits inside a
sentinel buffer, is poisoned with NaN before the launch and must equal the fp64 definition rounded once, bit for bit (SiLU: within
the derived one-ulp bound); a failure names the element, its pixel, its tile and its wave fragment.  The case tables live in
exact_vae.py, where test_vae_exact_cpu.py checks their conditions and their coverage of the stock model's convolutions."""
import pytest
import torch

import exact_vae as xv
from exact_vae import BF, GuardedOut, bad_elements

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def _padded_input(c, dat, dev):
    """The zero-padded conv input of a KT = 3 case: [To + 2, H + 2, W + 2, C], the context frames (cache, or the first frame twice)
    in front."""
    x, ctx = dat["x"], dat["ctx"]
    T, H, W, C = x.shape
    xpad = torch.zeros(T + c["KT"] - 1, H + 2, W + 2, C, dtype=BF, device=dev)
    xpad[c["KT"] - 1:, 1:-1, 1:-1] = x
    if c["KT"] == 3:
        xpad[:2, 1:-1, 1:-1] = ctx if ctx is not None else x[:1].expand(2, H, W, C)
    return xpad


def _run_conv(ops, c, dat, xpad, ref64, dev):
    """bya_vae_conv3d of case ``c`` on the padded input into a guarded, poisoned view; exact against ``ref64``."""
    g = xv.conv_geometry(c)
    rows, Cout = g["To"] * g["H"] * g["W"], c["Cout"]
    out = GuardedOut(rows, Cout, dev)
    y = out.view().view(g["To"], g["H"], g["W"], Cout)
    assert y.stride(2) > Cout                                             # ldc > Cout: sentinel columns between Cout and ldc
    res = None
    if c["res"] == "alias":
        out.fill(dat["res"])
        res = y
    elif c["res"] == "separate":
        wide = torch.zeros(rows, Cout + 24, dtype=BF, device=dev)
        wide[:, :Cout] = dat["res"]
        res = wide[:, :Cout].view(g["To"], g["H"], g["W"], Cout)
        assert res.stride(2) != y.stride(2)                               # ldres != ldc
    assert dat["w"].shape[0] == Cout                                      # w has exactly Cout rows: the rest of the tile is clipped
    ops.vae_conv3d(xpad, dat["w"], dat["bias"], y, res=res, KT=c["KT"])
    torch.cuda.synchronize()
    xv.assert_conv_exact(c, out.gathered(), ref64)
    assert out.guard_intact(), f"{c['name']}: a write outside [To, H, W, Cout] (rows before / after the view or columns Cout .. ldc)"


@pytest.mark.parametrize("c", xv.CONV_CASES, ids=lambda c: c["name"])
def test_conv3d_exact(ops, dev, c):
    dat = xv.conv_data(c, dev)
    ref = xv.conv_reference(dat["x"], dat["ctx"], dat["w"], dat["bias"], dat["res"], c["KT"])
    _run_conv(ops, c, dat, _padded_input(c, dat, dev), ref, dev)
    g = xv.conv_geometry(c)
    print(f"{c['name']}: {g['M']} padded rows, {g['tiles_m']} x {g['tiles_n']} tiles, K = {9 * c['KT'] * c['C']}: bit-exact, guards intact")


def test_conv3d_exact_multi_round(ops, dev):
    """More output tiles than the persistent grid, and no multiple of it: the tile walk, the next tile's two K-tiles prefetched
    under the current epilogue and the clipped last tiles, all behind a full round.  380 tiles on 256 workgroups: 124 workgroups
    walk two tiles, 132 one (``persistent_walk``, persistent_grid's rule)."""
    c = xv.CONV_MULTI_ROUND
    g = xv.conv_geometry(c)
    grid, counts = xv.persistent_walk(g["tiles"])
    hist = {n: counts.count(n) for n in sorted(set(counts))}
    print(f"{c['name']}: {g['tiles']} tiles ({g['tiles_m']} x {g['tiles_n']}) on {grid} workgroups; tiles per workgroup: {hist}; "
          f"{g['M'] % 256} rows in the last row tile")
    assert g["tiles"] > grid == 256 and g["tiles"] % grid and max(counts) >= 2 and hist == {1: 132, 2: 124}
    dat = xv.conv_data(c, dev)
    ref = xv.conv_reference(dat["x"], dat["ctx"], dat["w"], dat["bias"], dat["res"], c["KT"])
    _run_conv(ops, c, dat, _padded_input(c, dat, dev), ref, dev)


@pytest.mark.parametrize("c", xv.UP_CASES, ids=lambda c: c["name"])
def test_upsample_pad_and_conv_exact(ops, dev, c):
    """bya_vae_upsample_pad into a sentinel-bordered buffer: the interior equals repeat_interleave bit for bit, the border is
    untouched; then bya_vae_conv3d(KT = 1) on exact data against the fp64 definition (not against the patch path)."""
    dat = xv.conv_data(c, dev)
    g = xv.conv_geometry(c)
    up = xv.upsample_reference(dat["x"], c["up"])
    assert tuple(up.shape[:3]) == (g["To"], g["H"], g["W"])
    ypad = xv.sentinel((g["To"], g["Hp"], g["Wp"], c["C"]), dev)
    ypad[:, 1:-1, 1:-1] = float("nan")
    ops.vae_upsample_pad(dat["x"], ypad, c["up"])
    torch.cuda.synchronize()
    bad = bad_elements(ypad[:, 1:-1, 1:-1], up)
    assert not bool(bad.any()), f"{c['name']}: {xv.describe_norm(tuple(up.shape), bad, ypad[:, 1:-1, 1:-1], up)}"
    border = torch.ones(ypad.shape, dtype=torch.bool, device=dev)
    border[:, 1:-1, 1:-1] = False
    assert bool(xv.is_sentinel(ypad)[border].all()), f"{c['name']}: the border of the padded buffer was written"
    ypad[border] = 0.0                                                     # the convolution's zero padding
    ref = xv.conv_reference(up, None, dat["w"], dat["bias"], None, 1)
    _run_conv(ops, c, dat, ypad, ref, dev)


# ------------------------------------------------------------------------------------------------------------ GroupNorm statistics
def _run_stats(ops, dev, C, rows):
    dat = xv.stats_data(C, rows)
    x = dat["x"].to(dev)
    blocks = dat["partial"].shape[0]
    runs = []
    for _ in range(2):
        sums = torch.full((2 * xv.GROUPS + 8,), float("nan"), dtype=torch.float32, device=dev)
        part = torch.full((blocks * xv.GROUPS * 2 + 8,), float("nan"), dtype=torch.float32, device=dev)
        ops.vae_groupnorm_stats(x, sums[:2 * xv.GROUPS], xv.GROUPS, part[:blocks * xv.GROUPS * 2])
        torch.cuda.synchronize()
        assert bool(sums[2 * xv.GROUPS:].isnan().all()) and bool(part[blocks * xv.GROUPS * 2:].isnan().all()), "a write past the outputs"
        runs.append((sums[:2 * xv.GROUPS].cpu(), part[:blocks * xv.GROUPS * 2].cpu()))
    got, gpart = runs[0]
    want = dat["sums"].double()
    bad = (got.double() != want).nonzero()
    assert bad.numel() == 0, (f"C={C} rows={rows}: {bad.shape[0]} of 64 sums differ; first: group {int(bad[0]) // 2} moment {int(bad[0]) % 2}: "
                              f"got {float(got[int(bad[0])])!r}, want {float(want[int(bad[0])])!r} (a difference of "
                              f"{float(got[int(bad[0])]) - float(want[int(bad[0])])!r})")
    wpart = dat["partial"].double().reshape(-1)
    bad = (gpart.double() != wpart).nonzero()
    assert bad.numel() == 0, (f"C={C} rows={rows}: {bad.shape[0]} partial sums differ; first: block {int(bad[0]) // 64} group {int(bad[0]) % 64 // 2} "
                              f"moment {int(bad[0]) % 2}: got {float(gpart[int(bad[0])])!r}, want {float(wpart[int(bad[0])])!r}")
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), "two launches on the same data differ"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), "two launches' partial sums differ"


@pytest.mark.parametrize("C,rows", xv.STATS_CASES, ids=lambda v: str(v))
def test_groupnorm_stats_exact(ops, dev, C, rows):
    _run_stats(ops, dev, C, rows)


def test_groupnorm_stats_exact_large(ops, dev):
    """258 blocks: the second trip of pass 2's strided loop and a ragged last block of 188 rows; every partial is the exact sum of
    its 512 rows."""
    _run_stats(ops, dev, *xv.STATS_LARGE)


# ------------------------------------------------------------------------------------------------------------ norm + activation
def _launch_norm(ops, dev, c, dat, act):
    """-> (result [T, H, W, C], the buffer it lives in, mask of the elements the kernel does not own)."""
    T, H, W, C = dat["x"].shape
    x = dat["x"].to(dev)
    kw = {}
    if dat["zyb"] is not None:
        zyb = dat["zyb"].to(dev)
        assert zyb.stride(0) == 2 * C
        kw = dict(zy=zyb[:, :C], zb=zyb[:, C:], latent_shape=c["lat"], tmode=c["tmode"])
    if c["out_pad"]:
        buf = xv.sentinel((T + 2, H + 2, W + 2, C), dev)
        y, rest = xv.padded_interior(buf), xv.pad_rest_mask(buf)
        y[:] = float("nan")
        ops.vae_norm_act(x, buf, dat["sums"].to(dev), dat["gamma"].to(dev), dat["beta"].to(dev), c["groups"], act=act, eps=c["eps"], out_pad=True, **kw)
    else:
        buf = xv.sentinel((T + 2, H, W, C), dev)                           # a spare frame of sentinel before and after
        y = buf[1:-1]
        rest = torch.ones(buf.shape, dtype=torch.bool, device=dev)
        rest[1:-1] = False
        y[:] = float("nan")
        ops.vae_norm_act(x, y, dat["sums"].to(dev), dat["gamma"].to(dev), dat["beta"].to(dev), c["groups"], act=act, eps=c["eps"], **kw)
    torch.cuda.synchronize()
    return y, buf, rest


@pytest.mark.parametrize("c", xv.NORM_CASES, ids=lambda c: c["name"])
def test_norm_act_exact(ops, dev, c):
    dat = xv.norm_data(c)
    y, buf, rest = _launch_norm(ops, dev, c, dat, "none")
    ref = xv.norm_reference(c, dat, dev).to(BF).view(y.shape)
    bad = bad_elements(y, ref)
    assert not bool(bad.any()), f"{c['name']}: {xv.describe_norm(c, bad, y, ref)}"
    assert bool(xv.is_sentinel(buf)[rest].all()), f"{c['name']}: the border, a context frame or a neighbouring frame was written"


@pytest.mark.parametrize("T,Tz,tmode,shift", xv.INDEX_CASES, ids=lambda v: str(v))
def test_norm_act_index_map(ops, dev, T, Tz, tmode, shift):
    """gamma = 0, beta = 1: y == zy[zr] + zb[zr] bit for bit, zr by nearest resizing in integer arithmetic."""
    dat = xv.index_data(T, Tz, tmode, shift)
    c = dict(lat=dat["lat"], tmode=tmode, out_pad=False, groups=xv.GROUPS, eps=0.0, name=f"index T{T} Tz{Tz} tmode{tmode} shift{shift}")
    y, buf, rest = _launch_norm(ops, dev, c, dat, "none")
    want = dat["want"].to(dev).view(y.shape)
    bad = bad_elements(y, want)
    assert not bool(bad.any()), f"{c['name']}: {xv.describe_norm(dat['shape'], bad, y, want)}"
    assert bool(xv.is_sentinel(buf)[rest].all())


@pytest.mark.parametrize("c", xv.SILU_CASES, ids=lambda c: c["name"])
def test_norm_act_silu_within_one_ulp(ops, dev, c):
    """SiLU of the exact pre-activation against fp64: at most one bf16 ulp from bf16(reference), and different only where the
    fp64 value lies within 2^-16 relative of a rounding boundary (one fp32 evaluation rounded once).  Measured on an MI355X: no
    element of the four cases differs (0 ulp), none lies in the window, worst relative error against fp64 3.0e-3."""
    dat = xv.norm_data(c)
    y, buf, rest = _launch_norm(ops, dev, c, dat, "silu")
    ref64 = xv.silu64(xv.norm_reference(c, dat, dev)).view(y.shape)
    ref = ref64.to(BF)
    ulps = xv.ulp_distance(y, ref)
    differ = ulps != 0
    window = xv.xn.boundary_distance(ref64) < xv.SILU_WINDOW
    rel = ((y.double() - ref64).abs() / ref64.abs()).max()
    print(f"{c['name']}: worst relative error against fp64 {float(rel):.3e} (half a bf16 ulp is at most 3.9e-3), {float(differ.double().mean()) * 100:.3f} % "
          f"of the elements differ from bf16(fp64), {float(window.double().mean()) * 100:.3f} % lie in the window, worst distance {int(ulps.max())} ulp")
    assert int(ulps.max()) <= 1, f"{c['name']}: {xv.describe_norm(c, ulps > 1, y, ref)}"
    assert not bool((differ & ~window).any()), f"{c['name']}: differs outside the window: {xv.describe_norm(c, differ & ~window, y, ref)}"
    assert bool(xv.is_sentinel(buf)[rest].all()), f"{c['name']}: the border, a context frame or a neighbouring frame was written"


# ------------------------------------------------------------------------------------------------------------ patch gather
@pytest.mark.parametrize("c", xv.PATCH_CASES, ids=lambda c: c["name"])
def test_patches_exact(ops, dev, c):
    g = torch.Generator().manual_seed(xv.seed_of(c["name"]))
    T, H, W, C, KT = c["T"], c["H"], c["W"], c["C"], c["KT"]
    x = torch.randn(T, H, W, C, generator=g).to(BF).to(dev)
    cache = torch.randn(2, H, W, C, generator=g).to(BF).to(dev) if c["cache"] else None
    Ho, Wo = xv.patch_out_shape(c)
    t0, nt = c["slab"] if c["slab"] else (0, T)
    want = xv.patch_reference(x, cache, KT, c["stride"])[t0 * Ho * Wo:(t0 + nt) * Ho * Wo]
    rows, K = nt * Ho * Wo, KT * 9 * C
    buf = xv.sentinel((rows + 8, c["Kpad"]), dev)
    out = buf[3:3 + rows]
    out[:] = float("nan")
    ops.vae_patches(x, cache, out, KT, c["stride"], 1 if c["stride"] == 1 else 0, False, 0, Ho, Wo, t0, nt)
    torch.cuda.synchronize()
    bad = bad_elements(out[:, :K], want)
    first = bad.nonzero()[0].tolist() if bool(bad.any()) else None
    assert first is None, (f"{c['name']}: {int(bad.sum())} elements differ; first: row {first[0]} (pixel {first[0] // (Ho * Wo) + t0}, {first[0] // Wo % Ho}, "
                           f"{first[0] % Wo}) column {first[1]} (tap {first[1] // C}, channel {first[1] % C})")
    assert bool((out[:, K:].view(torch.int16) == 0).all()), f"{c['name']}: the columns behind the last tap are not zero"
    assert bool(xv.is_sentinel(buf[:3]).all()) and bool(xv.is_sentinel(buf[3 + rows:]).all()), f"{c['name']}: a write outside the patch matrix"
