"""The kv-mix whose epilogue writes MX codes (include/bya.h, bya_attn_kv_mix_mx; ops.attn_kv_mix(mx_out=...)) and the two
cross-attention output projections as MX Linears (enable_mx_weights(linears=(.., "po", "ao"))): byte for byte bya_attn_kv_mix
followed by bya_quantize_mx over formats, weight modes, head dims, identity counts, groups, ragged row counts and masked keys;
canaries around the rows; the sharded engine's per-segment call shape; the run-time refusal; bias_rowscale on every MX GEMM
path on exact data; the pair as the next GEMM's operand; the engine (fused against unfused bit for bit, launch counts, graph
replay, accuracy against the fake-quantised oracle under forced hard routing, drift) and the 2-rank sharded step."""
import os

import pytest
import torch

from conftest import rel_fro
from test_mx_attn_out_gpu import Counter, first_diff, two_launch_ref
from test_mx_cpu import dequant_mx
from test_mx_gpu import FakeMXLinear, exact_operand, hard_inputs, with_mx_dit_linears

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FORMATS = ("mxfp8", "mxfp6")
SIX = ("qkv", "out", "ff1", "ff2", "po", "ao")


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def mix_case(dev, mode, D, H, n_id, grp, Sq, Skv, special=None):
    """q [grp, Sq, E], k / v [n_id, grp, Skv, E], routing logits r [grp * Sq, n_id], af (audio) and the launch keywords.
    ``special``: "zero_v" = identity 1's V all zero; "zero_rows" = routing that zeroes every weight of rows 3, 40 and the last
    (all-zero blocks: scale byte 127, zero codes); "hard" = V rows of large dynamic range (tests/test_mx_gpu.py, hard_inputs)."""
    E = H * D
    g = torch.Generator().manual_seed(1000 * D + 100 * n_id + 10 * grp + Sq + Skv + (mode == "audio"))
    rnd = lambda *s: torch.randn(*s, generator=g)
    q, k, v = rnd(grp, Sq, E), rnd(n_id, grp, Skv, E), rnd(n_id, grp, Skv, E) * 2.0
    r = torch.sigmoid(rnd(grp * Sq, n_id))
    af = None if mode == "face" else torch.roll(torch.eye(n_id), 1, dims=1)
    if special == "zero_v":
        v[1] = 0
    if special == "hard":
        v = hard_inputs(n_id * grp * Skv, E, seed=Sq).float().view(n_id, grp, Skv, E)
    if special == "zero_rows":
        # face: w = r; audio: w[a] = prod_{b != a} (1 - (af r)[b]) with af a permutation: every r = 1 zeroes every weight
        r[[3, 40, grp * Sq - 1]] = 0.0 if mode == "face" else 1.0
    to = lambda t: None if t is None else t.to(BF).to(dev)
    kw = dict(head_dim=D, heads=H, n_id=n_id, n_grp=grp, Sq=Sq, Skv=Skv, q_strides=(Sq * E, E),
              k_strides=(grp * Skv * E, Skv * E, E), v_strides=(grp * Skv * E, Skv * E, E), scale=D ** -0.5)
    return to(q), to(k), to(v), to(r), to(af), kw


def pair(ops, lead, E, fmt, dev, extra=(0, 0)):
    """A 0xA5-filled (codes, scales) pair for a [*lead, E] mix, ``extra`` spare bytes per row."""
    return (torch.full((*lead, ops.mx_code_bytes(E, fmt) + extra[0]), 0xA5, dtype=torch.uint8, device=dev),
            torch.full((*lead, E // 32 + extra[1]), 0xA5, dtype=torch.uint8, device=dev))


def the_pair(ops, dev, q, k, v, r, af, kw):
    """bya_attn_kv_mix, then (per format) bya_quantize_mx: -> (z [grp * Sq, E], wsum, {fmt: (codes, scales)})."""
    grp, Sq, E = kw["n_grp"], kw["Sq"], kw["heads"] * kw["head_dim"]
    z = torch.empty(grp, Sq, E, dtype=BF, device=dev)
    ws = torch.full((grp * Sq,), -1.0, dtype=torch.float32, device=dev)
    assert ops.attn_kv_mix_plan(z, af, z_strides=(Sq * E, E), **kw)["form"] == "mix32"
    ops.attn_kv_mix(q, k, v, r, af, z, ws, z_strides=(Sq * E, E), **kw)
    return z.view(grp * Sq, E), ws, {f: two_launch_ref(ops, z.view(grp * Sq, E), f) for f in FORMATS}


def check_fused(ops, dev, q, k, v, r, af, kw, what):
    grp, Sq, E = kw["n_grp"], kw["Sq"], kw["heads"] * kw["head_dim"]
    z, ws_ref, ref = the_pair(ops, dev, q, k, v, r, af, kw)
    for fmt in FORMATS:
        codes, scales = pair(ops, (grp * Sq,), E, fmt, dev)
        ws = torch.full((grp * Sq,), -1.0, dtype=torch.float32, device=dev)
        plan = ops.attn_kv_mix_plan(None, af, mx_out=(codes, scales, fmt), **kw)
        assert plan["form"] == "mix32" and plan["mx_out"] == fmt, plan
        lds = (2 * kw["n_id"] + 4) * 32 * kw["head_dim"] * 2                          # K, V per identity + a z patch per wave
        assert plan["lds_bytes"] == lds and plan["big_lds"] == (lds > 64 * 1024)      # (3 and 4 identities at head_dim 128)
        got = ops.attn_kv_mix(q, k, v, r, af, None, ws, mx_out=(codes, scales, fmt), **kw)
        assert got is not False and got[0] is codes and got[1] is scales
        assert torch.equal(scales, ref[fmt][1]), f"{what} {fmt} scales: " + first_diff(scales, ref[fmt][1])
        assert torch.equal(codes, ref[fmt][0]), f"{what} {fmt} codes: " + first_diff(codes, ref[fmt][0])
        assert torch.equal(ws, ws_ref), f"{what} {fmt} wsum"
    return z, ref


# ------------------------------------------------------------------------------------------ 1. byte equality with the pair
@pytest.mark.parametrize("mode", ["face", "audio"])
@pytest.mark.parametrize("D,H", [(64, 3), (128, 2)])
def test_fused_launch_equals_kv_mix_then_quantiser(ops, dev, mode, D, H):
    """Both formats (inside check_fused) x n_id 2, 3, 4 (3 and 4 at head_dim 128: the big-LDS opt-in) x 1 and 2 groups x 45 rows (one
    ragged tile, one row chunk) and 420 rows (14 tiles: two row chunks, ragged last tile) x 32 keys and 20 (masked keys)."""
    n = 0
    for n_id in (2, 3, 4):
        for grp in (1, 2):
            for Sq in (45, 420):
                for Skv in (32, 20):
                    q, k, v, r, af, kw = mix_case(dev, mode, D, H, n_id, grp, Sq, Skv)
                    if Sq == 420:
                        assert ops.attn_kv_mix_plan(None, af, mx_out=(*pair(ops, (grp * Sq,), H * D, "mxfp8", dev), "mxfp8"),
                                                    **kw)["row_chunks"] == 2
                    check_fused(ops, dev, q, k, v, r, af, kw, f"{mode} d{D} n_id {n_id} grp {grp} Sq {Sq} Skv {Skv}")
                    n += 1
    assert n == 24


@pytest.mark.parametrize("special", ["zero_v", "zero_rows", "hard"])
@pytest.mark.parametrize("mode,D,H", [("face", 128, 2), ("audio", 64, 3)])
def test_fused_launch_on_zero_and_wide_range_inputs(ops, dev, special, mode, D, H):
    q, k, v, r, af, kw = mix_case(dev, mode, D, H, 2, 2, 45, 32, special)
    z, ref = check_fused(ops, dev, q, k, v, r, af, kw, f"{special} {mode}")
    if special == "zero_rows":
        for row in (3, 40, 89):
            assert bool((z[row] == 0).all())
            for fmt in FORMATS:
                assert bool((ref[fmt][1][row] == 127).all()) and bool((ref[fmt][0][row] == 0).all())
    if special == "hard":
        amax = z.float().abs().view(z.shape[0], -1, 32).amax(-1)
        amax = amax[torch.isfinite(amax) & (amax > 0)]
        assert float(amax.max() / amax.min()) > 1e6                      # block scales over many binades


# ------------------------------------------------------------------------------------------ 2. canaries
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mode,D,H,n_id", [("audio", 64, 3, 2), ("face", 128, 2, 3)])
def test_no_stray_writes_around_the_rows_or_the_heads_bytes(ops, dev, fmt, mode, D, H, n_id):
    grp, Sq, E = 2, 45, H * D
    q, k, v, r, af, kw = mix_case(dev, mode, D, H, n_id, grp, Sq, 20)
    _, _, ref = the_pair(ops, dev, q, k, v, r, af, kw)
    cb, sb = ops.mx_code_bytes(E, fmt), E // 32
    codes, scales = pair(ops, (grp, Sq + 3), E, fmt, dev, extra=(12, 5))          # spare rows per group, spare bytes per row
    assert codes.stride(1) % 4 == 0 and codes.stride(1) % 8 != 0                   # a 4-byte, not 8-byte, aligned row stride
    ops.attn_kv_mix(q, k, v, r, af, None, None, mx_out=(codes, scales, fmt), **kw)
    torch.cuda.synchronize()
    want_c, want_s = torch.full_like(codes, 0xA5), torch.full_like(scales, 0xA5)
    want_c[:, :Sq, :cb] = ref[fmt][0].view(grp, Sq, cb)
    want_s[:, :Sq, :sb] = ref[fmt][1].view(grp, Sq, sb)
    assert torch.equal(codes, want_c), "codes: " + first_diff(codes, want_c)
    assert torch.equal(scales, want_s), "scales: " + first_diff(scales, want_s)


# ------------------------------------------------------------------------------------------ 3. segments (the sharded call shape)
@pytest.mark.parametrize("fmt", FORMATS)
def test_row_segments_write_the_rows_of_one_launch(ops, dev, fmt):
    D, H, n_id, Sq = 64, 3, 2, 45
    E = H * D
    q, k, v, r, af, kw = mix_case(dev, "audio", D, H, n_id, 1, Sq, 32)
    one = pair(ops, (Sq,), E, fmt, dev)
    ws_one = torch.full((Sq,), -1.0, dtype=torch.float32, device=dev)
    ops.attn_kv_mix(q, k, v, r, af, None, ws_one, mx_out=(*one, fmt), **kw)
    seg = pair(ops, (Sq,), E, fmt, dev)
    ws = torch.full((Sq,), -1.0, dtype=torch.float32, device=dev)
    for start, length in ((0, 29), (29, 16)):
        ops.attn_kv_mix(q[0, start:], k, v, r[start:start + length], af, None, ws[start:],
                        mx_out=(seg[0][start:], seg[1][start:], fmt), **dict(kw, Sq=length, q_strides=(0, E)))
    assert torch.equal(seg[0], one[0]) and torch.equal(seg[1], one[1]) and torch.equal(ws, ws_one)
    assert not bool((one[0] == 0xA5).all())


# ------------------------------------------------------------------------------------------ 4. refusal at run time
def test_more_than_32_keys_returns_false_and_writes_nothing(ops, dev):
    q, k, v, r, af, kw = mix_case(dev, "audio", 64, 3, 2, 1, 45, 40)
    codes, scales = pair(ops, (45,), 192, "mxfp6", dev)
    ws = torch.full((45,), -1.0, dtype=torch.float32, device=dev)
    assert ops.attn_kv_mix_plan(None, af, mx_out=(codes, scales, "mxfp6"), **kw) is None
    assert ops.attn_kv_mix(q, k, v, r, af, None, ws, mx_out=(codes, scales, "mxfp6"), **kw) is False
    torch.cuda.synchronize()
    assert bool((codes == 0xA5).all()) and bool((scales == 0xA5).all()) and bool((ws == -1.0).all())
    with ops.options(reference_forms="kv_mix_generic"):                            # ... and under the generic reference form
        assert ops.attn_kv_mix(q, k, v, r, af, None, ws, mx_out=(codes, scales, "mxfp6"), **dict(kw, Skv=32)) is False
    with pytest.raises(ValueError):
        ops.attn_kv_mix(q, k, v, r, af, torch.empty(1, 45, 192, dtype=BF, device=dev), ws, mx_out=(codes, scales, "mxfp6"), **kw)


# ------------------------------------------------------------------------------------------ 5. bias_rowscale on the MX GEMMs
def rowscale_case(dev, M, N, K, fmt, seed):
    """Exact operands plus bias, residual (multiples of 1/4), a NON-CONSTANT power-of-two row scale and alpha = 1/2: every
    intermediate of alpha * (A W^T + rowscale * bias) + res is exact in fp32 (multiples of 2^-7 far below 2^17), so whatever
    the order and contraction of the epilogue, the stored value is the exact value rounded to bf16 once."""
    g = torch.Generator().manual_seed(seed)
    ac, asc = exact_operand(M, K, fmt, seed=seed)
    wc, wsc = exact_operand(N, K, fmt, seed=seed + 1)
    bias = (torch.randint(-12, 13, (N,), generator=g) / 4).to(BF)
    res = (torch.randint(-40, 41, (M, N), generator=g) / 4).to(BF)
    rs = torch.tensor([0.25, 0.5, 1.0, 2.0, 0.0])[torch.randint(0, 5, (M,), generator=g)].float()
    assert rs.unique().numel() == 5
    prod = dequant_mx(ac, asc, fmt).to(dev) @ dequant_mx(wc, wsc, fmt).to(dev).T                     # fp64 on the device: exact
    want = (0.5 * (prod + rs.double().to(dev)[:, None] * bias.double().to(dev)[None]) + res.double().to(dev)).to(BF)
    return [t.to(dev) for t in (ac, asc, wc, wsc)], dict(bias=bias.to(dev), res=res.to(dev), bias_rowscale=rs.to(dev), alpha=0.5), want


def assert_exact(got, want, what):
    bad = got.float() != want.float()
    print(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ")
    assert not bad.any(), what


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (300, 256, 2048)])
def test_gemm_mx_honours_bias_rowscale_tiled(ops, dev, fmt, M, N, K):
    ab, kw, want = rowscale_case(dev, M, N, K, fmt, seed=M + K)
    out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    assert ops.gemm_mx_plan(*ab, out, fmt, **kw)["path"] == "t128x128"
    ops.gemm_mx(*ab, out, fmt, **kw)
    assert_exact(out, want, f"gemm_mx {fmt} t128x128 {M}x{N}x{K}")
    if fmt == "mxfp8":                                  # option mx_kernel = 2: the persistent kernel wherever it is eligible
        with ops.options(mx_kernel=2):
            path = ops.gemm_mx_plan(*ab, out, fmt, **kw)["path"]
            out.fill_(float("nan"))
            ops.gemm_mx(*ab, out, fmt, **kw)
        assert path == ("p256" if K >= 512 else "t128x128")
        assert_exact(out, want, f"gemm_mx {fmt} mx_kernel=2 {path} {M}x{N}x{K}")


def test_gemm_mx_honours_bias_rowscale_on_the_256_tile(ops, dev):
    """The e2m3 256 x 256 tile runs from 200 tiles on: 15 x 14 of them, ragged in M."""
    M, N, K, fmt = 3590, 3584, 256, "mxfp6"
    ab, kw, want = rowscale_case(dev, M, N, K, fmt, seed=5)
    out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
    assert ops.gemm_mx_plan(*ab, out, fmt, **kw)["path"] == "t256x256"
    ops.gemm_mx(*ab, out, fmt, **kw)
    assert_exact(out, want, "gemm_mx mxfp6 t256x256")


@pytest.mark.parametrize("fmt,kernel", [("mxfp8", 2), ("mxfp6", 18)])
def test_gemm_mx_call_honours_bias_rowscale(ops, dev, fmt, kernel):
    """260 rows with 512 and 256 as the other two dimensions: the persistent kernel takes K >= 512 only, so K = 512 and
    N = 256 (the plan must say p256); the same call at 300 x 256 x 256 stays on the tiled kernel."""
    for (M, N, K), path in (((260, 256, 512), "p256"), ((300, 256, 256), "t128x128")):
        ab, kw, want = rowscale_case(dev, M, N, K, fmt, seed=M + kernel)
        out = torch.full((M, N), float("nan"), dtype=BF, device=dev)
        assert ops.gemm_mx_call_plan(*ab, out, kernel, fmt, **kw)["path"] == path
        ops.gemm_mx_call(*ab, out, kernel, fmt, **kw)
        assert_exact(out, want, f"gemm_mx_call k{kernel} {fmt} {path}")
    with pytest.raises(ValueError):
        ops.gemm_mx_call(*ab, out, kernel, fmt, out_scales=torch.empty(M, N // 32, dtype=torch.uint8, device=dev),
                         bias_rowscale=kw["bias_rowscale"])


# ------------------------------------------------------------------------------------------ 6. the pair as the next operand
@pytest.mark.parametrize("fmt,w_fmt", [("mxfp6", "mxfp6"), ("mxfp8", "mxfp4")])
def test_fused_pair_is_a_legal_operand_of_the_next_gemm(ops, dev, fmt, w_fmt):
    D, H, Sq, grp, N = 128, 2, 150, 2, 384
    E = H * D
    q, k, v, r, af, kw = mix_case(dev, "audio", D, H, 2, grp, Sq, 32)
    z, ws, ref = the_pair(ops, dev, q, k, v, r, af, kw)
    g = torch.Generator().manual_seed(5)
    wc, wsc = ops.quantize_mx((torch.randn(N, E, generator=g) * E ** -0.5).to(BF).to(dev), w_fmt)
    bias = torch.randn(N, generator=g).to(BF).to(dev)
    codes, scales = pair(ops, (grp * Sq,), E, fmt, dev)
    ops.attn_kv_mix(q, k, v, r, af, None, None, mx_out=(codes, scales, fmt), **kw)
    y0, y1 = torch.empty(grp * Sq, N, dtype=BF, device=dev), torch.empty(grp * Sq, N, dtype=BF, device=dev)
    ops.gemm_mx(*ref[fmt], wc, wsc, y0, fmt, w_fmt=w_fmt, bias=bias, bias_rowscale=ws)
    ops.gemm_mx(codes, scales, wc, wsc, y1, fmt, w_fmt=w_fmt, bias=bias, bias_rowscale=ws)
    assert bool(torch.isfinite(y0.float()).all()) and torch.equal(y0, y1)


# ------------------------------------------------------------------------------------------ 7. engine
@pytest.fixture(scope="module")
def small(dev):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    inp = synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True)
    gi = to_dev(inp, dev)
    out_bf16 = model(**gi)[0].clone()
    four = {}
    for fmt in FORMATS:
        model.enable_mx_weights(fmt)
        four[fmt] = model(**gi)[0].clone()
    model.enable_mx_weights(enabled=False)
    return model, inp, gi, out_bf16, four


def counted_forward(model, gi, monkeypatch):
    """-> (output, quantize_mx calls, kv-mix launches that wrote MX codes, kv-mix launches) of one step."""
    from bind_your_avatar_implementation_amd import ops
    model(**gi)                                                                           # builds the engine (packs weights)
    with monkeypatch.context() as mp:
        qz, mix = Counter(ops.quantize_mx), Counter(ops.attn_kv_mix)
        mp.setattr(ops, "quantize_mx", qz)
        mp.setattr(ops, "attn_kv_mix", mix)
        out = model(**gi)[0].clone()
    return out, qz.n, mix.mx, mix.n


def test_engine_packs_the_six_kinds(small, dev):
    model, inp, gi, out_bf16, four = small
    try:
        for fmt, wf, bits in (("mxfp8", None, 8), ("mxfp6", None, 6), ("mxfp8", "mxfp4", 4)):
            model.enable_mx_weights(fmt, linears=SIX, weight_format=wf)
            model(**gi)
            eng = model._engine
            assert set(eng.wmx) == set(SIX) and eng.w8 is None and eng.mx_fuse_cross_quant
            c, s = eng.wmx["po"][0]
            assert c.shape == (3072, 2048 * bits // 8) and s.shape == (3072, 64) and len(eng.wmx["po"]) == 1
            c, s = eng.wmx["ao"][1]
            assert c.shape == (3072, 3072 * bits // 8) and s.shape == (3072, 96) and len(eng.wmx["ao"]) == 2
        model.enable_mx_weights("mxfp8", linears="qkv,po")
        model(**gi)
        assert set(model._engine.wmx) == {"qkv", "po"}
        model.enable_mx_weights("mxfp8", linears="all")
        model(**gi)
        assert set(model._engine.wmx) == {"qkv", "out", "ff1", "ff2", "pq", "aq"}
        model.enable_fp8_weights(linears=("ff1", "po"))
        model.enable_mx_weights(enabled=False)
        with pytest.raises(ValueError, match="fp8 linears"):
            model(**gi)
    finally:
        model.enable_fp8_weights(False)
        model.enable_mx_weights(enabled=False)


@pytest.mark.parametrize("fmt,kw", [("mxfp6", {}), ("mxfp8", {}), ("mxfp8", dict(persistent_gemm="always")),
                                    ("mxfp6", dict(persistent_gemm_mxfp6="always")),
                                    ("mxfp8", dict(weight_format="mxfp4", persistent_gemm="always"))],
                         ids=["mxfp6", "mxfp8", "mxfp8-p256", "mxfp6-p256", "mxfp8xfp4-p256"])
def test_engine_kv_mix_feeds_to_out_directly(small, dev, monkeypatch, fmt, kw):
    """fuse_cross_attention_quant=True against False: the same bits, one quantize_mx fewer per cross-attention (1 perceiver
    + 2 audio layers in this 2-layer model), hipGraph replay equal to eager, and the mode off restores the bf16 engine."""
    model, inp, gi, out_bf16, four = small
    cross = 1 + 2
    try:
        model.enable_mx_weights(fmt, linears=SIX, fuse_cross_attention_quant=False, **kw)
        off, q_off, mx_off, n_off = counted_forward(model, gi, monkeypatch)
        assert not model._engine.mx_fuse_cross_quant and mx_off == 0
        model.enable_mx_weights(fmt, linears=SIX, **kw)                                   # on by default
        assert model._engine is None
        on, q_on, mx_on, n_on = counted_forward(model, gi, monkeypatch)
        print(f"{fmt} {kw}: quantize_mx calls {q_off} -> {q_on}, kv-mix launches {n_off} -> {n_on}, of them MX {mx_off} -> {mx_on}")
        assert torch.equal(on, off)
        B = gi["hidden_states"].shape[0]
        assert q_off - q_on == cross and n_on == n_off == cross * B and mx_on == n_on
        drift4 = rel_fro(on.float(), four[fmt].float())
        print(f"{fmt} {kw}: six kinds vs the default four {drift4:.3e}")
        if not kw:
            assert drift4 > 1e-3                                                          # the new kinds were in use
        model.use_hip_graph = True
        try:
            model(**gi)                                                                   # capture
            for _ in range(2):
                assert torch.equal(model(**gi)[0], on)
        finally:
            model.use_hip_graph = False
            model._graphs = {}
        # the default linears: nothing changes for a caller who does not ask, whatever the switch says
        if not kw:
            model.enable_mx_weights(fmt, fuse_cross_attention_quant=False)
            a, qa, mxa, _ = counted_forward(model, gi, monkeypatch)
            model.enable_mx_weights(fmt)
            b, qb, mxb, _ = counted_forward(model, gi, monkeypatch)
            assert set(model._engine.wmx) == {"qkv", "out", "ff1", "ff2"} and mxa == mxb == 0 and qa == qb
            assert torch.equal(a, four[fmt]) and torch.equal(b, four[fmt])
    finally:
        model.enable_mx_weights(fmt, enabled=False)
    assert model._engine is None
    assert torch.equal(model(**gi)[0], out_bf16)                                          # and back: bit-identical bf16 engine


def test_unfused_arms_quantise_their_operand(small, dev, monkeypatch):
    """BYA_FUSED_ATTN_MIX=0 (attention, routed mix, to_out) and BYA_MIX_BEFORE_PROJECTION=0 (project every identity, then
    combine): with the six kinds the bf16 operand each arm hands to to_out goes through quantize_mx -- three calls more than
    the same arm with the default four (1 perceiver + 2 audio layers), no kv-mix launch, and an output that moved."""
    model, inp, gi, out_bf16, four = small
    try:
        for var in ("BYA_FUSED_ATTN_MIX", "BYA_MIX_BEFORE_PROJECTION"):
            with monkeypatch.context() as mp:
                mp.setenv(var, "0")
                model.enable_mx_weights("mxfp8")
                base, q4, _, n4 = counted_forward(model, gi, monkeypatch)
                model.enable_mx_weights("mxfp8", linears=SIX)
                out, q6, mx6, n6 = counted_forward(model, gi, monkeypatch)
                assert set(model._engine.wmx) == set(SIX)
            e = rel_fro(out.float(), base.float())
            print(f"{var}=0: quantize_mx calls {q4} (default four) -> {q6} (six kinds), kv-mix launches {n4} / {n6}, "
                  f"six kinds vs default four {e:.3e}")
            assert n4 == n6 == 0 and mx6 == 0 and q6 - q4 == 3
            assert bool(torch.isfinite(out.float()).all()) and e > 1e-3
    finally:
        model.enable_mx_weights(enabled=False)


# Upper caps of the 2-layer output drift, engine(MX, six kinds) against engine(bf16), on this test's random-init model, set as
# DRIFT_CAP of tests/test_mx_gpu.py was: about twice what the engine measured on an MI355X (mxfp8 3.72e-2, mxfp6 3.44e-2; the
# default four in the same run: 1.43e-2 both).  The floor shows the mode was in use.
DRIFT_CAP_SIX = {"mxfp6": 7e-2, "mxfp8": 7e-2}


@pytest.mark.parametrize("fmt", FORMATS)
def test_forward_with_mx_cross_out_vs_fake_quantised_oracle(small, dev, fmt):
    """The engine with the six kinds against the CPU oracle whose DiT Linears AND two cross-attention to_out modules are
    replaced by the MX definition, at taps face0, audio0, audio1 and at the output: err(engine, fp32 oracle) <= 1.5 x
    err(oracle run in bf16, fp32 oracle) + 1e-3.  The oracle projects each identity and then combines, the engine mixes and
    then projects; quantisation does not commute with a soft mix, so the routing is forced hard (the inputs of
    test_small_geometry_forcing_bit_exact_indexing): every mixing weight is exactly 0 or 1 -- checked first, on the oracle's
    own weight functions."""
    from oracle.model import OracleTransformer, audio_weights, forcing_over_frames
    from test_forward_gpu import SMALL_KW, to_dev
    model, inp, gi, out_bf16, four = small
    T, ht, wt = 3, 8, 12
    lab = torch.full((T, ht, wt), -1)
    lab[0, 1:5, 0:5] = 0
    lab[1, 2:6, 1:6] = 0
    lab[2, 3:7, 7:12] = 1
    lab = lab.reshape(-1)
    forcing = torch.zeros(1, T * ht * wt, 2)
    forcing[0, lab == 0, 0] = 1
    forcing[0, lab == 1, 1] = 1
    inp2 = dict(inp)
    inp2["af_matrix"] = (1 - torch.eye(2))[None].repeat(2, 1, 1)
    for dt in (torch.float32, BF):
        w_face = forcing_over_frames(forcing.to(dt), (T, ht, wt))
        av = (inp2["af_matrix"][:1].to(dt) @ w_face.transpose(-2, -1)).transpose(-2, -1)
        w_audio = audio_weights(av)
        for w in (w_face, w_audio):
            assert bool(((w == 0) | (w == 1)).all())
    sd = {k: v.float().cpu() for k, v in model.state_dict().items()}
    with torch.device("meta"):
        orc = OracleTransformer(**SMALL_KW)
    orc = orc.to_empty(device="cpu")
    orc.load_state_dict(sd, strict=True)
    orc.eval()
    taps32, taps16, tapsg = {}, {}, {}
    with torch.no_grad():
        orc = with_mx_dit_linears(orc, fmt)
        for pc in orc.perceiver_cross_attention:
            pc.to_out = FakeMXLinear(pc.to_out, fmt)
        for al in orc.audio_model.layers:
            al["attn"].to_out[0] = FakeMXLinear(al["attn"].to_out[0], fmt)
        ref = orc(taps=taps32, routing_logits_forcing=forcing, **inp2)[0]
        orc16 = orc.to(BF)
        inp16 = {k: (v.to(BF) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp2.items()}
        inp16["id_cond"] = [t.to(BF) for t in inp2["id_cond"]]
        inp16["id_vit_hidden"] = [[t.to(BF) for t in l] for l in inp2["id_vit_hidden"]]
        ref16 = orc16(taps=taps16, routing_logits_forcing=forcing, **inp16)[0]
    gi2 = to_dev(inp2, dev)
    f_dev = forcing.to(dev, BF)
    try:
        model.enable_mx_weights(fmt, linears=SIX)
        out = model(routing_logits_forcing=f_dev, **gi2)[0]
        assert set(model._engine.wmx) == set(SIX)
        model._engine.step(gi2["hidden_states"], gi2["encoder_hidden_states"], gi2["timestep"], gi2["image_rotary_emb"],
                           gi2["id_cond"], gi2["id_vit_hidden"], gi2["audio_embeds"], gi2["af_matrix"], f_dev, taps=tapsg)
        plain = model(**gi)[0].float().cpu()
    finally:
        model.enable_mx_weights(fmt, enabled=False)
    figures = []
    for name in ["face0", "audio0", "audio1"]:
        g, r32, r16 = tapsg[name].float().cpu(), taps32[name].float(), taps16[name].float()
        figures.append((name, rel_fro(g, r32), rel_fro(r16, r32)))
    figures.append(("output", rel_fro(out, ref), rel_fro(ref16, ref)))
    for name, e_g, e_16 in figures:
        print(f"{name:8s} engine({fmt}, six)-vs-fp32({fmt}) {e_g:.3e}   bf16({fmt})-oracle-vs-fp32({fmt}) {e_16:.3e}")
    drift, drift4 = rel_fro(plain, out_bf16.float().cpu()), rel_fro(four[fmt].float().cpu(), out_bf16.float().cpu())
    print(f"{fmt} six kinds vs bf16 engine after 2 layers: {drift:.3e} (cap {DRIFT_CAP_SIX[fmt]:.1e}); default four, same run: {drift4:.3e}")
    for name, e_g, e_16 in figures:
        assert e_g <= 1.5 * e_16 + 1e-3, name
    assert 1e-3 < drift < DRIFT_CAP_SIX[fmt]


# ------------------------------------------------------------------------------------------ 8. sharded
def _sp_mx_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # 2 ranks share the single test GPU
    try:
        from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
        from bind_your_avatar_implementation_amd.parallel import shard_sequence
        from bind_your_avatar_implementation_amd.synth import synth_inputs
        from test_forward_gpu import SMALL_KW, to_dev
        dev = torch.device("cuda:0")
        hw = (18, 22)
        model = BindyouravatarTransformer3DModel(**dict(SMALL_KW, sample_height=hw[0], sample_width=hw[1]), device=dev)
        model.init_synthetic(seed=1, fast=True)
        inp = to_dev(synth_inputs(batch=1, frames=3, height=hw[0], width=hw[1], seed=3, n_id=2), dev)
        model.enable_mx_weights("mxfp8", linears=SIX)
        full = model(**inp)[0].clone()
        shard_sequence(model, dist.group.WORLD, transport="p2p")
        calls = []
        real = ops.attn_kv_mix
        ops.attn_kv_mix = lambda *a, **k: (calls.append((k["Sq"], k.get("mx_out") is not None)), real(*a, **k))[1]
        try:
            fused = model(**inp)[0].clone()
        finally:
            ops.attn_kv_mix = real
        again = model(**inp)[0].clone()
        model.enable_mx_weights("mxfp8", linears=SIX, fuse_cross_attention_quant=False)      # (rebuilds the engine; still sharded)
        unfused = model(**inp)[0].clone()
        timeouts = model._seq_p2p.timeouts()
        ret[rank] = (float((fused.float() - full.float()).abs().max()), bool(torch.equal(fused, unfused)),
                     bool(torch.equal(again, fused)), timeouts, len(calls), all(mx for _, mx in calls),
                     len({sq for sq, _ in calls}))
    finally:
        dist.destroy_process_group()


def test_sharded_step_with_the_fused_epilogue(dev):
    """2 ranks on the one GPU, hw (18, 22) (shards that differ by a row, frames cut by the shard boundary), p2p transport, mxfp8
    with the six kinds: the per-segment kv-mix launches write their rows of the MX pair -- bit for bit the sharded step with
    fuse_cross_attention_quant=False, within 2e-2 of the unsharded MX step, repeatable, no P2P time-outs."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_sp_mx_worker, args=(2, 29700 + os.getpid() % 1000 + 61, ret), nprocs=2, join=True)
    print("sharded MX step, six kinds (max abs vs unsharded, == unfused, repeatable, time-outs, kv-mix launches, all MX, distinct "
          "segment lengths):", dict(ret))
    for r in (0, 1):
        assert ret[r][0] <= 2e-2, ret[r]
        assert ret[r][1] and ret[r][2] and ret[r][3] == 0, ret[r]
        assert ret[r][4] >= 3 and ret[r][5], ret[r]                         # every kv-mix launch went through the MX epilogue
    # (rank 0 holds the text rows and 35 video rows of frame 0: one segment; rank 1's rows span all three frames)
    assert max(ret[r][4] for r in (0, 1)) > 3 and max(ret[r][6] for r in (0, 1)) > 1, dict(ret)
