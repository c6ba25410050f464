"""The q/k score-bound statistics recorded by the fused q|k|v launches (the *_stats entry points, include/bya.h; epilogue_qkn and
epilogue_mx_wide8_qkn with STATS, csrc/gemm_wide_epilogue.h): with the same inputs and a zeroed table the ONE launch must give
  * C (q, k, v) bit for bit what the projection followed by qknorm_rope(..., stats=...) gives,
  * a table whose maximum over the slots equals that path's maximum over the slots, bit for bit, and equals the CPU
    restatement computed from the stored bf16 q and k (tests/qkn_stats_ref.py),
  * nothing outside the table: the row behind its last slot keeps its canary.
The raw per-slot tables need not agree (the workgroup-to-slot assignment differs).  No tolerance anywhere.  Operands as in the
existing q/k-norm tests (K = 512, k_scale = 0.18); a few elements of the k gain are multiplied by 5 and of the q gain by 2."""
import pytest
import torch

import qkn_stats_ref
from qkn_stats_ref import bits32

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
K, K_SCALE, EPS, CANARY = 512, 0.18, 1e-6, 12345.0


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


_CACHE = {}


def norm_params(dev, M, text):
    """LayerNorm vectors with a few large gains and the rotary tables of one row count, built once."""
    key = ("norm", M, text)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(M + text)
        qw, qb, kw, kb = ((torch.randn(64, generator=g) * 0.3 + (1 if i % 2 == 0 else 0)) for i in range(4))
        qw[[5, 33]] *= 2.0
        kw[[3, 17, 40]] *= 5.0
        ang = torch.rand(M - text, 64, generator=g) * 6.3
        _CACHE[key] = (*(t.to(BF).to(dev) for t in (qw, qb, kw, kb)), torch.cos(ang).to(dev).contiguous(), torch.sin(ang).to(dev).contiguous())
    return _CACHE[key]


def bf16_operands(dev, B, M, width):
    """x [B, M, K], w [3 width, K], bias [3 width]: gaussian, built once per shape."""
    key = ("bf16", B, M, width)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(B * 100000 + M + width)
        _CACHE[key] = (torch.randn(B, M, K, generator=g).to(BF).to(dev), (torch.randn(3 * width, K, generator=g) * K ** -0.5).to(BF).to(dev),
                       (torch.randn(3 * width, generator=g) * 0.5).to(BF).to(dev))
    return _CACHE[key]


def tables(dev, slots, nbh):
    """Two zeroed tables [slots, 2, nbh], each with one more row behind it that holds a canary."""
    full = torch.zeros(2, slots + 1, 2, nbh, dtype=torch.float32, device=dev)
    full[:, slots] = CANARY
    return full, full[0, :slots], full[1, :slots]


def check_tables(full, pair, fused, q, k, what):
    """The three equalities on the table (q, k: the stored rows as [batch, rows, heads * 64]) and the canary rows."""
    torch.cuda.synchronize()
    want = qkn_stats_ref.table(q, k)
    assert want.shape == tuple(pair.shape[1:]), (want.shape, pair.shape)
    got_pair, got_fused = pair.amax(0), fused.amax(0)
    assert torch.equal(bits32(got_pair), bits32(want)), f"{what}: the two-launch table is not the restatement's"
    diff = bits32(got_fused) != bits32(got_pair)
    assert not bool(diff.any()), (f"{what}: {int(diff.sum())} table entries differ from the two-launch path's, first at "
                                  f"{diff.nonzero()[0].tolist()}: {got_fused[diff][0].item()!r} != {got_pair[diff][0].item()!r}")
    assert torch.equal(bits32(got_fused), bits32(want)), what
    assert bool((want > 0).all()) and len(set(want.reshape(-1).tolist())) > want.numel() // 2      # heads with distinct maxima
    assert bool((full[:, -1] == CANARY).all()), f"{what}: the row behind the table was written"
    assert bool((fused >= 0).all())


def run_bf16(ops, dev, M, width, text, slots, opts, expect, tensors=3, W=1, B=1, pad=0):
    """One case on the bf16 entry point: dense (W = 1; B batch entries, ``pad`` rows between them: batch strides) or in the
    column-block form of the head-parallel sharded step (W > 1: n_split = width / W)."""
    x, w, bias = bf16_operands(dev, B, M + pad, width)
    x = x[:, :M] if B > 1 else x[0, :M]
    w, bias = w[:tensors * width], bias[:tensors * width]
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    Dl = width // W
    two = torch.zeros(3 * W, B, M + pad, Dl, dtype=BF, device=dev)
    one = torch.full_like(two, float("nan"))
    split = (Dl, B * (M + pad) * Dl)
    view = (lambda t: t[:, :M]) if B > 1 else (lambda t: t[0, :M])
    full, t_pair, t_fused = tables(dev, slots, B * width // 64)
    args = lambda out: (x, w, view(out[0]), bias, split, qw, qb, kw, kb, cos, sin, text)
    kw_ = dict(eps=EPS, k_scale=K_SCALE, tensors=tensors)
    with ops.options(**opts):
        ops.gemm(x, w, view(two[0]), bias=bias, split=split)
        if W == 1:
            ops.qknorm_rope(view(two[0]), view(two[1]), qw, qb, kw, kb, cos, sin, heads=width // 64, text_rows=text, eps=EPS,
                            k_scale=K_SCALE, stats=t_pair)
        else:       # the sharded step's call: the W column blocks of q and of k as a batch of W
            ops.qknorm_rope(two[:W, 0, :M], two[W:2 * W, 0, :M], qw, qb, kw, kb, cos, sin, heads=Dl // 64, text_rows=text, eps=EPS,
                            k_scale=K_SCALE, stats=t_pair)
        plan = ops.gemm_qkv_norm_rope_plan(*args(one), stats=t_fused, **kw_)
        assert plan is not None and ops.plan_key(plan) == expect, plan
        assert ops.gemm_qkv_norm_rope(*args(one), stats=t_fused, **kw_) is True
    torch.cuda.synchronize()
    live = tensors * W
    assert torch.equal(bits(one[:live, :, :M]), bits(two[:live, :, :M])), f"{expect}: C differs from the two launches'"
    assert bool(torch.isnan(one[:live, :, M:]).all()) and bool(torch.isnan(one[live:]).all())       # rows past M, tensors past N
    if W == 1:
        q, k = two[0, :, :M], two[1, :, :M]
    else:           # column block j of a tensor holds heads j * Dl / 64 ..: back to [1, M, width]
        q, k = (two[t * W:(t + 1) * W, 0, :M].permute(1, 0, 2).reshape(1, M, width) for t in (0, 1))
    check_tables(full, t_pair, t_fused, q, k, f"{expect} M={M} width={width} W={W} B={B} slots={slots}")
    return plan


P256, P128 = dict(gemm_tile=4), dict(gemm_tile=5)


@pytest.mark.parametrize("opts,expect", [(P256, "p256"), (P128, "p128")], ids=["p256", "p128"])
@pytest.mark.parametrize("M,width,slots", [(300, 128, 8), (300, 256, 1), (513, 128, 64)])
def test_fused_launch_records_the_two_launch_table(ops, dev, M, width, slots, opts, expect):
    """M = 300: a ragged last row block, rows past M inside the tile, 40 text rows unrotated; M = 513: a second (p256: third)
    row tile with one row.  Slots 1 (every workgroup on one table), 8, and 64 (more slots than workgroups)."""
    run_bf16(ops, dev, M, width, 40, slots, opts, expect)


_TAIL = {}


def smallest_tail_rows(ops, width):
    """The smallest M for which the plan of the q|k|v projection is p256 with a p128 tail (host-side queries on meta tensors)."""
    if width not in _TAIL:
        meta = lambda *s, dtype=BF: torch.empty(*s, dtype=dtype, device="meta")
        v = meta(64)
        for M in range(257, 1 << 16):
            cs = meta(M - 40, 64, dtype=torch.float32)
            plan = ops.gemm_qkv_norm_rope_plan(meta(M, K), meta(3 * width, K), meta(3, M, width)[0], meta(3 * width), (width, M * width),
                                               v, v, v, v, cs, cs, 40, stats=8)
            if plan is not None and plan["tail"] == "p128":
                _TAIL[width] = (M, plan["m0"])
                break
    return _TAIL[width]


def test_row_split_p256_with_a_p128_tail(ops, dev):
    """Two launches (rows [0, m0) on 256-row tiles, the rest on 128-row tiles) raise ONE table."""
    M, m0 = smallest_tail_rows(ops, 1024)
    print(f"smallest M with a p128 tail at width 1024: {M} (m0 = {m0})")
    plan = run_bf16(ops, dev, M, 1024, 40, 8, {}, "p256|p128")
    assert plan["m0"] == m0 and 0 < m0 < M


@pytest.mark.parametrize("opts,expect", [(P256, "p256"), (P128, "p128")], ids=["p256", "p128"])
def test_q_and_k_alone(ops, dev, opts, expect):
    run_bf16(ops, dev, 300, 256, 40, 8, opts, expect, tensors=2)


@pytest.mark.parametrize("opts,expect", [(P256, "p256"), (P128, "p128")], ids=["p256", "p128"])
def test_column_block_form_indexes_the_global_head(ops, dev, opts, expect):
    run_bf16(ops, dev, 300, 256, 40, 16, opts, expect, W=4)


@pytest.mark.parametrize("opts,expect", [(P256, "p256"), (P128, "p128")], ids=["p256", "p128"])
def test_batch_of_two_with_batch_strides(ops, dev, opts, expect):
    """Entry z * heads + head; 8 rows between the batch entries of A and of every output tensor."""
    run_bf16(ops, dev, 300, 128, 40, 8, opts, expect, B=2, pad=8)


# ------------------------------------------------------------------------------------------ the wide-8 kernels
def check_wide8(ops, dev, M, width, text, slots, pair, fused, what):
    """``pair(out, table)`` / ``fused(out, table)`` issue the two launches / the one launch into [3, M, width] buffers."""
    two = torch.zeros(3, M, width, dtype=BF, device=dev)
    one = torch.full_like(two, float("nan"))
    full, t_pair, t_fused = tables(dev, slots, width // 64)
    pair(two, t_pair)
    assert fused(one, t_fused) is True
    torch.cuda.synchronize()
    assert torch.equal(bits(one), bits(two)), f"{what}: C differs from the two launches'"
    check_tables(full, t_pair, t_fused, two[0][None], two[1][None], what)


@pytest.mark.parametrize("w_fmt", ["mxfp8", "mxfp4"])
def test_persistent_mx_kernel_records_its_own_two_launch_table(ops, dev, w_fmt):
    """gemm256p_mx_kernel<MX_EPI_QKN_STATS> at M = 300, kernel argument 2 (without the tile count); width 192: q | k inside a
    wave's 128 columns, the last column tile a quarter full.  mxfp4 weights reach that kernel through gemm_mx_call, whose
    ``norm`` dict carries the table.  The tiled kernel declines a table and launches nothing."""
    from test_mx_qkn_gpu import operands
    M, width, text, fmt = 300, 192, 40, "mxfp8"
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, fmt, w_fmt)
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    split = (width, M * width)

    def pair(out, table):
        ops.gemm_mx(ac, asc, wc, wsc, out[0], fmt, bias=bias, split=split, w_fmt=w_fmt)
        ops.qknorm_rope(out[0], out[1], qw, qb, kw, kb, cos, sin, heads=width // 64, text_rows=text, eps=EPS, k_scale=K_SCALE, stats=table)

    def fused(out, table):
        if w_fmt == "mxfp4":
            norm = dict(qw=qw, qb=qb, kw=kw, kb=kb, cos=cos, sin=sin, text_rows=text, eps=EPS, k_scale=K_SCALE, stats=table)
            args, kw_ = (ac, asc, wc, wsc, out[0], 2, fmt, w_fmt), dict(bias=bias, split=split, norm=norm)
            assert ops.gemm_mx_call_plan(*args, **kw_)["path"] == "p256"
            return ops.gemm_mx_call(*args, **kw_)
        args = (ac, asc, wc, wsc, out[0], bias, split, qw, qb, kw, kb, cos, sin, text)
        kw_ = dict(eps=EPS, k_scale=K_SCALE, fmt=fmt, w_fmt=w_fmt, stats=table)
        assert ops.gemm_mx_qkv_norm_rope_plan(*args, kernel=2, **kw_)["path"] == "p256"
        # the tiled kernel does not record the statistics: declined, nothing written
        assert ops.gemm_mx_qkv_norm_rope_plan(*args, kernel=0, **kw_) is None
        assert ops.gemm_mx_qkv_norm_rope(*args, kernel=0, **kw_) is False
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and not bool(table.any())
        return ops.gemm_mx_qkv_norm_rope(*args, kernel=2, **kw_)

    check_wide8(ops, dev, M, width, text, 8, pair, fused, f"mx p256 {fmt}*{w_fmt}")


def test_persistent_fp8_kernel_records_its_own_two_launch_table(ops, dev):
    """gemm256p_fp8_qkn_stats_kernel at M = 300.  bya_gemm_fp8 takes its persistent kernel from 200 tiles of 256 x 256 on, so
    the launch is 134 heads wide (2 x 101 tiles); a narrow launch runs the tiled kernel, which declines a table."""
    M, width, text = 300, 134 * 64, 40
    g = torch.Generator().manual_seed(11)
    a8, sa = ops.quantize_rows_fp8(torch.randn(M, K, generator=g).to(BF).to(dev))
    w8, sw = ops.quantize_rows_fp8((torch.randn(3 * width, K, generator=g) * K ** -0.5).to(BF).to(dev))
    bias = (torch.randn(3 * width, generator=g) * 0.5).to(BF).to(dev)
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    split = (width, M * width)

    def pair(out, table):
        assert ops.gemm_fp8_plan(a8, sa, w8, sw, out[0], bias=bias, split=split)["path"] == "p256"
        ops.gemm_fp8(a8, sa, w8, sw, out[0], bias=bias, split=split)
        ops.qknorm_rope(out[0], out[1], qw, qb, kw, kb, cos, sin, heads=width // 64, text_rows=text, eps=EPS, k_scale=K_SCALE, stats=table)

    def fused(out, table):
        args = (a8, sa, w8, sw, out[0], bias, split, qw, qb, kw, kb, cos, sin, text)
        assert ops.gemm_fp8_qkv_norm_rope_plan(*args, eps=EPS, k_scale=K_SCALE, stats=table)["path"] == "p256"
        return ops.gemm_fp8_qkv_norm_rope(*args, eps=EPS, k_scale=K_SCALE, stats=table)

    check_wide8(ops, dev, M, width, text, 8, pair, fused, "fp8 p256")
    # 2 x 3 tiles: the tiled kernel's launch, which declines a table (and takes the launch without one)
    n = 3 * 128
    small = torch.full((3, M, 128), float("nan"), dtype=BF, device=dev)
    args = (a8, sa, w8[:n].contiguous(), sw[:n].contiguous(), small[0], bias[:n].contiguous(), (128, M * 128), qw, qb, kw, kb, cos, sin, text)
    table = torch.zeros(8, 2, 2, dtype=torch.float32, device=dev)
    assert ops.gemm_fp8_qkv_norm_rope_plan(*args, eps=EPS, k_scale=K_SCALE)["path"] == "t128x128"
    assert ops.gemm_fp8_qkv_norm_rope_plan(*args, eps=EPS, k_scale=K_SCALE, stats=table) is None
    assert ops.gemm_fp8_qkv_norm_rope(*args, eps=EPS, k_scale=K_SCALE, stats=table) is False
    torch.cuda.synchronize()
    assert bool(torch.isnan(small).all()) and not bool(table.any())
