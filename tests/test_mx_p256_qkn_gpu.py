"""The MX q|k|v projection whose epilogue norms and rotates q and k, on the persistent one-wave-per-SIMD 256 x 256 kernel
(csrc/gemm_mx_v4.hip, gemm256p_mx_kernel<MX_EPI_QKN>; bya_gemm_mx_qkv_norm_rope_on, ops.gemm_mx_qkv_norm_rope(..., kernel=)):
bit for bit bya_gemm_mx(..., n_split) followed by bya_qknorm_rope AND the fused launch on the tiled kernel -- on shapes whose
waves straddle q | k and k | v, with ragged row and column tiles, more tiles than workgroups, with and without bias, for
q | k alone, in the column-block form, batched, with canaries behind the rows, between the split tensors and behind the last
column; the fallbacks; and the engine's step with enable_mx_weights("mxfp8", persistent_gemm=..., fuse_qk_norm=True).
No tolerance anywhere: every comparison is torch.equal on bit patterns, and the plan is asserted before every launch."""
import ctypes

import pytest
import torch

from test_mx_p256_gpu import Recorder
from test_mx_qkn_gpu import (BITS, CODE, EPS, K_SCALE, PAD, Counter, bits, check_equal_and_canaries, nan_buffer, norm_params,
                             operands, pair_and_fused)

pytestmark = pytest.mark.gpu
FMT = "mxfp8"


def fused_on(dev, ac, asc, wc, wsc, bias, M, width, text, kernel, expect, tensors=3, fmt=FMT, w_fmt=FMT):
    """The fused launch under ``kernel`` into a NaN-filled [tensors + 1, M + PAD, width] buffer (pair_and_fused's layout);
    the plan is asserted first."""
    from bind_your_avatar_implementation_amd import ops
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    one = nan_buffer(dev, tensors + 1, M + PAD, width)
    args = (ac, asc, wc, wsc, one[0, :M], bias, (width, (M + PAD) * width), qw, qb, kw, kb, cos, sin, text)
    kw_ = dict(eps=EPS, k_scale=K_SCALE, tensors=tensors, fmt=fmt, w_fmt=w_fmt, kernel=kernel)
    plan = ops.gemm_mx_qkv_norm_rope_plan(*args, **kw_)
    assert plan is not None and plan["path"] == expect and plan["row_chunks"] == 1, plan
    assert ops.gemm_mx_qkv_norm_rope(*args, **kw_) is True
    torch.cuda.synchronize()
    return one


# (M, width, K, text rows, kernel).  K = 512 is the shortest K the kernel takes: each K-tile variant A / B / C / D runs once.
#  * a ragged row tile, the text / video boundary inside a 16-row fragment, the second column tile half empty;
#  * q | k at column 192 inside a wave's 128 columns, the last tile 64 columns wide (a wave with one live head), fewer rows
#    than a fragment;
#  * all text: cos / sin None;
#  * 18 x 15 = 270 tiles, above the 256 workgroups of the grid: some workgroups run the epilogue and then a second tile whose
#    first K-tiles were requested under it; q | k at 1216 and k | v at 2432 inside waves; a quarter-full last column tile.
SHAPES = [(300, 128, 512, 40, 2), (17, 192, 512, 0, 2), (300, 192, 512, 300, 2), (4400, 1216, 512, 226, 1)]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,width,K,text,kernel", SHAPES)
def test_fused_p256_equals_two_launches_and_fused_tiled(dev, M, width, K, text, kernel, with_bias):
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, FMT, FMT)
    bias = bias if with_bias else None
    two, tiled = pair_and_fused(dev, ac, asc, wc, wsc, bias, FMT, FMT, M, width, text, expect="t128x128")
    one = fused_on(dev, ac, asc, wc, wsc, bias, M, width, text, kernel, "p256")
    check_equal_and_canaries(two, one, M, 3)
    assert torch.equal(bits(one), bits(tiled))
    assert float(one[:3, :M].float().abs().sum()) > 0
    if M == 300 and width == 128:
        # kernel = 0 through the new argument is the old entry point
        assert torch.equal(bits(fused_on(dev, ac, asc, wc, wsc, bias, M, width, text, 0, "t128x128")), bits(tiled))


def test_q_and_k_alone(dev):
    """tensors = 2: N = 2 width, the first two thirds of the packed weight; columns past N belong to no tensor."""
    M, width, K, text = 300, 192, 512, 40
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, FMT, FMT)
    wc2, wsc2, bias2 = wc[:2 * width].contiguous(), wsc[:2 * width].contiguous(), bias[:2 * width].contiguous()
    two, _ = pair_and_fused(dev, ac, asc, wc2, wsc2, bias2, FMT, FMT, M, width, text, tensors=2)
    one = fused_on(dev, ac, asc, wc2, wsc2, bias2, M, width, text, 2, "p256", tensors=2)
    check_equal_and_canaries(two, one, M, 2)
    three = fused_on(dev, ac, asc, wc, wsc, bias, M, width, text, 2, "p256")
    assert torch.equal(three[:2, :M], one[:2, :M])


def test_column_block_form(dev):
    """The head-parallel sharded step's layout: n_split = width / 4, column block t * 4 + j = tensor t, heads of rank j, each
    [M, width / 4] at c_split_stride; bya_qknorm_rope sees the q and k blocks as a batch of 4."""
    from bind_your_avatar_implementation_amd import ops
    M, width, K, text, W = 300, 256, 512, 40, 4
    Dl = width // W
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, FMT, FMT)
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    two, one = nan_buffer(dev, 3 * W + 1, M + PAD, Dl), nan_buffer(dev, 3 * W + 1, M + PAD, Dl)
    split = (Dl, (M + PAD) * Dl)
    ops.gemm_mx(ac, asc, wc, wsc, two[0, :M], FMT, bias=bias, split=split)
    ops.qknorm_rope(two[:W, :M], two[W:2 * W, :M], qw, qb, kw, kb, cos, sin, heads=Dl // 64, text_rows=text, eps=EPS,
                    k_scale=K_SCALE)
    args = (ac, asc, wc, wsc, one[0, :M], bias, split, qw, qb, kw, kb, cos, sin, text)
    plan = ops.gemm_mx_qkv_norm_rope_plan(*args, eps=EPS, k_scale=K_SCALE, fmt=FMT, kernel=2)
    assert plan["path"] == "p256", plan
    assert ops.gemm_mx_qkv_norm_rope(*args, eps=EPS, k_scale=K_SCALE, fmt=FMT, kernel=2) is True
    torch.cuda.synchronize()
    check_equal_and_canaries(two, one, M, 3 * W)


def test_batched_operands_with_batch_strides(dev):
    """batch = 2 with batch strides larger than the matrices, through the C ABI: A codes advance by a_batch_stride, C by
    c_batch_stride, the scale rows of entry z are z * M + m (dense), and the rotary row is the row of the batch entry."""
    from bind_your_avatar_implementation_amd import _hip, ops
    M, width, K, text = 300, 192, 512, 40
    ac0, asc0, wc, wsc, bias = operands(dev, M, 3 * width, K, FMT, FMT)
    ac1, asc1 = operands(dev, M, 3 * width, K, FMT, FMT, seed=1)[:2]
    lda = ac0.shape[1]
    a_bs, c_bs = M * lda + 160, (M + PAD) * width
    abuf = torch.zeros(2 * a_bs, dtype=torch.uint8, device=dev)
    abuf[:M * lda] = ac0.reshape(-1)
    abuf[a_bs:a_bs + M * lda] = ac1.reshape(-1)
    sa = torch.cat([asc0, asc1]).contiguous()
    one = nan_buffer(dev, 4, 2, M + PAD, width)                                           # [tensor, batch, rows, width]
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    d, n, p = ops.GemmDesc(), _hip.QkNormDesc(), _hip.GemmPlan()
    d.M, d.N, d.K, d.batch = M, 3 * width, K, 2
    d.lda, d.ldw, d.ldc = K * BITS[FMT] // 8, K * BITS[FMT] // 8, width
    d.a_batch_stride, d.c_batch_stride = a_bs, c_bs
    d.n_split, d.c_split_stride, d.alpha = width, 2 * c_bs, 1.0
    n.qw, n.qb, n.kw, n.kb, n.cos, n.sin = (t.data_ptr() for t in (qw, qb, kw, kb, cos, sin))
    n.text_rows, n.width, n.eps, n.k_scale = text, width, EPS, K_SCALE
    args = (abuf.data_ptr(), sa.data_ptr(), wc.data_ptr(), wsc.data_ptr(), bias.data_ptr(), one.data_ptr(), CODE[FMT], CODE[FMT],
            ctypes.byref(d), ctypes.byref(n))
    lib = _hip.load()
    assert lib.bya_gemm_mx_qkv_norm_rope_on_plan(*args, 2, ctypes.byref(p)) == 0 and p.path == 4 and p.row_chunks == 1
    assert lib.bya_gemm_mx_qkv_norm_rope_on(*args, 2, ops._stream()) == 0
    torch.cuda.synchronize()
    for z, (a_c, a_s) in enumerate(((ac0, asc0), (ac1, asc1))):
        two, _ = pair_and_fused(dev, a_c, a_s, wc, wsc, bias, FMT, FMT, M, width, text)
        assert torch.equal(bits(one[:, z]), bits(two))
    assert not torch.equal(one[0, 0, :M], one[0, 1, :M])
    # and the front end's own batch form (evenly stacked entries)
    front = nan_buffer(dev, 3, 2, M, width)
    fargs = (torch.stack([ac0, ac1]), torch.stack([asc0, asc1]), wc, wsc, front[0], bias, (width, 2 * M * width), qw, qb, kw, kb,
             cos, sin, text)
    assert ops.gemm_mx_qkv_norm_rope_plan(*fargs, eps=EPS, k_scale=K_SCALE, fmt=FMT, kernel=2)["path"] == "p256"
    assert ops.gemm_mx_qkv_norm_rope(*fargs, eps=EPS, k_scale=K_SCALE, fmt=FMT, kernel=2)
    assert torch.equal(front, one[:3, :, :M])


@pytest.mark.parametrize("fmt,w_fmt,kernel", [("mxfp8", "mxfp4", 2), ("mxfp6", "mxfp6", 2), ("mxfp8", "mxfp8", 1)])
def test_fallbacks_run_the_tiled_kernel(dev, fmt, w_fmt, kernel):
    """e2m1 weights and e2m3 operands under kernel = 2, and 300 rows (2 x 3 tiles) under kernel = 1: the plan is the tiled
    kernel and the launch is the existing entry point's."""
    M, width, K, text = 300, 192, 512, 40
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, fmt, w_fmt)
    two, tiled = pair_and_fused(dev, ac, asc, wc, wsc, bias, fmt, w_fmt, M, width, text, expect="t128x128")
    one = fused_on(dev, ac, asc, wc, wsc, bias, M, width, text, kernel, "t128x128", fmt=fmt, w_fmt=w_fmt)
    check_equal_and_canaries(two, one, M, 3)
    assert torch.equal(bits(one), bits(tiled))


# ------------------------------------------------------------------------------------------ engine
def recorded_forward(model, gi, monkeypatch):
    """One step with every fused q|k|v launch's plan recorded and the stand-alone q/k-norm launches counted."""
    from bind_your_avatar_implementation_amd import ops
    model(**gi)                                                                           # builds the engine (packs weights)
    with monkeypatch.context() as mp:
        f, n = Recorder(ops.gemm_mx_qkv_norm_rope, ops.gemm_mx_qkv_norm_rope_plan), Counter(ops.qknorm_rope)
        mp.setattr(ops, "gemm_mx_qkv_norm_rope", f)
        mp.setattr(ops, "qknorm_rope", n)
        out = model(**gi)[0].clone()
    return out, f.paths, n.n


def replay_equals(model, gi, want):
    model.use_hip_graph = True
    try:
        model(**gi)                                                                       # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], want)
    finally:
        model.use_hip_graph = False
        model._graphs = {}


def test_engine_both_switches_issue_qkv_as_one_persistent_launch(dev, monkeypatch):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    model.enable_mx_weights("mxfp8")
    off, f_off, n_off = recorded_forward(model, gi, monkeypatch)
    assert f_off == [] and model._engine.mx_kernel == 0
    # (the condition of the counts below: no layer of this model asks for the norm statistics, which keep the two launches)
    assert all(b <= ops.ATTN_BOUND_LIMIT for b in model._engine.score_bound)
    model.enable_mx_weights("mxfp8", persistent_gemm="always", fuse_qk_norm=True)
    assert model._engine is None                                                          # the switches invalidate the engine
    on, f_on, n_on = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_kernel == 2 and model._engine.mx_fuse_qk_norm
    print(f"gemm_mx_qkv_norm_rope plans {f_on}; qknorm_rope calls {n_off} -> {n_on}; {blocks} blocks")
    assert f_on == ["p256"] * blocks and n_off - n_on == blocks
    assert torch.equal(on, off)
    replay_equals(model, gi, off)
    # with the attention writing to_out's operand too
    model.enable_mx_weights("mxfp8", persistent_gemm="always", fuse_qk_norm=True, fuse_attention_quant=True)
    both, f_both, _ = recorded_forward(model, gi, monkeypatch)
    assert f_both == ["p256"] * blocks and torch.equal(both, off)
    replay_equals(model, gi, off)
    # mxfp6: persistent_gemm changes no launch of the fused projection
    model.enable_mx_weights("mxfp6", fuse_qk_norm=True)
    ref6, f6, n6 = recorded_forward(model, gi, monkeypatch)
    model.enable_mx_weights("mxfp6", persistent_gemm="always", fuse_qk_norm=True)
    got6, f6p, n6p = recorded_forward(model, gi, monkeypatch)
    assert model._engine.mx_kernel == 0 and len(f6p) == blocks and f6p == f6 and "p256" not in f6p and n6p == n6
    assert torch.equal(got6, ref6)
