"""The fp8 q|k|v projection whose epilogue norms and rotates q and k (include/bya.h, bya_gemm_fp8_qkv_norm_rope;
ops.gemm_fp8_qkv_norm_rope): bit for bit bya_gemm_fp8(..., n_split) followed by bya_qknorm_rope ON THE SAME KERNEL PATH -- the
128 x 128 tiled kernel and the persistent 256 x 256 one, on Gaussian operands (the row x channel scale, then the bias, then ONE
rounding to bf16: a fused multiply-add across the first two would show here), on shapes whose tiles and waves straddle the q | k
and k | v boundaries, with and without bias, batched, for q | k alone, in the sharded step's column-block form, with canaries
behind the rows, behind the last column tile and between the split tensors, and in the engine
(enable_fp8_weights(fuse_qk_norm=...)).  No tolerance anywhere: every comparison is torch.equal (on the bit patterns where a
buffer holds NaN canaries)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
K_SCALE, EPS, PAD = 0.18, 1e-6, 8
NAN_BITS = torch.tensor(float("nan"), dtype=BF).view(torch.int16).item()
T128, P256 = "t128x128", "p256"


def bits(t):
    return t.contiguous().view(torch.int16)


_OPERANDS, _NORM, _TWO = {}, {}, {}


def operands(dev, M, N, K, seed=0):
    """Gaussian e4m3 operands of one shape, built once: (a8, a scale, w8, w scale, bias)."""
    from bind_your_avatar_implementation_amd import ops
    key = (M, N, K, seed)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(1000 * seed + M + N)
        a = torch.randn(M, K, generator=g).to(BF)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
        bias = (torch.randn(N, generator=g) * 0.5).to(BF).to(dev)
        _OPERANDS[key] = (*ops.quantize_rows_fp8(a.to(dev)), *ops.quantize_rows_fp8(w.to(dev)), bias)
    return _OPERANDS[key]


def norm_params(dev, M, text):
    """LayerNorm vectors and rotary tables (angles in [0, 6.3)) of one row count, built once."""
    key = (M, text)
    if key not in _NORM:
        g = torch.Generator().manual_seed(M + text)
        qw, qb, kw, kb = ((torch.randn(64, generator=g) * 0.3 + (1 if i % 2 == 0 else 0)).to(BF).to(dev) for i in range(4))
        cos = sin = None
        if text < M:
            ang = (torch.rand(M - text, 64, generator=g) * 6.3).to(dev)
            cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
        _NORM[key] = (qw, qb, kw, kb, cos, sin)
    return _NORM[key]


def nan_buffer(dev, *shape):
    return torch.full(shape, float("nan"), dtype=BF, device=dev)


def two_launches(dev, a8, sa, w8, sw, bias, M, width, text, tensors=3, key=None):
    """The reference: gemm_fp8(split) + qknorm_rope into a NaN-filled [tensors + 1, M + PAD, width] buffer (PAD rows behind
    every tensor: the gap between the split tensors; one more tensor: where columns past N would land).  ``key``: computed
    once under that name (with the option state in it) and shared, never written again."""
    from bind_your_avatar_implementation_amd import ops
    if key is not None and key in _TWO:
        return _TWO[key]
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    two = nan_buffer(dev, tensors + 1, M + PAD, width)
    split = (width, (M + PAD) * width)
    ops.gemm_fp8(a8, sa, w8, sw, two[0, :M], bias=bias, split=split)
    ops.qknorm_rope(two[0, :M], two[1, :M], qw, qb, kw, kb, cos, sin, heads=width // 64, text_rows=text, eps=EPS, k_scale=K_SCALE)
    if key is not None:
        _TWO[key] = two
    return two


def fused(dev, a8, sa, w8, sw, bias, M, width, text, tensors=3, expect=None):
    from bind_your_avatar_implementation_amd import ops
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    one = nan_buffer(dev, tensors + 1, M + PAD, width)
    split = (width, (M + PAD) * width)
    args = (a8, sa, w8, sw, one[0, :M], bias, split, qw, qb, kw, kb, cos, sin, text)
    kw_ = dict(eps=EPS, k_scale=K_SCALE, tensors=tensors)
    if expect is not None:
        plan = ops.gemm_fp8_qkv_norm_rope_plan(*args, **kw_)
        assert plan is not None and plan["path"] == expect and plan["row_chunks"] == 1, plan
        # ... which is the plain GEMM's own path for these operands: the comparison below is on one kernel path
        assert ops.gemm_fp8_plan(a8, sa, w8, sw, one[0, :M], bias=bias, split=split)["path"] == expect
    assert ops.gemm_fp8_qkv_norm_rope(*args, **kw_) is True
    torch.cuda.synchronize()
    return one


def check_equal_and_canaries(two, one, M, tensors):
    """Every tensor bit for bit (v included: the plain fp8 GEMM's v), rows past M, the tensor past N and the gaps untouched."""
    for t in range(tensors):
        diff = bits(one[t, :M]) != bits(two[t, :M])
        assert not bool(diff.any()), f"tensor {t}: {int(diff.sum())} elements differ, first at {diff.nonzero()[0].tolist()}"
        assert not bool(torch.isnan(one[t, :M]).any())
    assert bool((bits(one[:tensors, M:]) == NAN_BITS).all()), "rows past M (the gap between the split tensors) were written"
    assert bool((bits(one[tensors]) == NAN_BITS).all()), "columns past N were written"
    assert torch.equal(bits(one), bits(two))


# (M, width, K, text rows, path).  Tiled: a ragged row tile with the text / video boundary inside a 16-row fragment; fewer rows
# than a fragment with q | k inside a 128-column tile (columns 128-191 q, 192-255 k); all text (cos and sin None).
# Persistent: 18 x 15 = 270 tiles, more than the 256 workgroups -- some run the epilogue and then a second tile --, a ragged last
# row tile, a quarter-full last column tile, q | k at column 1216 = 4 * 256 + 192 and k | v at 2432 = 9 * 256 + 128 inside waves,
# and the shortest K the kernel takes; 15 x 15 = 225 tiles, all text.
SHAPES = [(300, 128, 256, 40, T128), (17, 192, 128, 0, T128), (300, 192, 256, 300, T128),
          (4400, 1216, 512, 226, P256), (3700, 1216, 512, 3700, P256)]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,width,K,text,path", SHAPES)
def test_fused_launch_equals_gemm_then_qknorm_bit_for_bit(dev, M, width, K, text, path, with_bias):
    a8, sa, w8, sw, bias = operands(dev, M, 3 * width, K)
    b = bias if with_bias else None
    two = two_launches(dev, a8, sa, w8, sw, b, M, width, text, key=(M, width, K, text, with_bias, 0))
    one = fused(dev, a8, sa, w8, sw, b, M, width, text, expect=path)
    check_equal_and_canaries(two, one, M, 3)
    assert float(one[:3, :M].float().abs().sum()) > 0


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_the_tiled_instance_on_many_tiles_under_the_option(dev, with_bias):
    """fp8_kernel = 1: the first persistent shape on the 128 x 128 kernel -- 35 x 29 tiles, q / k / v per 64-column head with
    q | k and k | v inside tiles; both paths follow the option, so the pair is still on one kernel."""
    from bind_your_avatar_implementation_amd import ops
    M, width, K, text = 4400, 1216, 512, 226
    a8, sa, w8, sw, bias = operands(dev, M, 3 * width, K)
    b = bias if with_bias else None
    with ops.options(fp8_kernel=1):
        two = two_launches(dev, a8, sa, w8, sw, b, M, width, text, key=(M, width, K, text, with_bias, 1))
        one = fused(dev, a8, sa, w8, sw, b, M, width, text, expect=T128)
    check_equal_and_canaries(two, one, M, 3)


@pytest.mark.parametrize("M,width,K,path", [(300, 192, 256, T128), (5200, 1216, 512, P256)])
def test_q_and_k_alone(dev, M, width, K, path):
    """tensors = 2: N = 2 width, the first two thirds of the packed weight (persistent: 21 x 10 = 210 tiles); columns past N
    belong to no tensor."""
    text = 40 if M == 300 else 226
    a8, sa, w8, sw, bias = operands(dev, M, 3 * width, K)
    w2, sw2, bias2 = w8[:2 * width].contiguous(), sw[:2 * width].contiguous(), bias[:2 * width].contiguous()
    two = two_launches(dev, a8, sa, w2, sw2, bias2, M, width, text, tensors=2)
    one = fused(dev, a8, sa, w2, sw2, bias2, M, width, text, tensors=2, expect=path)
    check_equal_and_canaries(two, one, M, 2)
    # ... and q, k are what the three-tensor launch writes (on the same path)
    three = fused(dev, a8, sa, w8, sw, bias, M, width, text, expect=path)
    assert torch.equal(three[:2, :M], one[:2, :M])


@pytest.mark.parametrize("M,width,K,path", [(300, 256, 256, T128), (3500, 1280, 512, P256)])
def test_column_block_form(dev, M, width, K, path):
    """The head-parallel sharded step's layout: n_split = width / 4, column block t * 4 + j = tensor t, heads of rank j, each
    [M, width / 4] at c_split_stride; bya_qknorm_rope sees the q and k blocks as a batch of 4.  (Persistent: 14 x 15 = 210.)"""
    from bind_your_avatar_implementation_amd import ops
    text, W = 40, 4
    Dl = width // W
    a8, sa, w8, sw, bias = operands(dev, M, 3 * width, K)
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    two, one = nan_buffer(dev, 3 * W + 1, M + PAD, Dl), nan_buffer(dev, 3 * W + 1, M + PAD, Dl)
    split = (Dl, (M + PAD) * Dl)
    assert ops.gemm_fp8_plan(a8, sa, w8, sw, two[0, :M], bias=bias, split=split)["path"] == path
    ops.gemm_fp8(a8, sa, w8, sw, two[0, :M], bias=bias, split=split)
    ops.qknorm_rope(two[:W, :M], two[W:2 * W, :M], qw, qb, kw, kb, cos, sin, heads=Dl // 64, text_rows=text, eps=EPS,
                    k_scale=K_SCALE)
    args = (a8, sa, w8, sw, one[0, :M], bias, split, qw, qb, kw, kb, cos, sin, text)
    plan = ops.gemm_fp8_qkv_norm_rope_plan(*args, eps=EPS, k_scale=K_SCALE)
    assert plan["path"] == path and plan["row_chunks"] == 1, plan
    assert ops.gemm_fp8_qkv_norm_rope(*args, eps=EPS, k_scale=K_SCALE) is True
    torch.cuda.synchronize()
    check_equal_and_canaries(two, one, M, 3 * W)


def raw_qkn(a, sa, w, sw, bias, c_ptr, M, width, K, norm, text, ldc, n_split, c_split_stride, batch=1, a_bs=0, c_bs=0,
            expect=None):
    from bind_your_avatar_implementation_amd import _hip, ops
    qw, qb, kw, kb, cos, sin = norm
    d, n, plan = ops.GemmDesc(), _hip.QkNormDesc(), _hip.GemmPlan()
    d.M, d.N, d.K, d.batch = M, 3 * width, K, batch
    d.lda, d.ldw, d.ldc = K, K, ldc
    d.a_batch_stride, d.c_batch_stride = a_bs, c_bs
    d.n_split, d.c_split_stride, d.alpha = n_split, c_split_stride, 1.0
    p = lambda t: None if t is None else t.data_ptr()
    n.qw, n.qb, n.kw, n.kb, n.cos, n.sin = p(qw), p(qb), p(kw), p(kb), p(cos), p(sin)
    n.text_rows, n.width, n.eps, n.k_scale = text, width, EPS, K_SCALE
    args = (a.data_ptr(), sa.data_ptr(), w.data_ptr(), sw.data_ptr(), p(bias), c_ptr, ctypes.byref(d), ctypes.byref(n))
    lib = _hip.load()
    if expect is not None:
        assert lib.bya_gemm_fp8_qkv_norm_rope_plan(*args, ctypes.byref(plan)) == 0
        assert (ops.GEMM_PATHS[plan.path], plan.row_chunks) == (expect, 1)
    rc = lib.bya_gemm_fp8_qkv_norm_rope(*args, ops._stream())
    assert rc == 0, rc


@pytest.mark.parametrize("M,width,K,path", [(300, 192, 256, T128), (1800, 1216, 512, P256)])
def test_batched_operands_with_batch_strides(dev, M, width, K, path):
    """batch = 2 with an a_batch_stride that is not M * lda and a c_batch_stride larger than the matrix (persistent:
    2 x 8 x 15 = 240 tiles, taken by the batch as a whole): A advances by a_batch_stride, C by c_batch_stride, the row scale of
    entry z is a_scale[z * M + m] (dense), and the rotary row index restarts per batch entry."""
    text = 40
    a0, s0, w8, sw, bias = operands(dev, M, 3 * width, K)
    a1, s1 = operands(dev, M, 3 * width, K, seed=1)[:2]
    a_bs, c_bs = M * K + 160, (M + PAD) * width
    abuf = torch.zeros(2 * a_bs, dtype=torch.uint8, device=dev)
    abuf[:M * K] = a0.reshape(-1)
    abuf[a_bs:a_bs + M * K] = a1.reshape(-1)
    sa = torch.cat([s0, s1]).contiguous()
    one = nan_buffer(dev, 4, 2, M + PAD, width)                                           # [tensor, batch, rows, width]
    raw_qkn(abuf, sa, w8, sw, bias, one.data_ptr(), M, width, K, norm_params(dev, M, text), text, width, width, 2 * c_bs,
            batch=2, a_bs=a_bs, c_bs=c_bs, expect=path)
    torch.cuda.synchronize()
    # the reference: the plain GEMM on the same batched descriptor (so that it takes the same path), then the norm per entry
    from bind_your_avatar_implementation_amd import ops
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    two = nan_buffer(dev, 4, 2, M + PAD, width)
    a_st, s_st = torch.stack([a0, a1]), torch.stack([s0, s1])
    assert ops.gemm_fp8_plan(a_st, s_st, w8, sw, two[0, :, :M], bias=bias, split=(width, 2 * c_bs))["path"] == path
    ops.gemm_fp8(a_st, s_st, w8, sw, two[0, :, :M], bias=bias, split=(width, 2 * c_bs))
    for z in range(2):
        ops.qknorm_rope(two[0, z, :M], two[1, z, :M], qw, qb, kw, kb, cos, sin, heads=width // 64, text_rows=text, eps=EPS,
                        k_scale=K_SCALE)
    torch.cuda.synchronize()
    assert torch.equal(bits(one), bits(two))
    assert not torch.equal(one[0, 0, :M], one[0, 1, :M])
    # and the front end's own batch form (evenly stacked entries)
    front = nan_buffer(dev, 3, 2, M, width)
    assert ops.gemm_fp8_qkv_norm_rope(a_st, s_st, w8, sw, front[0], bias, (width, 2 * M * width), qw, qb, kw, kb, cos, sin, text,
                                      eps=EPS, k_scale=K_SCALE)
    assert torch.equal(front, one[:3, :, :M])


@pytest.mark.parametrize("M,width,K,path", [(300, 192, 256, T128), (3700, 1216, 512, P256)])
def test_row_stride_padding_is_not_written(dev, M, width, K, path):
    """ldc larger than the tensor's width: the padding of every row keeps its canary (16-byte stores stay inside a head)."""
    text, ldc = 40, width + 64
    a8, sa, w8, sw, bias = operands(dev, M, 3 * width, K)
    two = two_launches(dev, a8, sa, w8, sw, bias, M, width, text)
    one = nan_buffer(dev, 4, M + PAD, ldc)
    raw_qkn(a8, sa, w8, sw, bias, one.data_ptr(), M, width, K, norm_params(dev, M, text), text, ldc, width, (M + PAD) * ldc,
            expect=path)
    torch.cuda.synchronize()
    assert torch.equal(bits(one[:, :, :width]), bits(two))
    assert bool((bits(one[:, :, width:]) == NAN_BITS).all())


def test_declined_shapes_launch_nothing(dev):
    from bind_your_avatar_implementation_amd import ops
    M, K, text = 300, 256, 40
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    a8, sa, w8, sw, bias = operands(dev, M, 3 * 96, K)                                    # width 96: no whole heads
    out = nan_buffer(dev, 3, M, 96)
    assert ops.gemm_fp8_qkv_norm_rope(a8, sa, w8, sw, out[0], bias, (96, M * 96), qw, qb, kw, kb, cos, sin, text) is False
    torch.cuda.synchronize()
    assert bool((bits(out) == NAN_BITS).all())
    a8, sa, w8, sw, bias = operands(dev, M, 3 * 128, K)
    out = nan_buffer(dev, 3, M, 128)
    args = (a8, sa, w8, sw, out[0], bias, (128, M * 128), qw, qb, kw, kb, cos, sin, text)
    assert ops.gemm_fp8_qkv_norm_rope(*args, act="gelu_tanh") is False                    # an activation
    assert ops.gemm_fp8_qkv_norm_rope(*args, res=torch.zeros(M, 3 * 128, dtype=BF, device=dev)) is False      # a residual
    torch.cuda.synchronize()
    assert bool((bits(out) == NAN_BITS).all())
    assert ops.gemm_fp8_qkv_norm_rope(*args) is True                                      # (the same call without them is taken)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


# ------------------------------------------------------------------------------------------ engine
class Counter:
    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *a, **kw):
        self.n += 1
        return self.fn(*a, **kw)


def counted_forward(model, gi, monkeypatch):
    from bind_your_avatar_implementation_amd import ops
    model(**gi)                                                                           # builds the engine (packs weights)
    with monkeypatch.context() as mp:
        n, f = Counter(ops.qknorm_rope), Counter(ops.gemm_fp8_qkv_norm_rope)
        mp.setattr(ops, "qknorm_rope", n)
        mp.setattr(ops, "gemm_fp8_qkv_norm_rope", f)
        out = model(**gi)[0].clone()
    return out, n.n, f.n


def test_engine_qkv_projection_norms_q_and_k_itself(dev, monkeypatch):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    model.enable_fp8_weights()                                                            # the default is off
    off, n_off, f_off = counted_forward(model, gi, monkeypatch)
    assert model._engine.fp8_weights and not model._engine.fp8_fuse_qk_norm and f_off == 0
    # (the condition of the counts below: no layer of this model asks for the norm statistics, which keep the two launches)
    assert all(b <= ops.ATTN_BOUND_LIMIT for b in model._engine.score_bound)
    model.enable_fp8_weights(fuse_qk_norm=True)
    assert model._engine is None                                                          # the switch invalidates the engine
    on, n_on, f_on = counted_forward(model, gi, monkeypatch)
    assert model._engine.fp8_fuse_qk_norm
    print(f"fp8: qknorm_rope calls {n_off} -> {n_on}, gemm_fp8_qkv_norm_rope calls {f_off} -> {f_on}, {blocks} blocks")
    assert torch.equal(on, off)
    assert n_off - n_on == blocks and f_on == blocks
    # graph replay of the fused step: bit for bit the eager result
    model.use_hip_graph = True
    try:
        model(**gi)                                                                       # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], on)
    finally:
        model.use_hip_graph = False
        model._graphs = {}
    # q|k|v in bf16: the switch changes nothing and launches nothing new
    sel = ("out", "ff1", "ff2")
    model.enable_fp8_weights(linears=sel)
    ref, n0, f0 = counted_forward(model, gi, monkeypatch)
    model.enable_fp8_weights(linears=sel, fuse_qk_norm=True)
    got, n1, f1 = counted_forward(model, gi, monkeypatch)
    assert set(model._engine.w8) == set(sel) and (f0, f1) == (0, 0) and n0 == n1
    assert torch.equal(got, ref)
