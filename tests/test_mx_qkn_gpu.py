"""The MX q|k|v projection whose epilogue norms and rotates q and k (include/bya.h, bya_gemm_mx_qkv_norm_rope;
ops.gemm_mx_qkv_norm_rope): bit for bit bya_gemm_mx(_mixed)(..., n_split) followed by bya_qknorm_rope -- over every operand
pair and both tiles, on shapes whose tiles and waves straddle the q | k and k | v boundaries, with and without bias, batched,
for q | k alone, in the sharded step's column-block form, with canaries behind the rows, behind the last column tile and
between the split tensors, and in the engine (enable_mx_weights(fuse_qk_norm=...)).  No tolerance anywhere: every
comparison is torch.equal (on the bit patterns where a buffer holds NaN canaries)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FORMATS = ("mxfp8", "mxfp6")
CODE = {"mxfp8": 0, "mxfp6": 2, "mxfp4": 4}
BITS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
K_SCALE, EPS, PAD = 0.18, 1e-6, 8
NAN_BITS = torch.tensor(float("nan"), dtype=BF).view(torch.int16).item()


def bits(t):
    return t.contiguous().view(torch.int16)


_OPERANDS, _NORM = {}, {}


def operands(dev, M, N, K, fmt, w_fmt, seed=0):
    """Gaussian MX operands of one shape and format pair, built once: (a codes, a scales, w codes, w scales, bias)."""
    from bind_your_avatar_implementation_amd import ops
    key = (M, N, K, fmt, w_fmt, seed)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(1000 * seed + M + N)
        a = torch.randn(M, K, generator=g).to(BF)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
        bias = (torch.randn(N, generator=g) * 0.5).to(BF).to(dev)
        _OPERANDS[key] = (*ops.quantize_mx(a.to(dev), fmt), *ops.quantize_mx(w.to(dev), w_fmt), bias)
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


def pair_and_fused(dev, ac, asc, wc, wsc, bias, fmt, w_fmt, M, width, text, tensors=3, expect=None):
    """Both paths into NaN-filled [tensors + 1, M + PAD, width] buffers (PAD rows behind every tensor: the gap between the
    split tensors; one more tensor: where columns past N would land).  Returns (two launches, fused)."""
    from bind_your_avatar_implementation_amd import ops
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    two, one = nan_buffer(dev, tensors + 1, M + PAD, width), nan_buffer(dev, tensors + 1, M + PAD, width)
    split = (width, (M + PAD) * width)
    ops.gemm_mx(ac, asc, wc, wsc, two[0, :M], fmt, bias=bias, split=split, w_fmt=w_fmt)
    ops.qknorm_rope(two[0, :M], two[1, :M], qw, qb, kw, kb, cos, sin, heads=width // 64, text_rows=text, eps=EPS, k_scale=K_SCALE)
    args = (ac, asc, wc, wsc, one[0, :M], bias, split, qw, qb, kw, kb, cos, sin, text)
    kw_ = dict(eps=EPS, k_scale=K_SCALE, tensors=tensors, fmt=fmt, w_fmt=w_fmt)
    if expect is not None:
        plan = ops.gemm_mx_qkv_norm_rope_plan(*args, **kw_)
        assert plan is not None and plan["path"] == expect and plan["row_chunks"] == 1, plan
    assert ops.gemm_mx_qkv_norm_rope(*args, **kw_) is True
    torch.cuda.synchronize()
    return two, one


def check_equal_and_canaries(two, one, M, tensors):
    """Every tensor bit for bit (v included: the plain MX GEMM's v), rows past M, the tensor past N and the gaps untouched."""
    for t in range(tensors):
        diff = bits(one[t, :M]) != bits(two[t, :M])
        assert not bool(diff.any()), f"tensor {t}: {int(diff.sum())} elements differ, first at {diff.nonzero()[0].tolist()}"
        assert not bool(torch.isnan(one[t, :M]).any())
    assert bool((bits(one[:tensors, M:]) == NAN_BITS).all()), "rows past M (the gap between the split tensors) were written"
    assert bool((bits(one[tensors]) == NAN_BITS).all()), "columns past N were written"
    assert torch.equal(bits(one), bits(two))


# (M, width, K, text rows): a ragged row tile with the text / video boundary inside a 16-row fragment; a 128-column tile that
# straddles q | k (columns 128-191 q, 192-255 k) and fewer rows than a fragment; all text (cos and sin None); 14 x 15 = 210
# tiles of 256 x 256 (>= 200: mxfp6 activations run on 256 x 256 tiles) with q | k at column 1216 = 4 * 256 + 192, inside the
# second wave's 128 columns, k | v at 2432 = 9 * 256 + 128, and a last column tile of 64 columns
SHAPES = [(300, 128, 256, 40), (17, 192, 128, 0), (300, 192, 256, 300), (3500, 1216, 256, 226)]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("w_kind", ["same", "mxfp4"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,width,K,text", SHAPES)
def test_fused_launch_equals_gemm_then_qknorm_bit_for_bit(dev, M, width, K, text, fmt, w_kind, with_bias):
    w_fmt = fmt if w_kind == "same" else "mxfp4"
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, fmt, w_fmt)
    expect = "t256x256" if fmt == "mxfp6" and M == 3500 else "t128x128"
    two, one = pair_and_fused(dev, ac, asc, wc, wsc, bias if with_bias else None, fmt, w_fmt, M, width, text, expect=expect)
    check_equal_and_canaries(two, one, M, 3)
    assert float(one[:3, :M].float().abs().sum()) > 0


@pytest.mark.parametrize("fmt,w_fmt,M,width", [("mxfp8", "mxfp8", 300, 192), ("mxfp6", "mxfp4", 300, 192),
                                                ("mxfp6", "mxfp6", 3500, 1216)])
def test_q_and_k_alone(dev, fmt, w_fmt, M, width):
    """tensors = 2: N = 2 width, the first two thirds of the packed weight; columns past N belong to no tensor."""
    K, text = 256, 40
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, fmt, w_fmt)
    wc2, wsc2, bias2 = wc[:2 * width].contiguous(), wsc[:2 * width].contiguous(), bias[:2 * width].contiguous()
    two, one = pair_and_fused(dev, ac, asc, wc2, wsc2, bias2, fmt, w_fmt, M, width, text, tensors=2)
    check_equal_and_canaries(two, one, M, 2)
    # ... and q, k are what the three-tensor launch writes
    _, three = pair_and_fused(dev, ac, asc, wc, wsc, bias, fmt, w_fmt, M, width, text)
    assert torch.equal(three[:2, :M], one[:2, :M])


@pytest.mark.parametrize("fmt,w_fmt,M", [("mxfp8", "mxfp4", 300), ("mxfp6", "mxfp6", 300), ("mxfp6", "mxfp6", 3500)])
def test_column_block_form(dev, fmt, w_fmt, M):
    """The head-parallel sharded step's layout: n_split = width / 4, column block t * 4 + j = tensor t, heads of rank j, each
    [M, width / 4] at c_split_stride; bya_qknorm_rope sees the q and k blocks as a batch of 4."""
    from bind_your_avatar_implementation_amd import ops
    width, K, text, W = (256 if M == 300 else 1280), 256, 40, 4
    Dl = width // W
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, fmt, w_fmt)
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    two, one = nan_buffer(dev, 3 * W + 1, M + PAD, Dl), nan_buffer(dev, 3 * W + 1, M + PAD, Dl)
    split = (Dl, (M + PAD) * Dl)
    ops.gemm_mx(ac, asc, wc, wsc, two[0, :M], fmt, bias=bias, split=split, w_fmt=w_fmt)
    ops.qknorm_rope(two[:W, :M], two[W:2 * W, :M], qw, qb, kw, kb, cos, sin, heads=Dl // 64, text_rows=text, eps=EPS,
                    k_scale=K_SCALE)
    args = (ac, asc, wc, wsc, one[0, :M], bias, split, qw, qb, kw, kb, cos, sin, text)
    plan = ops.gemm_mx_qkv_norm_rope_plan(*args, eps=EPS, k_scale=K_SCALE, fmt=fmt, w_fmt=w_fmt)
    assert plan["path"] == ("t256x256" if M == 3500 else "t128x128"), plan
    assert ops.gemm_mx_qkv_norm_rope(*args, eps=EPS, k_scale=K_SCALE, fmt=fmt, w_fmt=w_fmt) is True
    torch.cuda.synchronize()
    check_equal_and_canaries(two, one, M, 3 * W)


def raw_qkn(a, asc, w, wsc, bias, c_ptr, M, width, K, fmt, w_fmt, norm, text, ldc, n_split, c_split_stride, batch=1, a_bs=0,
            c_bs=0):
    from bind_your_avatar_implementation_amd import _hip, ops
    qw, qb, kw, kb, cos, sin = norm
    d, n = ops.GemmDesc(), _hip.QkNormDesc()
    d.M, d.N, d.K, d.batch = M, 3 * width, K, batch
    d.lda, d.ldw, d.ldc = K * BITS[fmt] // 8, K * BITS[w_fmt] // 8, ldc
    d.a_batch_stride, d.c_batch_stride = a_bs, c_bs
    d.n_split, d.c_split_stride, d.alpha = n_split, c_split_stride, 1.0
    p = lambda t: None if t is None else t.data_ptr()
    n.qw, n.qb, n.kw, n.kb, n.cos, n.sin = p(qw), p(qb), p(kw), p(kb), p(cos), p(sin)
    n.text_rows, n.width, n.eps, n.k_scale = text, width, EPS, K_SCALE
    rc = _hip.load().bya_gemm_mx_qkv_norm_rope(a.data_ptr(), asc.data_ptr(), w.data_ptr(), wsc.data_ptr(), p(bias), c_ptr,
                                               CODE[fmt], CODE[w_fmt], ctypes.byref(d), ctypes.byref(n), ops._stream())
    assert rc == 0, rc


@pytest.mark.parametrize("fmt,w_fmt", [("mxfp6", "mxfp6"), ("mxfp8", "mxfp4")])
def test_batched_operands_with_batch_strides(dev, fmt, w_fmt):
    """batch = 2 as grid.z with batch strides larger than the matrices: A codes advance by a_batch_stride, C by
    c_batch_stride, the scale rows of entry z are z * M + m (dense), and the rotary row is the row of the batch entry."""
    from bind_your_avatar_implementation_amd import ops
    M, width, K, text = 300, 192, 256, 40
    ac0, asc0, wc, wsc, bias = operands(dev, M, 3 * width, K, fmt, w_fmt)
    ac1, asc1 = operands(dev, M, 3 * width, K, fmt, w_fmt, seed=1)[:2]
    lda = ac0.shape[1]
    a_bs, c_bs = M * lda + 160, (M + PAD) * width
    abuf = torch.zeros(2 * a_bs, dtype=torch.uint8, device=dev)
    abuf[:M * lda] = ac0.reshape(-1)
    abuf[a_bs:a_bs + M * lda] = ac1.reshape(-1)
    sa = torch.cat([asc0, asc1]).contiguous()
    one = nan_buffer(dev, 4, 2, M + PAD, width)                                           # [tensor, batch, rows, width]
    raw_qkn(abuf, sa, wc, wsc, bias, one.data_ptr(), M, width, K, fmt, w_fmt, norm_params(dev, M, text), text, width, width,
            2 * c_bs, batch=2, a_bs=a_bs, c_bs=c_bs)
    torch.cuda.synchronize()
    for z, (a_c, a_s) in enumerate(((ac0, asc0), (ac1, asc1))):
        two, _ = pair_and_fused(dev, a_c, a_s, wc, wsc, bias, fmt, w_fmt, M, width, text)
        assert torch.equal(bits(one[:, z]), bits(two))
    assert not torch.equal(one[0, 0, :M], one[0, 1, :M])
    # and the front end's own batch form (evenly stacked entries)
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    front = nan_buffer(dev, 3, 2, M, width)
    assert ops.gemm_mx_qkv_norm_rope(torch.stack([ac0, ac1]), torch.stack([asc0, asc1]), wc, wsc, front[0], bias,
                                     (width, 2 * M * width), qw, qb, kw, kb, cos, sin, text, eps=EPS, k_scale=K_SCALE, fmt=fmt,
                                     w_fmt=w_fmt)
    assert torch.equal(front, one[:3, :, :M])


def test_row_stride_padding_is_not_written(dev):
    """ldc larger than the tensor's width: the padding of every row keeps its canary (16-byte stores stay inside a head)."""
    fmt = w_fmt = "mxfp6"
    M, width, K, text, ldc = 300, 192, 256, 40, 192 + 64
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * width, K, fmt, w_fmt)
    two, _ = pair_and_fused(dev, ac, asc, wc, wsc, bias, fmt, w_fmt, M, width, text)
    one = nan_buffer(dev, 4, M + PAD, ldc)
    raw_qkn(ac, asc, wc, wsc, bias, one.data_ptr(), M, width, K, fmt, w_fmt, norm_params(dev, M, text), text, ldc, width,
            (M + PAD) * ldc)
    torch.cuda.synchronize()
    assert torch.equal(bits(one[:, :, :width]), bits(two))
    assert bool((bits(one[:, :, width:]) == NAN_BITS).all())


def test_declined_shapes_launch_nothing(dev):
    from bind_your_avatar_implementation_amd import ops
    fmt = w_fmt = "mxfp6"
    M, K, text = 300, 256, 40
    ac, asc, wc, wsc, bias = operands(dev, M, 3 * 96, K, fmt, w_fmt)                       # width 96: no whole heads
    qw, qb, kw, kb, cos, sin = norm_params(dev, M, text)
    out = nan_buffer(dev, 3, M, 96)
    assert ops.gemm_mx_qkv_norm_rope(ac, asc, wc, wsc, out[0], bias, (96, M * 96), qw, qb, kw, kb, cos, sin, text, fmt=fmt) is False
    torch.cuda.synchronize()
    assert bool((bits(out) == NAN_BITS).all())


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
        n, f = Counter(ops.qknorm_rope), Counter(ops.gemm_mx_qkv_norm_rope)
        mp.setattr(ops, "qknorm_rope", n)
        mp.setattr(ops, "gemm_mx_qkv_norm_rope", f)
        out = model(**gi)[0].clone()
    return out, n.n, f.n


@pytest.mark.parametrize("fmt,weight_format", [("mxfp6", None), ("mxfp8", "mxfp4")])
def test_engine_qkv_projection_norms_q_and_k_itself(dev, monkeypatch, fmt, weight_format):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    model.enable_mx_weights(fmt, weight_format=weight_format)                             # the default is off
    off, n_off, f_off = counted_forward(model, gi, monkeypatch)
    assert not model._engine.mx_fuse_qk_norm and f_off == 0
    # (the condition of the counts below: no layer of this model asks for the norm statistics, which keep the two launches)
    assert all(b <= ops.ATTN_BOUND_LIMIT for b in model._engine.score_bound)
    model.enable_mx_weights(fmt, weight_format=weight_format, fuse_qk_norm=True)
    assert model._engine is None                                                          # the switch invalidates the engine
    on, n_on, f_on = counted_forward(model, gi, monkeypatch)
    assert model._engine.mx_fuse_qk_norm
    print(f"{fmt}/{weight_format}: qknorm_rope calls {n_off} -> {n_on}, gemm_mx_qkv_norm_rope calls {f_off} -> {f_on}, "
          f"{blocks} blocks")
    assert torch.equal(on, off)
    assert n_off - n_on == blocks and f_on == blocks
    # with the attention writing to_out's operand too: still the same bits
    model.enable_mx_weights(fmt, weight_format=weight_format, fuse_qk_norm=True, fuse_attention_quant=True)
    both, _, f_both = counted_forward(model, gi, monkeypatch)
    model.enable_mx_weights(fmt, weight_format=weight_format, fuse_attention_quant=True)
    assert f_both == blocks and torch.equal(both, counted_forward(model, gi, monkeypatch)[0]) and torch.equal(both, off)
    # graph replay of the fused step: bit for bit the eager result
    model.enable_mx_weights(fmt, weight_format=weight_format, fuse_qk_norm=True)
    model(**gi)
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
    model.enable_mx_weights(fmt, weight_format=weight_format, linears=sel)
    ref, n0, f0 = counted_forward(model, gi, monkeypatch)
    model.enable_mx_weights(fmt, weight_format=weight_format, linears=sel, fuse_qk_norm=True)
    got, n1, f1 = counted_forward(model, gi, monkeypatch)
    assert set(model._engine.wmx) == set(sel) and (f0, f1) == (0, 0) and n0 == n1
    assert torch.equal(got, ref)
