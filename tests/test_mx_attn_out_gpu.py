"""The attention whose epilogue writes MX codes (include/bya.h, bya_attn_fwd_mx; ops.attention(mx_out=...)): byte for byte
bya_attn_fwd followed by bya_quantize_mx -- on the exact data of tests/exact_attn.py for every head_dim-64 kernel path (against
the torch restatement of tests/test_mx_cpu.py applied to the closed-form answer), on random data with block scales over many
exponents against the two launches, on zero blocks, with canaries around and between the rows, as the operand of the next
GEMM, and in the engine (enable_mx_weights(fuse_attention_quant=...)).  No tolerance anywhere: every comparison is torch.equal."""
import ctypes

import pytest
import torch

import exact_attn as X
from exact_attn import BF
from test_attn_exact_gpu import attn_layout
from test_mx_cpu import quant_mx_ref

pytestmark = pytest.mark.gpu

FORMATS = ("mxfp8", "mxfp6")
CODE = {"mxfp8": 0, "mxfp6": 2}
KINDS = ("run", "pre", "w4", "dev")
# every head_dim-64 case but the two 17776-row stream-K ones (building their data alone takes longer than a test may)
EXACT_CASES = [c for c in X.ATTN_CASES if c["D"] == 64 and c["Sq"] < 17776]


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def pair(ops, lead, heads, fmt, dev):
    """A 0xA5-filled (codes, scales) pair for a [*lead, heads * 64] output."""
    return (torch.full((*lead, ops.mx_code_bytes(heads * 64, fmt)), 0xA5, dtype=torch.uint8, device=dev),
            torch.full((*lead, heads * 2), 0xA5, dtype=torch.uint8, device=dev))


def two_launch_ref(ops, out, fmt):
    """``quantize_mx`` of the bf16 attention output: the second of the two launches.  bya_quantize_mx takes K % 128 == 0; three
    heads are 192 columns, so the matrix is padded with zero columns to the next multiple and the padding's blocks are cut off
    again -- a block's bytes depend on its own 32 values alone."""
    K = out.shape[-1]
    pad = -K % 128
    if pad:
        out = torch.cat([out, torch.zeros(*out.shape[:-1], pad, dtype=out.dtype, device=out.device)], -1)
    codes, scales = ops.quantize_mx(out.contiguous(), fmt)
    return codes[..., :ops.mx_code_bytes(K, fmt)].contiguous(), scales[..., :K // 32].contiguous()


def first_diff(got, ref):
    bad = (got != ref).nonzero()
    return f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}: got {int(got[tuple(bad[0])])}, want {int(ref[tuple(bad[0])])}"


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c["name"] for c in EXACT_CASES])
def test_exact_data_every_d64_path(ops, dev, case):
    c = case
    d = X.attn_case_data(c, dev)
    q, k, v, _, _, want, kw, flagged = attn_layout(c, d, dev)
    kw.pop("o_strides")
    wantb = want.to(BF)
    assert torch.equal(wantb.float(), want)
    for fmt in FORMATS:
        ref_c, ref_s = quant_mx_ref(wantb.cpu(), fmt)                       # the closed form, quantised on the CPU
        codes, scales = pair(ops, want.shape[:-1], c["H"], fmt, dev)
        with ops.options(attn_streamk=c["sk_opt"]):
            plan = ops.attention_plan(None, mx_out=(codes, scales, fmt), **kw)
            key = ops.attention_plan_key(plan)
            assert key == X.ATTN_KIND_VARIANT[c["kind"]] + ("+streamk" if c["sk"] else "") + "/" + fmt, (key, plan)
            assert plan["q_tile"] == (512 if c["kind"] in ("w4", "dev") else 128) and plan["second_launch"] == (c["kind"] == "dev")
            for rep in range(2 if plan["stream_k"] else 1):                 # the hand-off flags must be back at 0 after a launch
                codes.fill_(0xA5)
                scales.fill_(0xA5)
                got = ops.attention(q, k, v, None, mx_out=(codes, scales, fmt), tag="exact", **kw)
                assert got[0] is codes and got[1] is scales
                what = f"{c['name']} {fmt} launch {rep} [plan {key}]"
                assert torch.equal(scales.cpu(), ref_s), f"{what} scales (batch, row, block): {first_diff(scales.cpu(), ref_s)}"
                assert torch.equal(codes.cpu(), ref_c), f"{what} codes (batch, row, byte): {first_diff(codes.cpu(), ref_c)}"
        if flagged is not None:
            flags = kw["bound"][2]
            assert torch.equal(flags != 0, flagged) and bool((flags != -7).all())
        if plan["stream_k"]:
            assert ops.attn_workspace_status() == 0


_RANDOM = {}


def random_case(ops, dev, kind, Sq, Skv, H, zero_heads=()):
    """Gaussian q, k, v [1, S, H * 64] with outlier-heavy V columns (block maxima over ~20 binades), the launch arguments of
    ``kind`` and the bf16 output of the two-launch path; built once per (kind, shape)."""
    key = (kind, Sq, Skv, H, tuple(zero_heads))
    if key not in _RANDOM:
        g = torch.Generator().manual_seed(Sq * 7 + Skv + H)
        W = H * 64
        q = (torch.randn(1, Sq, W, generator=g) * 0.6).to(BF).to(dev)
        k = (torch.randn(1, Skv, W, generator=g) * 0.6).to(BF).to(dev)       # |q . k| ~ 3, far inside the static bound
        v = torch.randn(1, Skv, W, generator=g)
        nblk = W // 32                                                        # per 32-column block: 2^-12 .. 2^8, evenly spread
        v = v * torch.exp2(-12.0 + (torch.arange(nblk) * 20 // (nblk - 1)).float()).repeat_interleave(32)
        v[:, :, torch.randperm(W, generator=g)[:max(1, W // 16)]] *= 100.0    # and outlier columns
        for h in zero_heads:
            v[:, :, h * 64:h * 64 + 32] = 0.0
        v = v.to(BF).to(dev)
        kw = dict(head_dim=64, heads=H, nb1=1, nb2=1, Sq=Sq, Skv=Skv, q_strides=(Sq * W, 0, W), k_strides=(Skv * W, 0, W),
                  v_strides=(Skv * W, 0, W))
        if kind == "run":
            kw.update(scale=0.125)
        elif kind == "pre":
            kw.update(scale=1.0, prescaled=True)
        elif kind == "w4":
            kw.update(scale=1.0, prescaled=True, score_bound=X.BOUND)
        else:
            # as in test_attn_exact_gpu.attn_layout: heads 1, 4, 7 exceed the limit and go to the second launch
            flagged = torch.arange(H, device=dev) % 3 == 1
            assert bool(flagged.any()) and not bool(flagged.all())
            stats = torch.full((2, 2, H + 5), 1.0, device=dev)
            stats[1, :, 2:2 + H] = torch.where(flagged, 100.0, 80.0)
            kw.update(scale=1.0, prescaled=True, bound=(stats, 2, torch.full((H,), -7, dtype=torch.int32, device=dev)))
        out = torch.full((1, Sq, W), float("nan"), dtype=BF, device=dev)
        ops.attention(q, k, v, out, o_strides=(Sq * W, 0, W), tag="exact", **kw)
        assert bool(torch.isfinite(out.float()).all())
        _RANDOM[key] = (q, k, v, kw, out)
    return _RANDOM[key]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Sq,Skv,H", [(40, 40, 8), (513, 1350, 4), (1031, 4133, 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_launch_equals_attention_then_quantiser(ops, dev, kind, Sq, Skv, H, fmt):
    q, k, v, kw, out = random_case(ops, dev, kind, Sq, Skv, H)
    ref_c, ref_s = two_launch_ref(ops, out, fmt)
    assert int(ref_s.max()) - int(ref_s.min()) >= 12                        # the block scales do span many exponents
    codes, scales = pair(ops, (1, Sq), H, fmt, dev)
    plan = ops.attention_plan(None, mx_out=(codes, scales, fmt), **kw)
    assert plan["variant"] == X.ATTN_KIND_VARIANT[kind] and plan["second_launch"] == (kind == "dev"), plan
    ops.attention(q, k, v, None, mx_out=(codes, scales, fmt), tag="exact", **kw)
    assert torch.equal(scales, ref_s), first_diff(scales, ref_s)
    assert torch.equal(codes, ref_c), first_diff(codes, ref_c)
    if kind == "dev":
        assert (kw["bound"][2] != 0).tolist() == [h % 3 == 1 for h in range(H)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", KINDS)
def test_zero_blocks(ops, dev, kind, fmt):
    """V zero on the first 32 columns of heads 1 and 6: scale byte 127 and all-zero codes there, ordinary blocks elsewhere."""
    H, zero = 8, (1, 6)
    q, k, v, kw, out = random_case(ops, dev, kind, 40, 40, H, zero_heads=zero)
    codes, scales = pair(ops, (1, 40), H, fmt, dev)
    ops.attention(q, k, v, None, mx_out=(codes, scales, fmt), tag="exact", **kw)
    bb = ops.mx_code_bytes(32, fmt)
    blocks = codes.view(40, 2 * H, bb)
    is_zero = torch.zeros(2 * H, dtype=torch.bool, device=dev)
    is_zero[[2 * h for h in zero]] = True
    assert bool((scales.view(40, 2 * H)[:, is_zero] == 127).all()) and bool((blocks[:, is_zero] == 0).all())
    assert bool((blocks[:, ~is_zero].amax(-1) != 0).all())
    ref_c, ref_s = two_launch_ref(ops, out, fmt)
    assert torch.equal(scales, ref_s) and torch.equal(codes, ref_c)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind,Sq,Skv,H", [("run", 1, 40, 8), ("w4", 1, 40, 8), ("pre", 513, 1350, 4), ("w4", 513, 1350, 4),
                                           ("dev", 513, 1350, 4)])
def test_no_stray_writes_around_or_between_the_rows(ops, dev, kind, Sq, Skv, H, fmt):
    """Codes and scales inside larger 0xA5-filled buffers, row strides wider than the data, a byte offset that leaves the
    codes 4-byte and the scales 1-byte aligned, two guard rows behind the last one: only [rows < Sq] x [the heads' bytes] change."""
    from bind_your_avatar_implementation_amd import _hip
    if Sq == 1:
        q, k, v, kw, _ = random_case(ops, dev, kind, 40, Skv, H)
        q = q[:, 17:18].contiguous()
        kw = {**kw, "Sq": 1, "q_strides": (H * 64, 0, H * 64)}
        out = torch.empty(1, 1, H * 64, dtype=BF, device=dev)
        ops.attention(q, k, v, out, o_strides=(H * 64, 0, H * 64), tag="exact", **kw)
    else:
        q, k, v, kw, out = random_case(ops, dev, kind, Sq, Skv, H)
    ref_c, ref_s = two_launch_ref(ops, out, fmt)
    cb, sb = ops.mx_code_bytes(H * 64, fmt), 2 * H
    c_row, s_row, c_off, s_off, guard = cb + 20, sb + 3, 36, 5, 2
    cbuf = torch.full(((Sq + guard) * c_row + 64,), 0xA5, dtype=torch.uint8, device=dev)
    sbuf = torch.full(((Sq + guard) * s_row + 64,), 0xA5, dtype=torch.uint8, device=dev)
    d = ops._attn_desc(kw["head_dim"], H, 1, 1, Sq, Skv, kw["q_strides"], kw["k_strides"], kw["v_strides"], (0, 0, 0), kw["scale"],
                       kw.get("prescaled", False), kw.get("score_bound", 0.0), kw.get("bound"))
    rc = _hip.load().bya_attn_fwd_mx(q.data_ptr(), k.data_ptr(), v.data_ptr(), cbuf.data_ptr() + c_off, sbuf.data_ptr() + s_off,
                                     ctypes.byref(d), CODE[fmt], 0, 0, c_row, 0, 0, s_row, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    want_c = torch.full_like(cbuf, 0xA5)
    want_c[c_off:c_off + (Sq + guard) * c_row].view(Sq + guard, c_row)[:Sq, :cb] = ref_c.view(Sq, cb)
    want_s = torch.full_like(sbuf, 0xA5)
    want_s[s_off:s_off + (Sq + guard) * s_row].view(Sq + guard, s_row)[:Sq, :sb] = ref_s.view(Sq, sb)
    assert torch.equal(cbuf, want_c), "codes: " + first_diff(cbuf, want_c)
    assert torch.equal(sbuf, want_s), "scales: " + first_diff(sbuf, want_s)


@pytest.mark.parametrize("fmt,w_fmt", [("mxfp6", "mxfp6"), ("mxfp8", "mxfp4")])
def test_fused_pair_is_a_legal_operand_of_the_next_gemm(ops, dev, fmt, w_fmt):
    H, M, N = 8, 300, 512
    q, k, v, kw, out = random_case(ops, dev, "w4", M, 300, H)
    g = torch.Generator().manual_seed(5)
    wc, ws = ops.quantize_mx((torch.randn(N, H * 64, generator=g) * (H * 64) ** -0.5).to(BF).to(dev), w_fmt)
    codes, scales = pair(ops, (1, M), H, fmt, dev)
    ops.attention(q, k, v, None, mx_out=(codes, scales, fmt), tag="exact", **kw)
    ref_c, ref_s = two_launch_ref(ops, out, fmt)
    y0 = torch.empty(M, N, dtype=BF, device=dev)
    y1 = torch.empty(M, N, dtype=BF, device=dev)
    ops.gemm_mx(ref_c[0], ref_s[0], wc, ws, y0, fmt, w_fmt=w_fmt)
    ops.gemm_mx(codes[0], scales[0], wc, ws, y1, fmt, w_fmt=w_fmt)
    assert bool(torch.isfinite(y0.float()).all()) and torch.equal(y0, y1)


class Counter:
    def __init__(self, fn):
        self.fn, self.n, self.mx = fn, 0, 0

    def __call__(self, *a, **kw):
        self.n += 1
        self.mx += kw.get("mx_out") is not None
        return self.fn(*a, **kw)


def counted_forward(model, gi, monkeypatch):
    """-> (output, quantize_mx calls, joint-attention launches that wrote MX codes, joint-attention launches) of one step."""
    from bind_your_avatar_implementation_amd import ops
    model(**gi)                                                                           # builds the engine (packs weights)
    with monkeypatch.context() as mp:
        qz, at = Counter(ops.quantize_mx), Counter(ops.attention)
        mp.setattr(ops, "quantize_mx", qz)
        mp.setattr(ops, "attention", at)                                                  # self_attention calls through it
        out = model(**gi)[0].clone()
    return out, qz.n, at.mx, at.n


@pytest.mark.parametrize("fmt,weight_format", [("mxfp6", None), ("mxfp8", "mxfp4")])
def test_engine_attention_feeds_to_out_directly(dev, monkeypatch, fmt, weight_format):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    gi = to_dev(synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True), dev)
    blocks = len(model.transformer_blocks)
    kw = dict(weight_format=weight_format)
    model.enable_mx_weights(fmt, fuse_activation_quant=False, **kw)                       # the attention switch is off by default
    off, q_off, a_off, n_off = counted_forward(model, gi, monkeypatch)
    assert not model._engine.mx_fuse_attn_quant and a_off == 0
    model.enable_mx_weights(fmt, fuse_activation_quant=False, fuse_attention_quant=True, **kw)
    assert model._engine is None                                                          # the switch invalidates the engine
    on, q_on, a_on, n_on = counted_forward(model, gi, monkeypatch)
    assert model._engine.mx_fuse_attn_quant
    print(f"{fmt}/{weight_format}: quantize_mx calls {q_off} -> {q_on}, MX attention launches {a_off} -> {a_on}, {blocks} blocks")
    assert torch.equal(on, off)
    assert q_off - q_on == blocks and a_on == blocks and n_on == n_off                   # one fused attention per block
    # both fusions: no standalone quantiser launch is left in the step
    model.enable_mx_weights(fmt, fuse_attention_quant=True, **kw)
    both, q_both, a_both, _ = counted_forward(model, gi, monkeypatch)
    assert torch.equal(both, off) and q_both == 0 and a_both == blocks
    # graph replay of the fused step: bit for bit the eager result
    model.use_hip_graph = True
    try:
        model(**gi)                                                                       # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], off)
    finally:
        model.use_hip_graph = False
        model._graphs = {}
    # to_out in bf16: nothing to feed, the output and the launches do not depend on the switch
    sel = ("qkv", "ff1", "ff2")
    model.enable_mx_weights(fmt, linears=sel, fuse_attention_quant=False, **kw)
    ref, q0, a0, _ = counted_forward(model, gi, monkeypatch)
    model.enable_mx_weights(fmt, linears=sel, fuse_attention_quant=True, **kw)
    got, q1, a1, _ = counted_forward(model, gi, monkeypatch)
    assert set(model._engine.wmx) == set(sel) and a0 == 0 and a1 == 0 and q0 == q1
    assert torch.equal(got, ref)
