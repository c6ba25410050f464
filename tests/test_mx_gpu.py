"""MX weights (include/bya.h, "MX weights"; enable_mx_weights): the block quantisers byte for byte against the CPU
restatement of tests/test_mx_cpu.py, the GEMM's operand map on exact data, the GEMM against the exact product of the very
bytes it multiplied, and the engine stage by stage against the CPU oracle whose selected Linears are fake-quantised by the
same restatement.  The reference has no MX path (it is bf16 / fp16 only)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_fro
from exact_gemm import SENTINEL, assert_exact
from mx_ref import BITS, dequant_mx, e2m3_encode, hard_inputs, pack6, quant_mx_ref, rnd  # noqa: F401

pytestmark = pytest.mark.gpu

FORMATS = ("mxfp6", "mxfp8")


def sample_rows(M, gate_split, limit=288):
    """Every row of a small launch; of a large one the first 8 (``hard_inputs`` plants its blocks in rows 0 .. 3), the 8 around the
    gate boundary, the last 8 (the tail tile) and rows at a fixed odd stride."""
    if M <= limit:
        return torch.arange(M)
    picks = set(range(8)) | set(range(M - 8, M)) | set(range(0, M, (M // (limit - 24)) | 1))
    if gate_split:
        picks |= set(range(max(0, gate_split - 4), min(M, gate_split + 4)))
    return torch.tensor(sorted(picks))


def check_vs_fp64(name, got, ad, wd, K, bias, act, args, fmts, scales):
    """cond_gemm.check of an output against the fp64 definition on the dequantised bytes ``ad``, ``wd``: the bar per element with
    the EXACT block term, the differing share (without an activation) and, at K = 12288, where eps is wide, the signed mean
    against the restatement.  e2m3 activations (block term zero): every element.  e4m3 activations: every element of
    ``sample_rows``, since the exact term costs M N K operations."""
    import cond_gemm as C
    M = got.shape[0]
    e = dict(C.NO_EPILOGUE, bias=bias, act=act, gate0=args.get("gate0"), gate1=args.get("gate1"), gate_split=args.get("gate_split", 0),
             res=args.get("res"))
    asc, wsc = scales
    if fmts[0] != "mxfp6":
        rows = sample_rows(M, e["gate_split"]).to(got.device)
        got, ad, asc = got[rows], ad[rows], asc[rows]
        e.update(row_ids=rows, res=None if e["res"] is None else e["res"][rows])
    y64, S, T = C.reference(ad, wd, e, T=C.mx_block_term(ad, wd, *fmts, asc, wsc))
    fam = torch.full(got.shape, C.MIXED, device=got.device)
    C.check(name, got.contiguous(), y64, S, K, fam, restated=C.restate(ad, wd, e) if K == 12288 else None, ops=C.epilogue_ops(e),
            act=act, exact=(), T=T)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,K", [(300, 3072), (17, 12288), (5, 128), (64, 1152)])
def test_quantize_mx_matches_the_definition_byte_for_byte(dev, fmt, M, K):
    from bind_your_avatar_implementation_amd import ops
    x = hard_inputs(M, K, seed=M + K)
    codes, scales = ops.quantize_mx(x.to(dev), fmt)
    c_ref, s_ref = quant_mx_ref(x, fmt)
    assert codes.shape == (M, K * BITS[fmt] // 8) and scales.shape == (M, K // 32)
    assert torch.equal(scales.cpu(), s_ref)
    same = codes.cpu() == c_ref
    print(f"{fmt} {M}x{K}: {int((~same).sum())} of {same.numel()} code bytes differ")
    assert same.all()
    # a strided batch view of the same rows: the row stride is honoured
    wide = torch.zeros(M, K + 128, dtype=torch.bfloat16, device=dev)
    wide[:, :K] = x.to(dev)
    c2, s2 = ops.quantize_mx(wide[:, :K], fmt)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


@pytest.mark.parametrize("fmt", FORMATS)
def test_layernorm_mx_equals_layernorm_then_quantiser(dev, fmt):
    """bya_layernorm_mx is bya_layernorm (AdaLN-modulated, text / video split, CFG batch of 2) followed by bya_quantize_mx,
    byte for byte."""
    from bind_your_avatar_implementation_amd import ops
    B, S, D, split = 2, 600, 3072, 226
    x = (rnd((B, S, D), 1, std=2.0).float() + 4.0 * rnd((D,), 2).float()).to(torch.bfloat16).to(dev)   # outlier channels
    w, b = (1 + 0.1 * rnd((D,), 3).float()).to(torch.bfloat16).to(dev), rnd((D,), 4).to(dev)
    mo = rnd((B, 4 * D), 5, std=0.5).to(dev)
    kw = dict(eps=1e-5, shift0=mo[:, 0:], scale0=mo[:, D:], shift1=mo[:, 2 * D:], scale1=mo[:, 3 * D:], split=split,
              mod_batch_stride=4 * D)
    y = torch.empty(B, S, D, dtype=torch.bfloat16, device=dev)
    ops.layernorm(x, y, w, b, **kw)
    c_ref, s_ref = ops.quantize_mx(y, fmt)
    codes = torch.empty_like(c_ref)
    scales = torch.empty_like(s_ref)
    ops.layernorm_mx(x, codes, scales, fmt, w, b, **kw)
    assert torch.equal(scales, s_ref)
    assert torch.equal(codes, c_ref)
    # and the GPU pair against the CPU restatement of the quantiser
    c_cpu, s_cpu = quant_mx_ref(y.cpu(), fmt)
    assert torch.equal(codes.cpu(), c_cpu) and torch.equal(scales.cpu(), s_cpu)


def exact_operand(rows, K, fmt, seed):
    """MX bytes of small exact values: elements in {0, +-0.5, +-1, +-1.5, +-2, +-3}, block scales 2^-2 .. 2^2."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0], dtype=torch.float64)
    el = vals[torch.randint(0, len(vals), (rows, K), generator=g)]
    scales = (127 + torch.randint(-2, 3, (rows, K // 32), generator=g)).to(torch.uint8)
    if fmt == "mxfp8":
        codes = el.float().to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        codes = pack6(e2m3_encode(el))
    assert torch.equal(dequant_mx(codes, scales, fmt), torch.ldexp(el.reshape(rows, -1, 32),
                       (scales.long() - 127)[..., None].double()).reshape(rows, K))
    return codes, scales


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,K", [(200, 144, 512), (37, 400, 384), (130, 20, 128)])
def test_gemm_mx_operand_map_on_exact_data(dev, fmt, M, N, K):
    """Every product is a multiple of 2^-6 below 2^7, every sum of K of them exact in fp32: the only rounding is the final
    one to bf16, so the result must EQUAL the exact product rounded to bf16.  A wrong lane -> K-block -> scale-byte map, or
    a wrong fp6 bit order, changes almost every element."""
    from bind_your_avatar_implementation_amd import ops
    ac, asc = exact_operand(M, K, fmt, seed=M)
    wc, wsc = exact_operand(N, K, fmt, seed=N + 1)
    ref = dequant_mx(ac, asc, fmt) @ dequant_mx(wc, wsc, fmt).T
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.gemm_mx(ac.to(dev), asc.to(dev), wc.to(dev), wsc.to(dev), out, fmt)
    got = out.cpu()
    bad = got.float() != ref.to(torch.bfloat16).float()
    print(f"{fmt} {M}x{N}x{K}: {int(bad.sum())} of {bad.numel()} elements differ")
    assert not bad.any()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("M,N,K,kw", [
    (17776, 9216, 3072, {"bias": True, "split": True}),        # attn1 q|k|v (three outputs)
    (17776, 3072, 3072, {"bias": True, "gate_res": True}),     # attn1.to_out (gated residual)
    (17776, 12288, 3072, {"bias": True, "act": "gelu_tanh"}),  # ff.net.0
    (2221, 3072, 12288, {"bias": True, "gate_res": True}),     # ff.net.2 -- odd row count (tail rows), K = 12288
    (2222, 9216, 3072, {}),
])
def test_gemm_mx_vs_exact_product_of_the_same_bytes(dev, fmt, M, N, K, kw):
    from bind_your_avatar_implementation_amd import ops
    a = hard_inputs(M, K, seed=7).to(dev)
    w = rnd((N, K), 3, std=K ** -0.5).to(dev)
    bias = rnd((N,), 4).to(dev) if kw.get("bias") else None
    ac, asc = ops.quantize_mx(a, fmt)
    wc, wsc = ops.quantize_mx(w, fmt)
    ad, wd = dequant_mx(ac, asc, fmt), dequant_mx(wc, wsc, fmt)
    ref = ad @ wd.T                                                                      # fp64, on the device
    if bias is not None:
        ref = ref + bias.double()
    if kw.get("act") == "gelu_tanh":
        ref = F.gelu(ref, approximate="tanh")
    args = {}
    if kw.get("gate_res"):
        gate, res = rnd((2, N), 5).to(dev), rnd((M, N), 6).to(dev)
        split_row = 226
        g = torch.where(torch.arange(M, device=dev)[:, None] < split_row, gate[0].double()[None], gate[1].double()[None])
        ref = res.double() + g * ref
        args = dict(res=res, gate0=gate[0].contiguous(), gate1=gate[1].contiguous(), gate_split=split_row)
    if kw.get("split"):
        out = torch.empty(3, M, N // 3, dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac, asc, wc, wsc, out[0], fmt, bias=bias, split=(N // 3, M * (N // 3)))
        got = out.permute(1, 0, 2).reshape(M, N)
    else:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac, asc, wc, wsc, out, fmt, bias=bias, act=kw.get("act"), **args)
        got = out
    err = rel_fro(got.float(), ref.to(torch.bfloat16).float())
    print(f"{fmt} {M}x{N}x{K} {kw}: rel-Fro vs bf16(exact) = {err:.3e}")
    assert err <= 1e-3
    # the Frobenius bar sees row 3 alone (its 1e30 block carries the whole norm: test_gemm_cond_cpu.py); every element:
    check_vs_fp64(f"{fmt} {M}x{N}x{K} {kw}", got, ad, wd, K, bias, kw.get("act"), args, (fmt, fmt), (asc, wsc))


def test_gemm_mx_batched_operands(dev):
    """batch > 1 (the CFG pair as grid.z): A codes and A scales advance per batch entry."""
    from bind_your_avatar_implementation_amd import ops
    fmt = "mxfp6"
    a = rnd((2, 300, 1024), 8).to(dev)
    w = rnd((256, 1024), 9, std=1024 ** -0.5).to(dev)
    ac, asc = ops.quantize_mx(a, fmt)
    wc, wsc = ops.quantize_mx(w, fmt)
    out = torch.empty(2, 300, 256, dtype=torch.bfloat16, device=dev)
    ops.gemm_mx(ac, asc, wc, wsc, out, fmt)
    for z in range(2):
        one = torch.empty(300, 256, dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac[z].contiguous(), asc[z].contiguous(), wc, wsc, one, fmt)
        assert torch.equal(out[z], one)


@pytest.mark.parametrize("fmt", FORMATS)
def test_gemm_mx_row_chunks_past_2gib_on_exact_data(dev, fmt):
    """An MX launch cut into row chunks: ``out`` is the first 128 columns of rows 2^21 + 64 elements (4 MiB + 128 bytes) apart,
    so row 512 starts at byte offset 2^31 + 65536 -- past the reach of the epilogue's buffer descriptor -- and the launch runs as
    pieces of 256, 256 and 1 rows.  Each piece must start at ITS rows of the one-byte codes (row0 * lda bytes), of the scale bytes
    (row0 * K / 32) and of the output: on exact data (operand-map test above) a piece fed another piece's rows or scales is wrong
    in almost every element.  The rest of the buffer holds a canary."""
    from bind_your_avatar_implementation_amd import ops
    M, N, K, LD = 513, 128, 128, 2 ** 21 + 64
    ac, asc = exact_operand(M, K, fmt, seed=11)
    wc, wsc = exact_operand(N, K, fmt, seed=12)
    meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")
    plan = ops.gemm_mx_plan(meta(ac), meta(asc), meta(wc), meta(wsc), torch.empty(M, LD, dtype=torch.bfloat16, device="meta")[:, :N], fmt)
    assert plan["row_chunks"] == 3 and plan["m0"] == 0, plan             # (needs no GPU: 256 + 256 + 1 rows)
    buf = torch.full((M, LD), SENTINEL, dtype=torch.int16, device=dev)
    out = buf.view(torch.bfloat16)[:, :N]
    assert ops.gemm_mx_plan(ac.to(dev), asc.to(dev), wc.to(dev), wsc.to(dev), out, fmt) == plan
    ops.gemm_mx(ac.to(dev), asc.to(dev), wc.to(dev), wsc.to(dev), out, fmt)
    ref = dequant_mx(ac, asc, fmt) @ dequant_mx(wc, wsc, fmt).T
    assert_exact(out.cpu(), ref, plan, f"{fmt} {M}x{N}x{K}, ldc {LD}")
    rows = torch.tensor([0, 255, 256, 511, 512], device=dev)
    assert bool((buf[rows, N:N + 64] == SENTINEL).all()), "canary behind the output columns"


# ------------------------------------------------------------------------------------------ forward level
class FakeMXLinear(torch.nn.Module):
    """bya_gemm_mx's definition on one nn.Linear of the CPU oracle: MX blocks of x and of W, exact products, then bias."""

    def __init__(self, lin, fmt):
        super().__init__()
        self.lin, self.fmt = lin, fmt

    def forward(self, x):
        xd = dequant_mx(*quant_mx_ref(x, self.fmt), self.fmt)
        wd = dequant_mx(*quant_mx_ref(self.lin.weight, self.fmt), self.fmt)
        y = (xd @ wd.T).float()
        if self.lin.bias is not None:
            y = y + self.lin.bias.float()
        return y.to(x.dtype)


def with_mx_dit_linears(orc, fmt):
    """The engine's default set (engine.FP8_DEFAULT: the four DiT Linears)."""
    for blk in orc.transformer_blocks:
        at = blk.attn1
        at.to_q, at.to_k, at.to_v = FakeMXLinear(at.to_q, fmt), FakeMXLinear(at.to_k, fmt), FakeMXLinear(at.to_v, fmt)
        at.to_out[0] = FakeMXLinear(at.to_out[0], fmt)
        blk.ff.net[0].proj = FakeMXLinear(blk.ff.net[0].proj, fmt)
        blk.ff.net[2] = FakeMXLinear(blk.ff.net[2], fmt)
    return orc


# Upper caps of the 2-layer output drift, engine(MX) against engine(bf16), on this test's random-init model: about twice
# what the engine measured (mxfp6 1.43e-2, mxfp8 1.43e-2 -- at this depth the bf16 rounding around the Linears, which
# differs between the two engines, weighs as much as the element format).  The floor shows the mode was in use.
DRIFT_CAP = {"mxfp6": 3e-2, "mxfp8": 3e-2}


@pytest.mark.parametrize("fmt", FORMATS)
def test_forward_with_mx_weights_vs_fake_quantised_oracle(dev, fmt):
    """Small geometry (3 x 8 x 12 video tokens + 226 text rows, full 3072-wide model, 2 layers, 2 identities, CFG batch of
    2): the engine with MX weights on the default Linears against the CPU oracle whose DiT Linears are replaced by the MX
    definition.  Bar at every tap, as for fp8: err(engine, fp32 oracle) <= 1.5 x err(oracle run in bf16, fp32 oracle) + 1e-3.
    Then: graph replay equals eager bit for bit, and turning the mode off gives the never-enabled bf16 engine bit for bit."""
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from oracle.model import OracleTransformer
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    sd = {k: v.float().cpu() for k, v in model.state_dict().items()}
    with torch.device("meta"):
        orc = OracleTransformer(**SMALL_KW)
    orc = orc.to_empty(device="cpu")
    orc.load_state_dict(sd, strict=True)
    orc.eval()
    inp = synth_inputs(batch=2, frames=3, height=16, width=24, seed=3, uncond_first=True)
    gi = to_dev(inp, dev)
    out_bf16 = model(**gi)[0].float().cpu()
    taps32, taps16, tapsg = {}, {}, {}
    with torch.no_grad():
        orc = with_mx_dit_linears(orc, fmt)
        ref = orc(taps=taps32, **inp)[0]
        orc16 = orc.to(torch.bfloat16)
        inp16 = {k: (v.to(torch.bfloat16) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
        inp16["id_cond"] = [t.to(torch.bfloat16) for t in inp["id_cond"]]
        inp16["id_vit_hidden"] = [[t.to(torch.bfloat16) for t in l] for l in inp["id_vit_hidden"]]
        ref16 = orc16(taps=taps16, **inp16)[0]
    model.enable_mx_weights(fmt)
    out = model(**gi)[0]
    assert model._engine.w8 is None and set(model._engine.wmx) == {"qkv", "out", "ff1", "ff2"}
    model._engine.step(gi["hidden_states"], gi["encoder_hidden_states"], gi["timestep"], gi["image_rotary_emb"],
                       gi["id_cond"], gi["id_vit_hidden"], gi["audio_embeds"], gi["af_matrix"], None, taps=tapsg)
    for name in ["block0", "face0", "audio0", "block1", "audio1"]:
        g, r32, r16 = tapsg[name].float().cpu(), taps32[name].float(), taps16[name].float()
        e_g, e_16 = rel_fro(g, r32), rel_fro(r16, r32)
        print(f"{name:8s} engine({fmt})-vs-fp32({fmt}) {e_g:.3e}   bf16({fmt})-oracle-vs-fp32({fmt}) {e_16:.3e}")
        assert e_g <= 1.5 * e_16 + 1e-3, name
    e_g, e_16 = rel_fro(out, ref), rel_fro(ref16, ref)
    print(f"output   engine({fmt})-vs-fp32({fmt}) {e_g:.3e}   bf16({fmt})-oracle-vs-fp32({fmt}) {e_16:.3e}")
    assert e_g <= 1.5 * e_16 + 1e-3
    drift = rel_fro(out.float().cpu(), out_bf16)
    print(f"{fmt} engine vs bf16 engine after 2 layers: {drift:.3e} (cap {DRIFT_CAP[fmt]:.1e})")
    assert 1e-3 < drift < DRIFT_CAP[fmt]
    # graph replay of the MX step: bit for bit the eager result
    eager = out.clone()
    model.use_hip_graph = True
    try:
        model(**gi)                                                         # capture
        for _ in range(2):
            assert torch.equal(model(**gi)[0], eager)
    finally:
        model.use_hip_graph = False
        model._graphs = {}
    model.enable_mx_weights(fmt, enabled=False)
    assert model._engine is None
    assert torch.equal(model(**gi)[0].float().cpu(), out_bf16)            # and back: bit-identical bf16 engine


def test_mx_linear_selection_and_conflicts(dev):
    """enable_mx_weights(linears=...) packs exactly the chosen kinds; fp8 and MX weights together refuse to build."""
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=2, fast=True)
    gi = to_dev(synth_inputs(batch=1, frames=3, height=16, width=24, seed=3), dev)
    model.enable_mx_weights("mxfp8", linears=("ff1", "aq"))
    model(**gi)
    assert set(model._engine.wmx) == {"ff1", "aq"} and model._engine.w8 is None
    model.enable_mx_weights("mxfp6", linears="all")
    model(**gi)
    assert set(model._engine.wmx) == {"qkv", "out", "ff1", "ff2", "pq", "aq"}
    assert all(len(pair) == 2 for v in model._engine.wmx.values() for pair in v)              # (codes, scales) per layer
    model.enable_mx_weights("mxfp6", linears=("out",))
    model(**gi)
    assert set(model._engine.wmx) == {"out"}
    c, s = model._engine.wmx["out"][0]
    assert c.shape == (3072, 3072 * 6 // 8) and s.shape == (3072, 96)
    with pytest.raises(ValueError):
        model.enable_mx_weights("mxfp4")
    model.enable_mx_weights("mxfp6", linears=("qkv", "nope"))
    with pytest.raises(ValueError):
        model(**gi)
    model.enable_mx_weights("mxfp6")
    model.enable_fp8_weights()
    with pytest.raises(ValueError, match="fp8.*MX"):
        model(**gi)
    model.enable_fp8_weights(False)
    model(**gi)
    assert set(model._engine.wmx) == {"qkv", "out", "ff1", "ff2"} and model._engine.w8 is None
