"""MXFP4 (e2m1) weights under MXFP6 / MXFP8 activations (include/bya.h, "MX weights"; bya_gemm_mx_mixed;
enable_mx_weights(weight_format="mxfp4")): the weight quantiser byte for byte against the CPU restatement of
tests/test_mxfp4_cpu.py, the mixed instruction's operand map on exact data, the GEMM against the exact product of the very
bytes it multiplied, and the engine stage by stage against the CPU oracle whose DiT Linears are fake-quantised with
activations in the activation format and weights in e2m1."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_fro
from test_mx_gpu import check_vs_fp64, exact_operand, hard_inputs, rnd
from test_mxfp4_cpu import dequant, e2m1_encode, pack4, quant_ref

pytestmark = pytest.mark.gpu

ACT_FORMATS = ("mxfp6", "mxfp8")


@pytest.mark.parametrize("M,K", [(300, 3072), (5, 128), (64, 1152)])
def test_quantize_mxfp4_matches_the_definition_byte_for_byte(dev, M, K):
    from bind_your_avatar_implementation_amd import ops
    x = hard_inputs(M, K, seed=M + K)
    codes, scales = ops.quantize_mx(x.to(dev), "mxfp4")
    c_ref, s_ref = quant_ref(x, "mxfp4")
    assert codes.shape == (M, K // 2) and scales.shape == (M, K // 32)
    assert torch.equal(scales.cpu(), s_ref)
    same = codes.cpu() == c_ref
    print(f"mxfp4 {M}x{K}: {int((~same).sum())} of {same.numel()} code bytes differ")
    assert same.all()
    # a strided view of the same rows: the row stride is honoured
    wide = torch.zeros(M, K + 128, dtype=torch.bfloat16, device=dev)
    wide[:, :K] = x.to(dev)
    c2, s2 = ops.quantize_mx(wide[:, :K], "mxfp4")
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


def exact_weights_e2m1(rows, K, seed):
    """exact_operand of tests/test_mx_gpu.py in e2m1: elements in {0, +-0.5, +-1, +-1.5, +-2, +-3}, block scales 2^-2 .. 2^2."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0], dtype=torch.float64)
    el = vals[torch.randint(0, len(vals), (rows, K), generator=g)]
    scales = (127 + torch.randint(-2, 3, (rows, K // 32), generator=g)).to(torch.uint8)
    codes = pack4(e2m1_encode(el))
    assert torch.equal(dequant(codes, scales, "mxfp4"), torch.ldexp(el.reshape(rows, -1, 32),
                       (scales.long() - 127)[..., None].double()).reshape(rows, K))
    return codes, scales


@pytest.mark.parametrize("fmt", ACT_FORMATS)
@pytest.mark.parametrize("M,N,K,expect", [(200, 144, 512, "t128x128"), (37, 400, 384, "t128x128"), (130, 20, 128, "t128x128"),
                                          (3500, 3700, 256, {"mxfp6": "t256x256", "mxfp8": "t128x128"})])
def test_mixed_gemm_operand_map_on_exact_data(dev, fmt, M, N, K, expect):
    """Every product is a multiple of 2^-6 below 2^7, every sum of K <= 512 of them exact in fp32: the only rounding is the
    final one to bf16, so the result must EQUAL the exact product rounded to bf16.  A wrong nibble order, lane -> K-block
    map or scale byte of the e2m1 operand changes almost every element.  The last shape is the smallest launch that reaches
    the 256 x 256 tile of e2m3 activations (14 x 15 = 210 >= 200 tiles), ragged in both directions."""
    from bind_your_avatar_implementation_amd import ops
    ac, asc = exact_operand(M, K, fmt, seed=M)
    wc, wsc = exact_weights_e2m1(N, K, seed=N + 1)
    ref = dequant(ac, asc, fmt).to(dev) @ dequant(wc, wsc, "mxfp4").to(dev).T
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    args = (ac.to(dev), asc.to(dev), wc.to(dev), wsc.to(dev), out, fmt)
    assert ops.gemm_mx_plan(*args, w_fmt="mxfp4")["path"] == (expect if isinstance(expect, str) else expect[fmt])
    ops.gemm_mx(*args, w_fmt="mxfp4")
    bad = out.float() != ref.to(torch.bfloat16).float()
    print(f"{fmt} x mxfp4 {M}x{N}x{K}: {int(bad.sum())} of {bad.numel()} elements differ")
    assert not bad.any()


@pytest.mark.parametrize("fmt", ACT_FORMATS)
@pytest.mark.parametrize("M,N,K,kw", [
    (300, 384, 3072, {"bias": True, "split": True}),           # three outputs (attn1 q|k|v's epilogue)
    (290, 256, 1024, {"bias": True, "gate_res": True}),        # gated residual, gate changes at row 226
    (130, 512, 3072, {"bias": True, "act": "gelu_tanh"}),
    (130, 128, 12288, {"bias": True}),                         # the longest K of the model
])
def test_mixed_gemm_vs_exact_product_of_the_same_bytes(dev, fmt, M, N, K, kw):
    from bind_your_avatar_implementation_amd import ops
    a = hard_inputs(M, K, seed=7).to(dev)
    w = rnd((N, K), 3, std=K ** -0.5).to(dev)
    bias = rnd((N,), 4).to(dev)
    ac, asc = ops.quantize_mx(a, fmt)
    wc, wsc = ops.quantize_mx(w, "mxfp4")
    ad, wd = dequant(ac, asc, fmt), dequant(wc, wsc, "mxfp4")
    ref = ad @ wd.T + bias.double()                                                      # fp64, on the device
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
        ops.gemm_mx(ac, asc, wc, wsc, out[0], fmt, bias=bias, split=(N // 3, M * (N // 3)), w_fmt="mxfp4")
        got = out.permute(1, 0, 2).reshape(M, N)
    else:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac, asc, wc, wsc, out, fmt, bias=bias, act=kw.get("act"), w_fmt="mxfp4", **args)
        got = out
    err = rel_fro(got.float(), ref.to(torch.bfloat16).float())
    print(f"{fmt} x mxfp4 {M}x{N}x{K} {kw}: rel-Fro vs bf16(exact) = {err:.3e}")
    assert err <= 1e-3
    check_vs_fp64(f"{fmt} x mxfp4 {M}x{N}x{K} {kw}", got, ad, wd, K, bias, kw.get("act"), args, (fmt, "mxfp4"), (asc, wsc))


@pytest.mark.parametrize("fmt", ACT_FORMATS)
def test_mixed_gemm_batched_operands(dev, fmt):
    """batch > 1 (the CFG pair as grid.z): A codes and A scales advance per batch entry, the e2m1 weights are shared."""
    from bind_your_avatar_implementation_amd import ops
    a = rnd((2, 300, 1024), 8).to(dev)
    w = rnd((256, 1024), 9, std=1024 ** -0.5).to(dev)
    ac, asc = ops.quantize_mx(a, fmt)
    wc, wsc = ops.quantize_mx(w, "mxfp4")
    out = torch.empty(2, 300, 256, dtype=torch.bfloat16, device=dev)
    ops.gemm_mx(ac, asc, wc, wsc, out, fmt, w_fmt="mxfp4")
    wd = dequant(wc, wsc, "mxfp4")
    for z in range(2):
        ref = dequant(ac[z], asc[z], fmt) @ wd.T
        err = rel_fro(out[z].float(), ref.to(torch.bfloat16).float())
        print(f"{fmt} x mxfp4 batch entry {z}: rel-Fro vs bf16(exact) = {err:.3e}")
        assert err <= 1e-3
        one = torch.empty(300, 256, dtype=torch.bfloat16, device=dev)
        ops.gemm_mx(ac[z].contiguous(), asc[z].contiguous(), wc, wsc, one, fmt, w_fmt="mxfp4")
        assert torch.equal(out[z], one)


# ------------------------------------------------------------------------------------------ forward level
class FakeMixedMXLinear(torch.nn.Module):
    """bya_gemm_mx_mixed's definition on one nn.Linear of the CPU oracle: MX blocks of x in ``fmt``, of W in e2m1, exact
    products, then bias."""

    def __init__(self, lin, fmt):
        super().__init__()
        self.lin, self.fmt = lin, fmt

    def forward(self, x):
        xd = dequant(*quant_ref(x, self.fmt), self.fmt)
        wd = dequant(*quant_ref(self.lin.weight, "mxfp4"), "mxfp4")
        y = (xd @ wd.T).float()
        if self.lin.bias is not None:
            y = y + self.lin.bias.float()
        return y.to(x.dtype)


def with_mixed_dit_linears(orc, fmt):
    """The engine's default set (engine.FP8_DEFAULT: the four DiT Linears)."""
    for blk in orc.transformer_blocks:
        at = blk.attn1
        at.to_q, at.to_k, at.to_v = (FakeMixedMXLinear(l, fmt) for l in (at.to_q, at.to_k, at.to_v))
        at.to_out[0] = FakeMixedMXLinear(at.to_out[0], fmt)
        blk.ff.net[0].proj = FakeMixedMXLinear(blk.ff.net[0].proj, fmt)
        blk.ff.net[2] = FakeMixedMXLinear(blk.ff.net[2], fmt)
    return orc


# Upper caps of the 2-layer output drift, engine(MX activations x e2m1 weights) against engine(bf16), on this test's
# random-init model: about twice what the engine measured on its first GPU run (MEASURED_DRIFT).  The floor shows the mode
# was in use.
MEASURED_DRIFT = {"mxfp6": 3.339e-2, "mxfp8": 3.331e-2}       # (same-format weights: 1.43e-2 for both, tests/test_mx_gpu.py)
DRIFT_CAP = {"mxfp6": 7e-2, "mxfp8": 7e-2}


@pytest.mark.parametrize("fmt", ACT_FORMATS)
def test_forward_with_mxfp4_weights_vs_fake_quantised_oracle(dev, fmt):
    """The geometry and structure of tests/test_mx_gpu.py's forward test (3 x 8 x 12 video tokens + 226 text rows, full
    3072-wide model, 2 layers, 2 identities, CFG batch of 2) with weight_format="mxfp4": the engine against the CPU oracle
    whose DiT Linears are replaced by the mixed MX definition.  Bar at every tap and at the output:
    err(engine, fp32 oracle) <= 1.5 x err(oracle run in bf16, fp32 oracle) + 1e-3.  Then: the packed weights are 4-bit, graph
    replay equals eager bit for bit, and turning the mode off gives the never-enabled bf16 engine bit for bit."""
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
        orc = with_mixed_dit_linears(orc, fmt)
        ref = orc(taps=taps32, **inp)[0]
        orc16 = orc.to(torch.bfloat16)
        inp16 = {k: (v.to(torch.bfloat16) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
        inp16["id_cond"] = [t.to(torch.bfloat16) for t in inp["id_cond"]]
        inp16["id_vit_hidden"] = [[t.to(torch.bfloat16) for t in l] for l in inp["id_vit_hidden"]]
        ref16 = orc16(taps=taps16, **inp16)[0]
    model.enable_mx_weights(fmt, weight_format="mxfp4")
    out = model(**gi)[0]
    eng = model._engine
    assert eng.w8 is None and set(eng.wmx) == {"qkv", "out", "ff1", "ff2"} and (eng.mx_fmt, eng.mx_wfmt) == (fmt, "mxfp4")
    c, s = eng.wmx["out"][0]
    assert c.shape == (3072, 1536) and s.shape == (3072, 96) and c.dtype == s.dtype == torch.uint8
    eng.step(gi["hidden_states"], gi["encoder_hidden_states"], gi["timestep"], gi["image_rotary_emb"],
             gi["id_cond"], gi["id_vit_hidden"], gi["audio_embeds"], gi["af_matrix"], None, taps=tapsg)
    for name in ["block0", "face0", "audio0", "block1", "audio1"]:
        g, r32, r16 = tapsg[name].float().cpu(), taps32[name].float(), taps16[name].float()
        e_g, e_16 = rel_fro(g, r32), rel_fro(r16, r32)
        print(f"{name:8s} engine({fmt} x mxfp4)-vs-fp32 {e_g:.3e}   bf16-oracle-vs-fp32 {e_16:.3e}")
        assert e_g <= 1.5 * e_16 + 1e-3, name
    e_g, e_16 = rel_fro(out, ref), rel_fro(ref16, ref)
    print(f"output   engine({fmt} x mxfp4)-vs-fp32 {e_g:.3e}   bf16-oracle-vs-fp32 {e_16:.3e}")
    assert e_g <= 1.5 * e_16 + 1e-3
    drift = rel_fro(out.float().cpu(), out_bf16)
    print(f"{fmt} x mxfp4 engine vs bf16 engine after 2 layers: {drift:.3e} (cap {DRIFT_CAP[fmt]:.1e})")
    assert 1e-3 < drift < DRIFT_CAP[fmt]
    # graph replay of the step: bit for bit the eager result
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


def test_mxfp4_linear_selection(dev):
    """enable_mx_weights(linears=("ff1",), weight_format="mxfp4") packs only that kind, in e2m1; weight_format=None packs the
    activations' format as before."""
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=2, fast=True)
    gi = to_dev(synth_inputs(batch=1, frames=3, height=16, width=24, seed=3), dev)
    model.enable_mx_weights("mxfp8", linears=("ff1",), weight_format="mxfp4")
    model(**gi)
    assert set(model._engine.wmx) == {"ff1"} and model._engine.w8 is None
    c, s = model._engine.wmx["ff1"][0]
    assert c.shape == (12288, 1536) and s.shape == (12288, 96)
    model.enable_mx_weights("mxfp6", linears=("ff1",))
    model(**gi)
    c, s = model._engine.wmx["ff1"][0]
    assert c.shape == (12288, 3072 * 6 // 8) and model._engine.mx_wfmt == "mxfp6"
