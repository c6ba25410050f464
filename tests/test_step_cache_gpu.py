"""GPU: the first-block step cache (include/bya.h "First-block step cache").

Kernels: ``ops.step_cache_probe`` / ``_capture`` / ``_apply`` against the torch restatement (tests/step_cache_ref.py, kept
on the CPU) -- every written tensor bit for bit, the probe's two sums within 2^-22 relative of fp64 (a term is one fp32
subtraction of two bf16 values: relative error <= 2^-24; an fp64 sum of n <= 2^27 non-negative terms adds <= 2^-26), the same
16 bytes from three launches, guard bytes around every output, and the refusals with nothing written.

Engine: the tests' 2-layer model (SMALL_KW of tests/test_forward_gpu.py) on the guided step's [uncond, cond] pair, bf16 and MX
weights: threshold 0 is the uncached step bit for bit plus exactly the cache's launches; a re-used step is the prefix through
block 0, the probe, the apply and the head; the hit cap; what drops the state; a 6-step guided clip through the pipeline."""
import math
import statistics

import pytest
import torch
import torch.nn.functional as F

import step_cache_ref as ref
from conftest import rel_fro
from test_batch_engine_gpu import cfg_inputs
from test_engine_launch_order_gpu import recorded
from test_forward_gpu import SMALL_KW, to_dev

pytestmark = pytest.mark.gpu

GUARD = 256            # bytes of 0xA5 either side of every output
BF = torch.bfloat16


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Guarded:
    """A device tensor inside a buffer with GUARD bytes of 0xA5 in front of it and behind it."""

    def __init__(self, src, dev):
        nbytes = src.numel() * src.element_size()
        self.buf = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=dev)
        self.t = self.buf[GUARD:GUARD + nbytes].view(src.dtype).view(src.shape)
        self.t.copy_(src)
        self.nbytes = nbytes

    def intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all() and (self.buf[GUARD + self.nbytes:] == 0xA5).all())


def plan_sized_elements():
    """n at which every workgroup of the probe walks two full passes and a partial third: twice the grid cap's pass, then
    1000 of its 2048 workgroups with a whole pass more, one with 37 vectors, the rest with none."""
    from bind_your_avatar_implementation_amd import ops
    meta = lambda n: torch.empty(n, dtype=BF, device="meta")
    cap = ops.step_cache_probe_plan(meta(1 << 26), meta(1 << 26), None, meta(1 << 26))
    per_pass = cap["grid"] * cap["wg_pass_elems"]
    n = 2 * per_pass + 1000 * cap["wg_pass_elems"] + 37 * cap["vec"]
    plan = ops.step_cache_probe_plan(meta(n), meta(n), None, meta(n))
    assert plan["grid"] == cap["grid"] and plan["passes"] == 3 and n % per_pass != 0 and n * 2 <= 64 << 20
    return n


SHAPES = {"one_vector": (1, 1, 8), "small": (1, 3, 64), "ragged": (2, 37, 192), "small_model_stream": (1, 514, 3072),
          "three_passes": None}
DATA = ("gaussian", "zero_stretch", "signed_zeros", "ref_all_zero", "nan", "huge", "no_ref")
_CASES = {}


def case(shape_name, data):
    """-> the CPU operands of one case and what the restatement makes of them (computed once, shared, never written)."""
    key = (shape_name, data)
    if key in _CASES:
        return _CASES[key]
    shape = SHAPES[shape_name] or (plan_sized_elements(),)
    g = torch.Generator().manual_seed(1000 + 17 * list(SHAPES).index(shape_name) + DATA.index(data))
    rnd = lambda s=1.0: (s * torch.randn(shape, generator=g)).to(BF)
    x, E, r_ref, x2 = rnd(), rnd(), rnd(0.5), rnd()
    n = x.numel()
    flat = lambda t: t.view(-1)
    if data == "zero_stretch":
        flat(r_ref)[n // 3:max(n // 3 + 1, 2 * n // 3)] = 0
    elif data == "signed_zeros":
        flat(x)[0::2], flat(x)[1::4] = 0.0, -0.0
        flat(E)[0::3], flat(E)[1::3] = -0.0, 0.0
        flat(r_ref)[0::5] = -0.0
        flat(x2)[0::2] = -0.0
    elif data == "ref_all_zero":
        r_ref.zero_()
    elif data == "nan":
        flat(x)[n // 2] = float("nan")
    elif data == "huge":
        x, E, r_ref, x2 = (t * 2.0 ** 100 for t in (x, E, r_ref, x2))
        assert x.dtype == BF and x.float().abs().max() > 2.0 ** 100
    elif data == "no_ref":
        r_ref = None
    r_new, E_new, num, den = ref.probe(x, E, r_ref)
    R = ref.capture(x2, E_new)
    out = dict(x=x, E=E, r_ref=r_ref, x2=x2, r_new=r_new, E_new=E_new, num=num, den=den, R=R, applied=ref.apply(x, R))
    _CASES[key] = out
    return out


def close(got, want):
    """within 2^-22 relative of the fp64 restatement; NaN where it is NaN; exactly 0 where it is 0"""
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= 2.0 ** -22 * abs(want)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_kernels_against_the_restatement(dev, shape_name, data):
    from bind_your_avatar_implementation_amd import ops
    c = case(shape_name, data)
    x, x2 = c["x"].to(dev), c["x2"].to(dev)
    r_ref = None if c["r_ref"] is None else c["r_ref"].to(dev)
    plan = ops.step_cache_probe_plan(x, x, r_ref, x)
    n = x.numel()
    assert plan["grid"] == min(2048, -(-n // 2048)) and plan["vec"] == 8 and plan["wg_pass_elems"] == 2048
    sums_seen = []
    for _ in range(3):                                     # three launches on the same inputs: the same 16 bytes
        E, r_new = Guarded(c["E"], dev), Guarded(torch.zeros_like(c["x"]), dev)
        partials = Guarded(torch.full((plan["partials_bytes"] // 8,), -7.0, dtype=torch.float64), dev)
        sums = Guarded(torch.full((2,), -7.0, dtype=torch.float64), dev)
        ops.step_cache_probe(x, E.t, r_ref, r_new.t, partials.t, sums.t)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (E, r_new, partials, sums))
        sums_seen.append(sums.t.cpu().view(torch.int64).tolist())
    num, den = sums.t.tolist()
    print(f"{shape_name}/{data}: n={n} grid={plan['grid']} passes={plan['passes']} num={num!r} (fp64 {c['num']!r}) den={den!r} "
          f"(fp64 {c['den']!r})")
    assert same_bits(x, c["x"])                            # the input is read only
    assert same_bits(r_new.t, c["r_new"]) and same_bits(E.t, c["E_new"])
    assert close(num, c["num"]) and close(den, c["den"])
    if data == "nan":
        assert math.isnan(num)
    if data in ("ref_all_zero", "no_ref"):
        assert den == 0.0 and (data == "ref_all_zero" or num == 0.0)
    assert sums_seen[0] == sums_seen[1] == sums_seen[2]
    # capture on the probe's E, apply on x
    R = Guarded(torch.zeros_like(c["x"]), dev)
    ops.step_cache_capture(x2, E.t, R.t)
    xa = Guarded(c["x"], dev)
    ops.step_cache_apply(xa.t, R.t)
    torch.cuda.synchronize()
    assert R.intact() and xa.intact() and E.intact()
    assert same_bits(R.t, c["R"]) and same_bits(xa.t, c["applied"]) and same_bits(E.t, c["E_new"])


def test_bad_alignment_and_length_are_refused_with_nothing_written(dev):
    from bind_your_avatar_implementation_amd import _hip, ops
    n = 64
    pool = torch.full((4, n + 16), 3.0, dtype=BF, device=dev)
    good = [pool[k, :n] for k in range(4)]
    off = [pool[k, 1:n + 1] for k in range(4)]             # 2 bytes off a 16-byte boundary
    assert all(t.data_ptr() % 16 == 0 for t in good) and all(t.data_ptr() % 16 == 2 for t in off)
    partials, sums = torch.full((2,), -7.0, dtype=torch.float64, device=dev), torch.full((2,), -7.0, dtype=torch.float64, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((pool == 3.0).all() and (partials == -7.0).all() and (sums == -7.0).all())

    for k in range(4):                                     # each operand of the probe in turn
        args = list(good)
        args[k] = off[k]
        with pytest.raises(_hip.ByaError, match="BYA_ERR_ALIGN"):
            ops.step_cache_probe(*args, partials, sums)
        assert untouched()
    for k in range(3):
        args = list(good[:3])
        args[k] = off[k]
        with pytest.raises(_hip.ByaError, match="BYA_ERR_ALIGN"):
            ops.step_cache_capture(*args)
        assert untouched()
    for k in range(2):
        args = list(good[:2])
        args[k] = off[k]
        with pytest.raises(_hip.ByaError, match="BYA_ERR_ALIGN"):
            ops.step_cache_apply(*args)
        assert untouched()
    short = [t[:12] for t in good]                         # n % 8 != 0
    with pytest.raises(_hip.ByaError, match="BYA_ERR_SHAPE"):
        ops.step_cache_probe(*short, partials, sums)
    with pytest.raises(_hip.ByaError, match="BYA_ERR_SHAPE"):
        ops.step_cache_capture(*short[:3])
    with pytest.raises(_hip.ByaError, match="BYA_ERR_SHAPE"):
        ops.step_cache_apply(*short[:2])
    assert untouched()
    lib = _hip.load()                                      # the fp64 pair: 8 bytes
    p = [t.data_ptr() for t in good]
    assert lib.bya_step_cache_probe(*p, partials.data_ptr() + 4, sums.data_ptr(), n, None) == -2
    assert lib.bya_step_cache_probe(*p, partials.data_ptr(), sums.data_ptr() + 4, n, None) == -2
    assert untouched()


# ------------------------------------------------------------------------------------------ the engine
SIX = ("qkv", "out", "ff1", "ff2", "po", "ao")
STEPS = 6


@pytest.fixture(scope="module", params=["bf16", "mx"])
def model(dev, request):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    m = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
    if request.param == "mx":
        m.enable_mx_weights("mxfp8", linears=SIX)
    return m


@pytest.fixture(scope="module")
def clip(dev):
    """The inputs of STEPS consecutive guided steps: the SAME conditioning tensors, latents that drift a little, falling
    timesteps."""
    base = cfg_inputs(dev, 31)
    g = torch.Generator().manual_seed(77)
    hs = base["hidden_states"]
    steps = []
    for k in range(STEPS):
        drift = (0.03 * k * torch.randn(hs.shape, generator=g)).to(dev, BF)
        t = torch.tensor([900 - 150 * k] * 2, dtype=torch.int64, device=dev)
        steps.append(dict(base, hidden_states=(hs + drift).contiguous(), timestep=t))
    return steps


def fresh(model, threshold=None, **kw):
    """The model with a new engine and the cache off (``threshold`` None) or enabled anew."""
    model.enable_step_cache(0.0, enabled=False)
    model.invalidate_engine()
    if threshold is not None:
        model.enable_step_cache(threshold, **kw)
    return model


def kinds(model, run):
    """``run()`` -> (its result, "F" or "R": what the step cache made of the ONE step it ran)."""
    before = model.step_cache_stats()
    out = run()
    after = model.step_cache_stats()
    assert after["steps"] == before["steps"] + 1 and len(after["distances"]) == after["steps"] == after["full"] + after["reused"]
    return out, "R" if after["reused"] > before["reused"] else "F"


CACHE_LAUNCHES = ("step_cache_snapshot", "bya_step_cache_probe", "bya_step_cache_capture", "bya_step_cache_apply")


def test_threshold_zero_is_the_uncached_step_plus_the_cache_launches(model, clip):
    fresh(model)
    model(**clip[0])                                        # builds the engine; not recorded
    off = [recorded(lambda k=k: model(**clip[k])[0].clone()) for k in range(2)]
    fresh(model, 0.0)
    model(**clip[0])
    model.reset_step_cache()
    on = [recorded(lambda k=k: model(**clip[k])[0].clone()) for k in range(2)]
    assert model.step_cache_stats()["full"] == 2 and model.step_cache_stats()["reused"] == 0
    assert model.step_cache_stats()["distances"][0] == math.inf and 0.0 < model.step_cache_stats()["distances"][1] < math.inf
    for k in range(2):
        assert same_bits(on[k][0], off[k][0]), f"step {k}"
        got, want = on[k][1]["launches"], off[k][1]["launches"]
        assert not any(name in CACHE_LAUNCHES for name in want)
        # exactly one snapshot copy, one probe (its entry point issues the pass and the one-workgroup finish) and one
        # capture, in that order; everything else is the uncached step's list, in its order
        assert [n_ for n_ in got if n_ in CACHE_LAUNCHES] == list(CACHE_LAUNCHES[:3])
        assert [n_ for n_ in got if n_ not in CACHE_LAUNCHES] == want
        assert on[k][1]["attn_variants"] == off[k][1]["attn_variants"]
    fresh(model)


def torch_head(model, eng, x, shape):
    """The step's head (final norm, AdaLN, projection, unpatchify) in fp32 torch on the resident stream ``x``."""
    B, T, _, Hh, Ww = shape
    D, f = eng.D, lambda p: p.float()
    xv = x[:, x.shape[1] - T * (Hh // 2) * (Ww // 2):].float()
    h = F.layer_norm(xv, (D,), f(model.norm_final.weight), f(model.norm_final.bias), model.norm_final.eps)
    no = model.norm_out
    shift, scale = F.linear(F.silu(eng._ws["emb"].float()), f(no.linear.weight), f(no.linear.bias)).chunk(2, dim=1)
    h = F.layer_norm(h, (D,), f(no.norm.weight), f(no.norm.bias), no.norm.eps) * (1 + scale[:, None]) + shift[:, None]
    y = F.linear(h, f(model.proj_out.weight), f(model.proj_out.bias))
    return y.reshape(B, T, Hh // 2, Ww // 2, -1, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)


def test_a_reused_step_is_block_zero_the_probe_the_apply_and_the_head(model, clip):
    shape = clip[1]["hidden_states"].shape
    # the same two steps uncached (the bar's yardstick) and with threshold 0 (the launch list to cut, and E)
    fresh(model)
    model(**clip[0])
    out_off = model(**clip[1])[0].clone()
    err_off = rel_fro(out_off, torch_head(model, model._engine, model._engine._ws["x"], shape))
    fresh(model, 0.0)
    model(**clip[0])
    model.reset_step_cache()
    model(**clip[0])
    _, rec0 = recorded(lambda: model(**clip[1])[0].clone())
    E0 = model._step_cache.E.clone()
    # threshold inf: step 1 is full (no reference), step 2 re-uses
    fresh(model, math.inf)
    _, k1 = kinds(model, lambda: model(**clip[0])[0])
    R1 = model._step_cache.R.clone()
    (out, rec), k2 = kinds(model, lambda: recorded(lambda: model(**clip[1])[0].clone()))
    assert (k1, k2) == ("F", "R")
    full = rec0["launches"]
    probe, capture = full.index("bya_step_cache_probe"), full.index("bya_step_cache_capture")
    block1 = full[probe + 1:capture]
    assert len(block1) > 10 and any("gemm" in n_ for n_ in block1)
    assert rec["launches"] == full[:probe + 1] + ["bya_step_cache_apply"] + full[capture + 1:]
    sc = model._step_cache
    assert same_bits(sc.E, E0)                              # x after block 0 does not depend on the cache's decision
    assert same_bits(sc.R, R1)                              # a re-used step leaves R alone
    x = model._engine._ws["x"]
    assert same_bits(x, ref.apply(E0.cpu(), R1.cpu()))
    err = rel_fro(out, torch_head(model, model._engine, x, shape))
    print(f"rel-Fro of the engine's head against fp32 torch on the same stream: re-used step {err:.3e}, uncached step {err_off:.3e}")
    assert err <= 1.5 * err_off + 1e-3
    assert torch.isfinite(out.float()).all()
    fresh(model)


def test_the_hit_cap_gives_f_r_r_f_r_r_twice_the_same(model, clip):
    runs = []
    for _ in range(2):
        fresh(model, math.inf, max_consecutive_hits=2)
        outs, pattern = [], ""
        for k in range(STEPS):
            out, kind = kinds(model, lambda k=k: model(**clip[k])[0].clone())
            outs.append(out)
            pattern += kind
        st = model.step_cache_stats()
        assert pattern == "FRRFRR" == ref.pattern(STEPS, 2)
        assert (st["steps"], st["full"], st["reused"]) == (6, 2, 4) and len(st["distances"]) == 6
        assert st["distances"][0] == math.inf and all(0.0 < d < math.inf for d in st["distances"][1:])
        runs.append((outs, st["distances"]))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert same_bits(a, b)
    assert runs[0][1] == runs[1][1]                         # the probe's sums too: the same doubles
    fresh(model)


def test_what_drops_the_state(model, clip):
    eng_step = lambda inp, taps: model._engine.step(inp["hidden_states"], inp["encoder_hidden_states"], inp["timestep"], inp["image_rotary_emb"],
                                                    inp["id_cond"], inp["id_vit_hidden"], inp["audio_embeds"], inp["af_matrix"], None, taps=taps)
    step = lambda inp: kinds(model, lambda: model(**inp)[0].clone())
    fresh(model, math.inf)
    assert [step(clip[k])[1] for k in range(3)] == ["F", "R", "R"]
    # another text tensor (the same values): the reference was taken under other conditioning inputs
    moved = dict(clip[3], encoder_hidden_states=clip[3]["encoder_hidden_states"].clone())
    assert step(moved)[1] == "F"
    assert step(dict(clip[4], encoder_hidden_states=moved["encoder_hidden_states"]))[1] == "R"
    # a taps= run bypasses the cache and leaves its state alone: the step behind it is what it is without the tap run
    fresh(model, math.inf)
    plain = [step(clip[k]) for k in range(3)]
    fresh(model, math.inf)
    tapped = [step(clip[k]) for k in range(2)]
    before, taps = model.step_cache_stats(), {}
    sc = model._step_cache
    held = (sc.has_ref, sc.hits, sc.R.clone(), sc.r_ref.clone())
    eng_step(clip[2], taps)
    assert "block1" in taps and model.step_cache_stats() == before          # every block ran, nothing was counted
    assert (sc.has_ref, sc.hits) == held[:2] and same_bits(sc.R, held[2]) and same_bits(sc.r_ref, held[3])
    tapped.append(step(clip[2]))
    assert [k for _, k in tapped] == [k for _, k in plain] == ["F", "R", "R"]
    assert all(same_bits(a, b) for (a, _), (b, _) in zip(tapped, plain))
    # reset_step_cache(), invalidate_engine() and another batch: a full step each
    model.reset_step_cache()
    assert model.step_cache_stats()["steps"] == 0 and step(clip[3])[1] == "F" and step(clip[4])[1] == "R"
    model.invalidate_engine()
    assert step(clip[5])[1] == "F" and step(clip[5])[1] == "R"
    one = {k: (v[1:] if torch.is_tensor(v) and v.shape[0] == 2 else v) for k, v in clip[5].items()}
    one["id_cond"] = [t[1:] for t in clip[5]["id_cond"]]
    one["id_vit_hidden"] = [[t[1:] for t in level] for level in clip[5]["id_vit_hidden"]]
    assert step(one)[1] == "F"
    fresh(model)


def test_a_guided_clip_through_the_pipeline(model, dev):
    from bind_your_avatar_implementation_amd.pipeline import BindyouravatarPipeline
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    inp = to_dev(synth_inputs(batch=1, frames=3, height=16, width=24, seed=11), dev)
    lat, img = inp["hidden_states"][:, :, :16].contiguous(), inp["hidden_states"][:, :, 16:32].contiguous()
    neg = torch.zeros_like(inp["encoder_hidden_states"])
    pipe = BindyouravatarPipeline(model)

    def run():
        return pipe(height=128, width=192, num_frames=9, num_inference_steps=STEPS, guidance_scale=3.0, latents=lat.clone(),
                    prompt_embeds=inp["encoder_hidden_states"], negative_prompt_embeds=neg, image_latents=img, image_bg_latents=img,
                    id_vit_hidden=inp["id_vit_hidden"], id_cond=inp["id_cond"], audio_embs=inp["audio_embeds"],
                    af_matrix=inp["af_matrix"], output_type="latent").frames
    fresh(model)
    want = run()
    fresh(model, 0.0)
    got = run()
    st = model.step_cache_stats()
    assert same_bits(got, want)
    assert (st["steps"], st["full"], st["reused"]) == (STEPS, STEPS, 0) and st["distances"][0] == math.inf
    threshold = statistics.median(st["distances"])          # (one of them is the first step's inf: the median is finite)
    assert 0.0 < threshold < math.inf
    fresh(model, threshold)
    cached = run()
    st2 = model.step_cache_stats()
    print(f"distances at threshold 0: {st['distances']}; threshold {threshold:.4g}: {st2['reused']} of {STEPS} steps re-used, "
          f"distances {st2['distances']}, rel-Fro of the latents against the uncached clip {rel_fro(cached, want):.3e}")
    assert st2["reused"] >= 1 and st2["steps"] == STEPS == st2["full"] + st2["reused"] == len(st2["distances"])
    assert torch.isfinite(cached.float()).all()
    got2 = run()                                            # the next clip starts over: the same steps, the same latents
    assert model.step_cache_stats() == st2 and same_bits(got2, cached)
    fresh(model)
