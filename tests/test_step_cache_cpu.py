"""CPU: the host side of the first-block step cache (include/bya.h "First-block step cache") -- the policy against its torch
restatement, the arguments of ``enable_step_cache``, the pipeline's resets (per clip, and before a healed re-run) on a
stand-in transformer that records its calls, the refusals, and the plan query of the kernels (host-side, launches nothing)."""
import ctypes
import itertools
import math
from types import SimpleNamespace

import pytest
import torch

import step_cache_ref as ref


def test_the_policy_agrees_with_the_restatement_over_a_grid():
    from bind_your_avatar_implementation_amd.engine import step_cache_decide, step_cache_distance
    values = [0.0, 1e-300, 0.5, 1.0, 3.0, 1e300, math.inf, math.nan]
    thresholds = [0.0, 1e-6, 0.5, 1.0, 10.0, math.inf]
    n = 0
    for num, den, has_ref, hits, thr, cap in itertools.product(values, values, (False, True), (0, 1, 2, 5), thresholds, (None, 0, 1, 2, 6)):
        want = ref.decide(num, den, has_ref, hits, thr, cap)
        assert step_cache_decide(num, den, has_ref, hits, thr, cap) is want, (num, den, has_ref, hits, thr, cap)
        d, dr = step_cache_distance(num, den), ref.distance(num, den)
        assert d == dr or (math.isnan(d) and math.isnan(dr)), (num, den)
        n += 1
    assert n > 10000
    # the named corners, spelled out
    assert step_cache_decide(0.0, 1.0, False, 0, math.inf, None) is False          # no reference
    assert step_cache_distance(1.0, 0.0) == math.inf and step_cache_distance(0.0, 0.0) == math.inf
    assert step_cache_decide(0.0, 0.0, True, 0, math.inf, None) is False           # den = 0: d = inf, never below a threshold
    assert step_cache_decide(math.nan, 1.0, True, 0, math.inf, None) is False      # NaN compares false
    assert step_cache_decide(1.0, math.nan, True, 0, math.inf, None) is False
    assert step_cache_decide(0.0, 1.0, True, 0, 0.0, None) is False                # threshold 0 never re-uses
    assert step_cache_decide(0.0, 1.0, True, 0, 1e-9, None) is True
    assert step_cache_decide(0.0, 1.0, True, 2, math.inf, 2) is False and step_cache_decide(0.0, 1.0, True, 1, math.inf, 2) is True
    assert ref.pattern(6, 2) == "FRRFRR" and ref.pattern(4, None) == "FRRR" and ref.pattern(3, 0) == "FFF"


def _meta_model():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    with torch.device("meta"):
        return BindyouravatarTransformer3DModel(num_layers=1, in_channels=48, use_rotary_positional_embeddings=True)


def test_enable_step_cache_validates_its_arguments():
    m = _meta_model()
    assert m._step_cache is None and m.step_cache_stats() is None               # off by default
    assert m.reset_step_cache() is m                                             # a no-op while off
    with pytest.raises(TypeError):
        m.enable_step_cache()                                                    # the threshold has no default
    for bad in ("0.1", None, True, [0.1]):
        with pytest.raises(TypeError):
            m.enable_step_cache(bad)
    for bad in (-1e-9, -1, math.nan):
        with pytest.raises(ValueError):
            m.enable_step_cache(bad)
    with pytest.raises(TypeError):
        m.enable_step_cache(0.1, 3)                                              # max_consecutive_hits is keyword only
    for bad in (1.5, "2", True):
        with pytest.raises(TypeError):
            m.enable_step_cache(0.1, max_consecutive_hits=bad)
    with pytest.raises(ValueError):
        m.enable_step_cache(0.1, max_consecutive_hits=-1)
    with pytest.raises(TypeError):
        m.enable_step_cache(0.1, enabled=1)
    assert m._step_cache is None                                                 # a refused call changes nothing
    assert m.enable_step_cache(0.25, max_consecutive_hits=3) is m
    sc = m._step_cache
    assert (sc.threshold, sc.max_hits, sc.enabled, sc.has_ref, sc.hits) == (0.25, 3, True, False, 0)
    assert m.step_cache_stats() == {"steps": 0, "full": 0, "reused": 0, "distances": []}
    assert m.enable_step_cache(math.inf)._step_cache.threshold == math.inf and m.enable_step_cache(0)._step_cache.threshold == 0.0
    assert m.enable_step_cache(0.5, enabled=False)._step_cache is None


def test_the_state_counts_steps_and_drops_its_reference():
    from bind_your_avatar_implementation_amd.engine import StepCache
    sc = StepCache(0.5, 2)
    sc.has_ref, sc.hits = True, 1
    sc.count(False, math.inf)
    sc.count(True, 0.25)
    assert sc.stats() == {"steps": 2, "full": 1, "reused": 1, "distances": [math.inf, 0.25]}
    sc.uncount_last()                                                            # the step is run again: counted once
    sc.uncount_last()                                                            # (only the last one can be taken back)
    assert sc.stats() == {"steps": 1, "full": 1, "reused": 0, "distances": [math.inf]}
    sc.drop()
    assert (sc.has_ref, sc.hits, sc.E, sc.cond_key) == (False, 0, None, None) and sc.steps == 1
    sc.reset()
    assert sc.stats() == {"steps": 0, "full": 0, "reused": 0, "distances": []}
    # invalidate_engine() drops the reference and keeps the counters
    m = _meta_model().enable_step_cache(1.0)
    m._step_cache.has_ref = True
    m._step_cache.count(False, math.inf)
    m.invalidate_engine()
    assert m._step_cache.has_ref is False and m.step_cache_stats()["steps"] == 1


class _Tr:
    """A stand-in transformer that records what the pipeline calls on it."""
    device, dtype = torch.device("cpu"), torch.float32
    config = SimpleNamespace(in_channels=48, patch_size=2, attention_head_dim=64, use_rotary_positional_embeddings=False)

    def __init__(self):
        self.calls, self._graphs = [], {}

    def precompute_conditioning(self, *a):
        self.calls.append("precompute")

    def release_conditioning(self):
        self.calls.append("release")

    def reset_step_cache(self, uncount_last=False):
        self.calls.append("reset(uncount_last)" if uncount_last else "reset")

    def __call__(self, hidden_states, encoder_hidden_states, **kw):
        self.calls.append("step")
        return (torch.ones_like(hidden_states[:, :, :16]),)


class _Sch:
    def set_timesteps(self, n, dev):
        return torch.arange(n - 1, -1, -1, device=dev)

    def scale_model_input(self, x, t):
        return x

    def step(self, n32, t, latents, return_dict=False):
        return (latents - 0.5 * n32,)


def _clip(pipe, steps):
    lat = torch.zeros(1, 3, 16, 4, 6)
    return pipe(height=32, width=48, num_frames=9, num_inference_steps=steps, guidance_scale=1.0, latents=lat,
                prompt_embeds=torch.ones(1, 4, 8), image_latents=lat.clone(), image_bg_latents=lat.clone(), output_type="latent")


def test_the_pipeline_resets_the_cache_per_clip():
    from bind_your_avatar_implementation_amd.pipeline import BindyouravatarPipeline
    tr = _Tr()
    pipe = BindyouravatarPipeline(tr, scheduler=_Sch())
    _clip(pipe, 3)
    _clip(pipe, 2)
    assert tr.calls == ["precompute", "reset", "step", "step", "step", "release", "precompute", "reset", "step", "step", "release"]


def test_the_pipeline_resets_the_cache_before_a_healed_rerun(monkeypatch):
    from bind_your_avatar_implementation_amd import ops, pipeline
    tr, answers = _Tr(), [False, True, False]
    monkeypatch.setattr(ops, "heal_handoffs", lambda device=None: answers.pop(0))
    predict = lambda: tr(torch.zeros(1, 1, 16), None)
    pipeline._self_healing_step(tr, "cuda:0", predict)                           # a healthy step: no reset
    assert tr.calls == ["step"]
    pipeline._self_healing_step(tr, "cuda:0", predict)                           # a time-out: reset, then the re-run
    assert tr.calls == ["step", "step", "reset(uncount_last)", "step"] and answers == []
    # ... and on the real model the re-run's reset forgets the reference and takes the step out of the counters
    m = _meta_model().enable_step_cache(1.0)
    sc = m._step_cache
    sc.count(False, math.inf)
    sc.count(True, 0.5)
    sc.has_ref, sc.hits = True, 1
    m.reset_step_cache(uncount_last=True)
    assert (sc.has_ref, sc.hits) == (False, 0) and m.step_cache_stats() == {"steps": 1, "full": 1, "reused": 0, "distances": [math.inf]}
    m.reset_step_cache()
    assert m.step_cache_stats()["steps"] == 0


def test_sharded_steps_and_the_cfg_rank_split_are_refused():
    from bind_your_avatar_implementation_amd.engine import DenoiseEngine, StepCache, step_cache_refusal
    assert step_cache_refusal(SimpleNamespace()) is None
    assert "sequence-parallel" in step_cache_refusal(SimpleNamespace(_seq_world=2, _seq_group=object()))
    assert "sequence-parallel" in step_cache_refusal(SimpleNamespace(_seq_world=1, _seq_group=object()))
    assert "CFG rank split" in step_cache_refusal(SimpleNamespace(_cfg=object()))
    # the step itself refuses before it touches a tensor (an engine cannot be built without a GPU: a bare one will do here)
    for attrs, word in ((dict(_cfg=object()), "CFG rank split"), (dict(_seq_world=4, _seq_group=object()), "sequence-parallel")):
        eng = DenoiseEngine.__new__(DenoiseEngine)
        eng.m = SimpleNamespace(_step_cache=StepCache(0.5), **attrs)
        with pytest.raises(NotImplementedError, match=word):
            eng._step(None, None, None, None, None, None, None, None, None)
        eng.m._step_cache.enabled = False                                       # cache off: the step goes on (and trips on the None)
        with pytest.raises((AttributeError, TypeError)):
            eng._step(None, None, None, None, None, None, None, None, None)


def test_graph_replay_is_bypassed_while_the_cache_is_enabled(monkeypatch):
    """use_hip_graph with the cache on: forward takes the eager path (the host decides mid-step); off again, the graphed one."""
    m = _meta_model()
    m.is_train_face = False
    taken = []
    m._engine = SimpleNamespace(step=lambda *a: taken.append("eager") or "out")
    monkeypatch.setattr(m, "_graphed_step", lambda args: taken.append("graph") or "out")
    m.use_hip_graph = True
    t = torch.zeros(1, dtype=torch.int64)
    m.forward(None, None, t)
    m.enable_step_cache(0.0)
    m._engine = SimpleNamespace(step=lambda *a: taken.append("eager") or "out")   # (enable_step_cache keeps the engine: set again anyway)
    m.forward(None, None, t)
    m.enable_step_cache(0.0, enabled=False)
    m.forward(None, None, t)
    assert taken == ["graph", "eager", "graph"]


def test_the_plan_query_validates_like_the_entry_points():
    from bind_your_avatar_implementation_amd import _hip, ops
    lib = _hip.load()
    base = 1 << 40
    sp = _hip.StepCachePlan(-9)
    q = lambda x, E, rr, rn, n, plan: lib.bya_step_cache_probe_plan(x, E, rr, rn, n, plan)
    assert q(None, base, base, base, 64, ctypes.byref(sp)) == -1 and q(base, base, base, None, 64, ctypes.byref(sp)) == -1
    assert q(base, base, base, base, 64, None) == -1
    assert q(base, base, base, base, 0, ctypes.byref(sp)) == -1 and q(base, base, base, base, 68, ctypes.byref(sp)) == -1
    for k in range(4):                                                           # every operand: 16 bytes
        ptrs = [base] * 4
        ptrs[k] += 8
        assert q(*ptrs, 64, ctypes.byref(sp)) == -2
    assert sp.grid == -9                                                         # untouched on rejection
    assert q(base, base, None, base, 8, ctypes.byref(sp)) == 0                   # no reference yet: r_ref may be NULL
    assert (sp.grid, sp.vec, sp.wg_pass_elems, sp.passes, sp.partials_bytes) == (1, 8, 2048, 1, 16)
    n = 2 * 17776 * 3072                                                         # the headline stream, both halves of the pair
    assert q(base, base, base, base, n, ctypes.byref(sp)) == 0
    assert (sp.grid, sp.passes, sp.partials_bytes) == (2048, -(-n // (2048 * 2048)), 32768)
    # the launchers refuse the same arguments with nothing launched (no GPU here: a launch would fail otherwise)
    assert lib.bya_step_cache_probe(base, base, base, base, base, base, 68, None) == -1
    assert lib.bya_step_cache_probe(base, base, base, base, None, base, 64, None) == -1
    assert lib.bya_step_cache_probe(base, base + 2, base, base, base, base, 64, None) == -2
    assert lib.bya_step_cache_probe(base, base, base, base, base + 4, base, 64, None) == -2
    assert lib.bya_step_cache_capture(base, base, base, 12, None) == -1 and lib.bya_step_cache_capture(base, base, base + 6, 16, None) == -2
    assert lib.bya_step_cache_capture(base, None, base, 16, None) == -1
    assert lib.bya_step_cache_apply(base, base, 7, None) == -1 and lib.bya_step_cache_apply(base + 8, base, 16, None) == -2
    assert lib.bya_step_cache_apply(None, base, 16, None) == -1
    # ops: meta tensors stand for device tensors in the query, never in a launch
    meta = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device="meta")
    x = meta(1, 514, 3072)
    assert ops.step_cache_probe_plan(x, meta(1, 514, 3072), None, meta(1, 514, 3072)) == {
        "grid": 771, "vec": 8, "wg_pass_elems": 2048, "passes": 1, "partials_bytes": 771 * 16}
    with pytest.raises(ValueError):
        ops.step_cache_probe_plan(x, meta(1, 514, 3064), None, meta(1, 514, 3072))
    with pytest.raises(ValueError):
        ops.step_cache_apply(x, meta(1, 514, 3072))
