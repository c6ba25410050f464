"""The guided step ([uncond, cond], B = 2) of the tests' 2-layer model with the two opt-in switches of the product path:
``batch_launches`` -- the four per-sample launches of the face / audio routing become one launch per layer, the output unchanged
bit for bit -- and graph replay on a precomputed conditioning -- the captured graph reads the cached tensors in place and holds no
conditioning launch."""
import ctypes

import pytest
import torch

from test_forward_gpu import SMALL_KW, to_dev

pytestmark = pytest.mark.gpu

FACE_LAYERS = -(-SMALL_KW["num_layers"] // SMALL_KW["cross_attn_interval"])        # 1
AUDIO_LAYERS = -(-SMALL_KW["num_layers"] // SMALL_KW["audio_attn_interval"])       # 2
B = 2


@pytest.fixture(scope="module")
def model(dev):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    return BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)


def cfg_inputs(dev, seed, t=None):
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    inp = to_dev(synth_inputs(batch=B, frames=3, height=16, width=24, seed=seed, uncond_first=True), dev)
    if t is not None:
        inp["timestep"] = torch.tensor([t, t], dtype=torch.int64, device=dev)
    return inp


def counted_step(model, inp):
    """One eager step under the kernel timers -> (output, {label: launches})."""
    from bind_your_avatar_implementation_amd import ops
    ops.enable_kernel_timers()
    try:
        out = model(**inp)[0].clone()
    finally:
        times = ops.collect_kernel_timers()
    return out, {k: len(v) for k, v in times.items()}


def family(counts, name):
    """Launches of an entry point and of its _mx / _batch / _mx_batch forms, by form."""
    return {k: v for k, v in counts.items() if k in (name, name + "_mx", name + "_batch", name + "_mx_batch")}


@pytest.mark.parametrize("weights", ["bf16", "mx"])
def test_one_launch_per_layer_and_the_same_bits(model, dev, weights):
    mx = weights == "mx"
    if mx:
        model.enable_mx_weights("mxfp8", linears=("qkv", "out", "ff1", "ff2", "po", "ao"))
    try:
        inp = cfg_inputs(dev, 31)
        got = {}
        for on in (False, True):
            model.batch_launches = on
            model.invalidate_engine()
            got[on] = counted_step(model, inp)
            assert model._engine.batch_launches is on
    finally:
        model.batch_launches = False
        if mx:
            model.enable_mx_weights(enabled=False)
        model.invalidate_engine()
    assert torch.equal(got[True][0], got[False][0])
    sfx = "_mx" if mx else ""
    off, on = (family(got[sw][1], "bya_attn_kv_mix") for sw in (False, True))
    print("kv-mix launches, switch off / on:", off, on)
    assert off == {"bya_attn_kv_mix" + sfx: B * (FACE_LAYERS + AUDIO_LAYERS)}
    assert on == {"bya_attn_kv_mix" + sfx + "_batch": FACE_LAYERS + AUDIO_LAYERS}
    for name in ("bya_router_scores", "bya_router_head"):
        assert family(got[False][1], name) == {name: B * FACE_LAYERS}, name
        assert family(got[True][1], name) == {name + "_batch": FACE_LAYERS}, name
    # nothing else changed: the other labels and their counts are the same
    rest = lambda c: {k: v for k, v in c.items() if not k.startswith(("bya_attn_kv_mix", "bya_router_scores", "bya_router_head"))}
    assert rest(got[True][1]) == rest(got[False][1])


def test_the_switch_is_read_when_the_engine_is_built(model, dev, monkeypatch):
    """Off by default; on by the model's attribute or by BYA_BATCH_LAUNCHES=1, like its neighbours read at engine build."""
    from bind_your_avatar_implementation_amd.engine import DenoiseEngine
    assert model.batch_launches is False
    monkeypatch.delenv("BYA_BATCH_LAUNCHES", raising=False)
    assert DenoiseEngine(model).batch_launches is False
    monkeypatch.setenv("BYA_BATCH_LAUNCHES", "1")
    assert DenoiseEngine(model).batch_launches is True
    monkeypatch.setenv("BYA_BATCH_LAUNCHES", "0")
    assert DenoiseEngine(model).batch_launches is False
    monkeypatch.setattr(model, "batch_launches", True)
    assert DenoiseEngine(model).batch_launches is True


def test_a_shared_forcing_tensor_is_a_stride_of_zero(model, dev):
    """routing_logits_forcing: one sample of routing weights for the whole batch (r_logits.shape[0] == 1)."""
    inp = cfg_inputs(dev, 33)
    g = torch.Generator().manual_seed(3)
    inp["routing_logits_forcing"] = (torch.rand(3, 8 * 12, 2, generator=g) > 0.5).to(torch.bfloat16).to(dev)
    got = {}
    try:
        for on in (False, True):
            model.batch_launches = on
            model.invalidate_engine()
            got[on] = counted_step(model, inp)
    finally:
        model.batch_launches = False
        model.invalidate_engine()
    assert torch.equal(got[True][0], got[False][0])
    assert family(got[True][1], "bya_attn_kv_mix") == {"bya_attn_kv_mix_batch": FACE_LAYERS + AUDIO_LAYERS}


# ------------------------------------------------------------------------------------------ graph replay on the cache
def graph_nodes(graph):
    """Nodes of a captured graph (hipGraphGetNodes on the graph torch kept: ``kept_graphs``)."""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_size_t(0)
    rc = hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n))
    assert rc == 0, rc
    return n.value


@pytest.fixture
def kept_graphs(monkeypatch):
    """torch.cuda.CUDAGraph() keeps the captured graph beside its executable, so that its nodes can be counted."""
    orig = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: orig(keep_graph=True))


def test_graph_replay_reads_the_precomputed_conditioning(model, dev, kept_graphs):
    cond = cfg_inputs(dev, 41)
    ident = dict(id_cond=cond["id_cond"], id_vit_hidden=cond["id_vit_hidden"], audio_embeds=cond["audio_embeds"])

    def step_inputs(seed, t):                                    # new latents / text / timestep, the SAME conditioning tensors
        return dict(cfg_inputs(dev, seed, t), **ident)
    model.use_hip_graph = False
    model.invalidate_engine()
    try:
        # eager launch counts, cache off and on: the difference is the conditioning (extractor, projector, per-layer K / V)
        _, uncached = counted_step(model, step_inputs(50, 500))
        model.precompute_conditioning(ident["id_cond"], ident["id_vit_hidden"], ident["audio_embeds"], latent_frames=3)
        gen = model._engine._cache_generation
        want = {s: counted_step(model, step_inputs(s, 10 * s)) for s in (51, 52, 53)}
        cached = want[51][1]
        conditioning = sum(uncached.values()) - sum(cached.values())
        print("eager launches, cache off / on:", sum(uncached.values()), sum(cached.values()))
        assert conditioning > 0 and all(cached.get(k, 0) <= v for k, v in uncached.items())
        cache_before = {k: (v[0], [t.data_ptr() for t in BindTensors(v[2])]) for k, v in model._engine._inv_cache.items()}
        # three replayed steps on the cache: equal to eager, one graph, keyed by the cache's identity
        model.use_hip_graph = True
        for s in (51, 52, 53):
            assert torch.equal(model(**step_inputs(s, 10 * s))[0], want[s][0]), s
        assert len(model._graphs) == 1
        (key, entry), = model._graphs.items()
        assert key[1] is not None and key[1][0] == gen and entry.cache_hold is not None
        on_cache = graph_nodes(entry.graph)
        # the engine's cache was read, never written
        assert model._engine.cache_invariants and model._engine._cache_generation == gen
        assert cache_before == {k: (v[0], [t.data_ptr() for t in BindTensors(v[2])]) for k, v in model._engine._inv_cache.items()}
        # other identity tensors (equal values, other storage): not this graph -- no cache serves them, they are recomputed
        other = dict(step_inputs(52, 520), id_cond=[t.clone() for t in ident["id_cond"]])
        assert torch.equal(model(**other)[0], want[52][0])
        assert len(model._graphs) == 2
        (entry_off,) = [e for k, e in model._graphs.items() if k[1] is None]
        assert entry_off.cache_hold is None
        recomputing = graph_nodes(entry_off.graph)
        print("graph nodes, on the cache / recomputing:", on_cache, recomputing)
        # every conditioning launch of the library is missing from the graph on the cache (and so are torch's own kernels of
        # the conditioning, which the library's timers do not count: hence >=)
        assert recomputing - on_cache >= conditioning
        # the graph on the cache holds the cached eager step's launches plus the exchange-free constant -- on one GPU that is 0:
        # the copies into the graph's inputs and of its output run outside the graph, bf16 inputs need no cast, and with every
        # cache lookup a hit nothing but the library's launches is captured -- and not the uncached step's
        assert on_cache == sum(cached.values()) + 0 and on_cache < sum(uncached.values())
        # release: the graph on the cache goes with it, the next call recomputes the conditioning and still equals eager
        model.release_conditioning()
        assert [k[1] for k in model._graphs] == [None] and model._engine._cache_generation == gen + 1
        assert torch.equal(model(**step_inputs(53, 530))[0], want[53][0])
        assert len(model._graphs) == 1
    finally:
        model.use_hip_graph = False
        model.release_conditioning()
        model.invalidate_engine()


def BindTensors(val):
    """The tensors of a cache value (nested lists / tuples), flattened."""
    if torch.is_tensor(val):
        return [val]
    return [t for v in val for t in BindTensors(v)] if isinstance(val, (list, tuple)) else []
