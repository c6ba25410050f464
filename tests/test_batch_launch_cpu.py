"""CPU: the C ABI of the batch forms (include/bya.h: bya_attn_kv_mix_batch, bya_attn_kv_mix_mx_batch, bya_router_scores_batch,
bya_router_head_batch and their plan queries) -- the binding table against the header, every plan equal to the single-sample
plan with the grid multiplied by n, every refusal with its code before any launch and the plan left alone -- the ops front end
on meta tensors, the engine's switch, and the pipeline's self-heal re-run with the library calls stubbed."""
import ctypes
import os
import re

import pytest
import torch

OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
E4M3, E2M3 = 0, 2
BASE = 1 << 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bya_attn_kv_mix_batch", "bya_attn_kv_mix_mx_batch", "bya_router_scores_batch", "bya_router_head_batch")


@pytest.fixture(scope="module")
def lib():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    return _hip.load()


def header():
    return open(os.path.join(ROOT, "include", "bya.h")).read()


def test_binding_table_matches_the_header(lib):
    """The method of tests/test_abi_cpu.py: every int bya_*( of the header is bound and exported, and the by-value structs have the
    header's fields in the header's order and sizes."""
    from bind_your_avatar_implementation_amd import _hip
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(bya_\w+)\s*\(", src)))
    assert sorted(_hip.SIGNATURES) == declared
    for name in NEW:
        for entry in (name, name + "_plan"):
            assert entry in declared and hasattr(lib, entry), entry
            args = re.search(r"\bint\s+%s\s*\((.*?)\);" % entry, src, flags=re.S).group(1).split(",")
            assert len(_hip.SIGNATURES[entry]) == len(args), entry
    for cname, cls in (("bya_attn_mix_samples", _hip.AttnMixSamples), ("bya_attn_mix_mx_samples", _hip.AttnMixMxSamples),
                       ("bya_router_scores_samples", _hip.RouterScoresSamples), ("bya_router_head_samples", _hip.RouterHeadSamples)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            typ, first = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in first.split(",")]
        assert [f[0] for f in fields] == [f[0] for f in cls._fields_], cname
        for (n, typ), (_, ct) in zip(fields, cls._fields_):
            assert ctypes.sizeof(ct) == {"int32_t": 4, "int64_t": 8}[typ], (cname, n)
        assert ctypes.sizeof(cls) == 8 + 8 * (len(fields) - 2)
        by_value = [s for s in _hip.SIGNATURES.values() if cls in s]
        assert len(by_value) == 2                                     # the entry and its query take it BY VALUE


def desc(D=64, H=3, n_id=2, n_grp=4, Sq=500, Skv=32, mx=False):
    from bind_your_avatar_implementation_amd import _hip
    d = _hip.AttnMixDesc()
    d.head_dim, d.heads, d.n_id, d.n_grp, d.Sq, d.Skv = D, H, n_id, n_grp, Sq, Skv
    d.q_row = d.k_row = d.v_row = H * D
    d.q_grp = Sq * H * D
    d.z_row, d.z_grp = (0, 0) if mx else (H * D, Sq * H * D)
    d.k_grp = d.v_grp = Skv * H * D
    d.k_id = d.v_id = n_grp * Skv * H * D
    d.scale = D ** -0.5
    return d


def mx_strides(d, fmt):
    cb, sb = d.heads * d.head_dim * (8 if fmt == E4M3 else 6) // 8, d.heads * d.head_dim // 32
    return [d.Sq * cb, cb, d.Sq * sb, sb]


def samples(d, n, mx=False, fmt=E2M3, **over):
    """The strides of n samples stacked without a gap (r: rows * n_id, af: n_id^2, wsum: rows)."""
    from bind_your_avatar_implementation_amd import _hip
    rows, E = d.n_grp * d.Sq, d.heads * d.head_dim
    s = _hip.AttnMixMxSamples() if mx else _hip.AttnMixSamples()
    s.n, s.q, s.k, s.v, s.r, s.af, s.wsum = n, rows * E, d.n_id * d.k_id, d.n_id * d.v_id, rows * d.n_id, d.n_id ** 2, rows
    if mx:
        st = mx_strides(d, fmt)
        s.codes, s.scales = rows * st[1], rows * st[3]
    else:
        s.z = rows * E
    for k, v in over.items():
        setattr(s, k, v)
    return s


class Mix:
    """bya_attn_kv_mix[_mx]_batch or its query behind one signature; ``single`` asks the single-sample query."""

    def __init__(self, lib, mx, plan):
        self.lib, self.mx, self.plan = lib, mx, plan
        self.name = "bya_attn_kv_mix" + ("_mx" if mx else "") + "_batch" + ("_plan" if plan else "")

    def __call__(self, d, s, out=BASE, af=None, st=None, fmt=E2M3, q=BASE, wsum=None):
        from bind_your_avatar_implementation_amd import _hip
        self.filled = _hip.AttnMixPlan(-9, -9, -9, -9, -9, -9)
        dp = None if d is None else ctypes.byref(d)
        outs = (out, out) if self.mx else (out,)
        tail = (dp,) + ((fmt, *(st or (mx_strides(d, fmt) if d is not None else [0, 144, 0, 6]))) if self.mx else ())
        fn = getattr(self.lib, self.name)
        if self.plan:
            return fn(*outs, af, *tail, s, ctypes.byref(self.filled))
        return fn(q, BASE, BASE, BASE, af, *outs, wsum, *tail, s, None)

    def single(self, d, out=BASE, af=None, fmt=E2M3):
        from bind_your_avatar_implementation_amd import _hip
        p = _hip.AttnMixPlan()
        if self.mx:
            assert self.lib.bya_attn_kv_mix_mx_plan(out, out, af, ctypes.byref(d), fmt, *mx_strides(d, fmt), ctypes.byref(p)) == OK
        else:
            assert self.lib.bya_attn_kv_mix_plan(out, af, ctypes.byref(d), ctypes.byref(p)) == OK
        return p

    def untouched(self):
        p = self.filled
        return (p.form, p.head_dim, p.grid, p.row_chunks, p.lds_bytes, p.big_lds) == (-9,) * 6


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("mx", [False, True])
@pytest.mark.parametrize("D,H,n_id,n_grp,Sq", [(64, 3, 2, 4, 500), (64, 48, 3, 13, 1350), (128, 16, 2, 1, 17550), (128, 16, 4, 1, 33)])
def test_mix_batch_plan_is_the_single_plan_with_the_grid_times_n(lib, mx, n, D, H, n_id, n_grp, Sq):
    e = Mix(lib, mx, True)
    d = desc(D, H, n_id, n_grp, Sq, mx=mx)
    af = BASE if D == 64 else None
    assert e(d, samples(d, n, mx), af=af) == OK
    one, p = e.single(d, af=af), e.filled
    assert (p.form, p.head_dim, p.row_chunks, p.lds_bytes, p.big_lds) == (0, D, one.row_chunks, one.lds_bytes, one.big_lds)
    assert p.grid == one.grid * n and one.grid == one.row_chunks * H * n_grp
    assert one.big_lds == (D == 128 and n_id == 4)


@pytest.mark.parametrize("mx,plan", [(mx, plan) for mx in (False, True) for plan in (False, True)])
def test_every_mix_refusal_has_its_code_and_leaves_the_plan_alone(lib, mx, plan):
    from bind_your_avatar_implementation_amd import _hip
    e, query = Mix(lib, mx, plan), Mix(lib, mx, True)

    def refused(code, d, s, **kw):
        # (the addresses are made up: a launch entry is only ever called with what its query, the same checks, has refused)
        assert "q" in kw or "wsum" in kw or query(d, s, **kw) == code, (query.name, code, kw)
        assert e(d, s, **kw) == code, (e.name, code, kw)
        assert e.untouched()

    d = desc(mx=mx)
    rows, E = d.n_grp * d.Sq, d.heads * d.head_dim
    assert query(d, samples(d, 2, mx)) == OK                                       # the good call every refusal departs from
    # ---- n
    refused(ERR_SHAPE, d, samples(d, 0, mx))
    refused(ERR_SHAPE, d, samples(d, -2, mx))
    refused(ERR_SHAPE, d, samples(d, 65536, mx))
    # ---- negative strides
    for name in ("q", "k", "v", "r", "wsum"):
        refused(ERR_SHAPE, d, samples(d, 2, mx, **{name: -8}))
    refused(ERR_SHAPE, d, samples(d, 2, mx, af=-4), af=BASE)
    # ---- outputs that overlap (one element / byte short of what a sample covers); n = 1 has no neighbour to overlap
    out_names = ("codes", "scales") if mx else ("z",)
    for name in out_names:
        full = getattr(samples(d, 2, mx), name)
        short = full - (4 if name == "codes" else 8 if name == "z" else 1)
        refused(ERR_SHAPE, d, samples(d, 2, mx, **{name: short}))
        refused(ERR_SHAPE, d, samples(d, 3, mx, **{name: 0}))
        assert query(d, samples(d, 1, mx, **{name: 0})) == OK
        refused(ERR_SHAPE, d, samples(d, 2, mx, **{name: -full}))
    refused(ERR_SHAPE, d, samples(d, 2, mx, wsum=rows - 1))
    if not plan:
        refused(ERR_SHAPE, d, samples(d, 2, mx, wsum=rows - 1), wsum=BASE)
        assert query(d, samples(d, 2, mx, wsum=0)) == OK                           # no wsum: its stride is not looked at
    # ---- alignment
    for name in ("q", "k", "v"):
        refused(ERR_ALIGN, d, samples(d, 2, mx, **{name: getattr(samples(d, 2, mx), name) + 4}))
    if mx:
        refused(ERR_ALIGN, d, samples(d, 2, mx, codes=samples(d, 2, mx).codes + 2))
        assert query(d, samples(d, 2, mx, scales=samples(d, 2, mx).scales + 1)) == OK       # scale bytes need no alignment
    else:
        refused(ERR_ALIGN, d, samples(d, 2, z=rows * E + 2))
    assert query(d, samples(d, 2, mx, r=0)) == OK                                  # one r for the whole batch
    assert query(d, samples(d, 2, mx, r=rows * d.n_id + 1)) == OK                  # r is read element by element
    # ---- the generic form: BYA_ERR_UNSUPPORTED, as the segment form
    refused(ERR_UNSUPPORTED, desc(Skv=40, mx=mx), samples(desc(Skv=40, mx=mx), 2, mx))
    _hip.set_option("reference_forms", _hip.REFERENCE_FORMS["kv_mix_generic"])
    try:
        refused(ERR_UNSUPPORTED, d, samples(d, 2, mx))
    finally:
        _hip.set_option("reference_forms", 0)
    if not mx:
        refused(ERR_UNSUPPORTED, d, samples(d, 2), out=BASE + 8)                   # z not 16-byte aligned
        refused(ERR_UNSUPPORTED, d, samples(d, 2, z=rows * E + 4))                 # ... in the odd samples
    # ---- what the single-sample entry refuses
    refused(ERR_SHAPE, None, samples(d, 2, mx))
    refused(ERR_SHAPE, d, samples(d, 2, mx), out=None)
    refused(ERR_SHAPE, desc(Skv=65, mx=mx), samples(d, 2, mx))
    refused(ERR_SHAPE, desc(n_id=5, mx=mx), samples(d, 2, mx))
    refused(ERR_SHAPE, desc(n_id=1, mx=mx), samples(d, 2, mx), af=BASE)
    refused(ERR_UNSUPPORTED, desc(D=96, mx=mx), samples(d, 2, mx))
    dr = desc(mx=mx)
    dr.k_row = 196
    refused(ERR_ALIGN, dr, samples(d, 2, mx))
    if mx:
        st = mx_strides(d, E2M3)
        refused(ERR_SHAPE, d, samples(d, 2, mx), st=[st[0], st[1] - 4, st[2], st[3]])
        refused(ERR_ALIGN, d, samples(d, 2, mx), out=BASE + 2)
        refused(ERR_UNSUPPORTED, d, samples(d, 2, mx), fmt=4)
    else:
        refused(ERR_ALIGN, d, samples(d, 2), out=BASE + 4)
    if not plan:
        refused(ERR_SHAPE, d, samples(d, 2, mx), q=None)
        refused(ERR_ALIGN, d, samples(d, 2, mx), q=BASE + 8)
    assert query(d, samples(d, 2, mx)) == OK


def test_a_null_plan_is_refused(lib):
    from bind_your_avatar_implementation_amd import _hip
    d, dm = desc(), desc(mx=True)
    assert lib.bya_attn_kv_mix_batch_plan(BASE, None, ctypes.byref(d), samples(d, 2), None) == ERR_SHAPE
    assert lib.bya_attn_kv_mix_mx_batch_plan(BASE, BASE, None, ctypes.byref(dm), E2M3, *mx_strides(dm, E2M3), samples(dm, 2, True),
                                             None) == ERR_SHAPE
    b = _hip.RouterScoresSamples(2, 0, 8, 8, 1 << 30)
    assert lib.bya_router_scores_batch_plan(BASE, BASE, BASE, BASE, BASE, BASE, 2, 70, 16, 32, b, None) == ERR_SHAPE
    assert lib.bya_router_head_batch_plan(BASE, BASE, BASE, BASE, 2, 70, 512, _hip.RouterHeadSamples(2, 0, 8, 1 << 20), None) == ERR_SHAPE


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("n_id,N", [(2, 70), (3, 257), (2, 17550)])
def test_router_batch_plans_and_refusals(lib, n, n_id, N):
    from bind_your_avatar_implementation_amd import _hip
    F = lambda: _hip.StepPlan(-9, -9, -9, -9, -9, -9)
    tup = lambda p: (p.kernel, p.grid, p.rounds, p.items, p.items_per_round)
    # ---- scores
    one, p = F(), F()
    assert lib.bya_router_scores_plan(BASE, BASE, BASE, BASE, BASE, BASE, n_id, N, 16, 32, ctypes.byref(one)) == OK
    good = lambda **o: _hip.RouterScoresSamples(**dict(dict(n=n, qr=N * 2048, kr=n_id * 32 * 2048, out=n_id * N * 512), **o))
    q = lambda s, p, out=BASE, heads=16: lib.bya_router_scores_batch_plan(BASE, BASE, BASE, BASE, BASE, out, n_id, N, heads, 32, s,
                                                                         ctypes.byref(p))
    launch = lambda s, out=BASE, heads=16: lib.bya_router_scores_batch(BASE, BASE, BASE, BASE, BASE, out, n_id, N, heads, 32, 1e-5, s, None)
    assert q(good(), p) == OK
    assert tup(p) == (one.kernel, one.grid * n, one.rounds, one.items, one.items_per_round)
    assert one.kernel == (1 if N >= 4096 else 0)
    for code, s, kw in ((ERR_SHAPE, good(n=0), {}), (ERR_SHAPE, good(n=65536), {}), (ERR_SHAPE, good(qr=-8), {}),
                        (ERR_SHAPE, good(kr=-8), {}), (ERR_ALIGN, good(qr=N * 2048 + 4), {}), (ERR_ALIGN, good(kr=4), {}),
                        (ERR_ALIGN, good(out=n_id * N * 512 + 4), {}), (ERR_SHAPE, good(), dict(out=None)),
                        (ERR_ALIGN, good(), dict(out=BASE + 8)), (ERR_UNSUPPORTED, good(), dict(heads=8))):
        p = F()
        assert q(s, p, **kw) == code and launch(s, **kw) == code and tup(p) == (-9,) * 5, (code, kw)
    p = F()
    overlap = good(out=n_id * N * 512 - 8)
    assert q(overlap, p) == (ERR_SHAPE if n > 1 else OK)
    two = good(n=max(n, 2), out=n_id * N * 512 - 8)
    assert q(two, F()) == ERR_SHAPE and launch(two) == ERR_SHAPE
    assert q(good(qr=0, kr=0), F()) == OK                                          # shared inputs
    # ---- head
    goodh = lambda **o: _hip.RouterHeadSamples(**dict(dict(n=n, x=n_id * N * 512, r=N * n_id), **o))
    qh = lambda s, p, x=BASE, D=512: lib.bya_router_head_batch_plan(x, BASE, BASE, BASE, n_id, N, D, s, ctypes.byref(p))
    lh = lambda s, x=BASE, D=512: lib.bya_router_head_batch(x, BASE, BASE, BASE, n_id, N, D, s, None)
    p = F()
    assert qh(goodh(), p) == OK and tup(p) == (0, -(-N * n_id // 4) * n, 1, N * n_id, N * n_id)
    for code, s, kw in ((ERR_SHAPE, goodh(n=0), {}), (ERR_SHAPE, goodh(x=-8), {}), (ERR_SHAPE, goodh(r=-1), {}),
                        (ERR_ALIGN, goodh(x=n_id * N * 512 + 4), {}), (ERR_SHAPE, goodh(), dict(D=500)),
                        (ERR_SHAPE, goodh(), dict(x=None)), (ERR_ALIGN, goodh(), dict(x=BASE + 8))):
        p = F()
        assert qh(s, p, **kw) == code and lh(s, **kw) == code and tup(p) == (-9,) * 5, (code, kw)
    assert qh(goodh(r=N * n_id - 1), F()) == (ERR_SHAPE if n > 1 else OK)
    twoh = goodh(n=max(n, 2), r=N * n_id - 1)
    assert qh(twoh, F()) == ERR_SHAPE and lh(twoh) == ERR_SHAPE


def test_ops_front_end_on_meta_tensors(lib):
    from bind_your_avatar_implementation_amd import _hip, ops
    H, D, n = 3, 64, 2
    E = H * D
    meta = lambda *s, dt=torch.bfloat16: torch.empty(*s, dtype=dt, device="meta")
    kw = dict(head_dim=D, heads=H, n_id=2, n_grp=4, Sq=40, Skv=32, q_strides=(40 * E, E), k_strides=(4 * 32 * E, 32 * E, E),
              v_strides=(4 * 32 * E, 32 * E, E))
    z, af = meta(n, 160, E), meta(n, 2, 2)
    one = ops.attn_kv_mix_plan(z[0], af[0], z_strides=(40 * E, E), **kw)
    assert one["form"] == "mix32" and one["grid"] == 4 * H
    for m in (1, 2, 3):
        assert ops.attn_kv_mix_batch_plan(meta(m, 160, E), meta(m, 2, 2), n=m, z_strides=(40 * E, E), **kw) == dict(one, grid=one["grid"] * m)
    # declined: None, not an error; a malformed batch is an error
    assert ops.attn_kv_mix_batch_plan(z, af, n=n, z_strides=(40 * E, E), **dict(kw, Skv=40)) is None
    with pytest.raises(_hip.ByaError, match="BYA_ERR_SHAPE"):
        ops.attn_kv_mix_batch_plan(z[:1].expand(3, 160, E), None, n=3, z_strides=(40 * E, E), **kw)          # three samples in one place
    with pytest.raises(ValueError, match="first dimension"):
        ops.attn_kv_mix_batch_plan(z, af, n=3, z_strides=(40 * E, E), **kw)
    c, s = meta(n, 160, E * 6 // 8, dt=torch.uint8), meta(n, 160, E // 32, dt=torch.uint8)
    pm = ops.attn_kv_mix_batch_plan(None, af, n=n, mx_out=(c, s, "mxfp6"), **kw)
    assert pm == dict(one, grid=one["grid"] * n, mx_out="mxfp6")
    # the router
    qr, kr, w, pos, out = meta(n, 70, 2048), meta(n, 2, 32, 2048), meta(512), meta(70, 512), meta(n, 2, 70, 512)
    one = ops.router_scores_plan(qr[0], kr[0], w, w, pos, out[0], 2, 70)
    assert ops.router_scores_batch_plan(qr, kr, w, w, pos, out, 2, 70) == dict(one, grid=one["grid"] * n)
    assert ops.router_head_batch_plan(out, w, w[:1], meta(n, 70, 2), 2, 70) == {"kernel": "rows", "grid": 35 * n, "rounds": 1, "items": 140,
                                                                              "items_per_round": 140}
    # a launch never takes meta tensors
    with pytest.raises((ValueError, AssertionError)):
        ops.attn_kv_mix_batch(z, z, z, meta(n, 160, 2), af, z, z_strides=(40 * E, E), scale=0.125, **kw)
    with pytest.raises((ValueError, AssertionError)):
        ops.router_head_batch(out, w, w[:1], meta(n, 70, 2), 2, 70)


def test_the_model_switch_is_off_by_default():
    """(that the engine reads it and BYA_BATCH_LAUNCHES when it is built: tests/test_batch_engine_gpu.py -- an engine needs a GPU)"""
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    with torch.device("meta"):
        m = BindyouravatarTransformer3DModel(num_layers=1, in_channels=48, use_rotary_positional_embeddings=True)
    assert m.batch_launches is False and m.use_hip_graph is False and m._graphs == {}


# ------------------------------------------------------------------------------------------ self-heal under graph replay
class _Tr:
    def __init__(self):
        self._graphs = {"captured": object()}


def _steps(tr, seen):
    def predict():
        seen.append(dict(tr._graphs))
        return len(seen)
    return predict


def test_self_heal_drops_the_graphs_before_the_rerun_and_checks_it(monkeypatch):
    from bind_your_avatar_implementation_amd import _hip, ops, pipeline
    # a healthy step: one predict, one query, the graphs stay
    tr, seen, answers = _Tr(), [], [False]
    monkeypatch.setattr(ops, "heal_handoffs", lambda device=None: answers.pop(0))
    assert pipeline._self_healing_step(tr, "cuda:0", _steps(tr, seen)) == 1
    assert len(seen) == 1 and "captured" in tr._graphs and answers == []
    # a time-out: the graphs are gone BEFORE the re-run, whose result is returned after a second, clean query
    tr, seen, answers = _Tr(), [], [True, False]
    assert pipeline._self_healing_step(tr, "cuda:0", _steps(tr, seen)) == 2
    assert [("captured" in g) for g in seen] == [True, False] and tr._graphs == {} and answers == []
    # a time-out behind the re-run as well: nothing to stand on, the clip fails
    tr, seen, answers = _Tr(), [], [True, True]
    with pytest.raises(_hip.ByaError, match="timed out again"):
        pipeline._self_healing_step(tr, "cuda:0", _steps(tr, seen))
    assert len(seen) == 2 and answers == []


def test_the_denoising_loop_heals_through_the_checked_rerun(monkeypatch):
    """pipeline.__call__ on a stand-in transformer that says it lives on a GPU: a time-out behind the first step drops the graphs
    and repeats that step; a time-out behind the repeat fails the clip."""
    from types import SimpleNamespace
    from bind_your_avatar_implementation_amd import _hip, ops, pipeline

    class Tr:
        dtype = torch.float32
        config = SimpleNamespace(in_channels=48, patch_size=2, attention_head_dim=64, use_rotary_positional_embeddings=False)

        def __init__(self):
            self._graphs, self.graphs_seen = {"captured": object()}, []

        @property
        def device(self):                   # tensors stay on the CPU (.to(cpu)); only the heal switch sees "cuda"
            return FakeDev()

        def precompute_conditioning(self, *a):
            pass

        def release_conditioning(self):
            pass

        def __call__(self, hidden_states, encoder_hidden_states, **kw):
            self.graphs_seen.append(dict(self._graphs))
            return (torch.ones_like(hidden_states[:, :, :16]),)

    class Sch:
        def set_timesteps(self, n, dev):
            return torch.arange(n - 1, -1, -1)

        def scale_model_input(self, x, t):
            return x

        def step(self, n32, t, latents, return_dict=False):
            return (latents - 0.5 * n32,)

    class FakeDev:
        type = "cuda"

    real_device = torch.device
    monkeypatch.setattr(pipeline.torch, "device", lambda d=None, *a: d if isinstance(d, FakeDev) else real_device(d, *a))
    to = torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: to(self, *[x for x in a if not isinstance(x, FakeDev)], **k))
    monkeypatch.delenv("BYA_SELF_HEAL", raising=False)

    def run(answers):
        tr = Tr()
        monkeypatch.setattr(ops, "heal_handoffs", lambda device=None: answers.pop(0))
        monkeypatch.setattr(ops, "check_gemm_workspace", lambda device=None: None)       # the end-of-clip check: a library call too
        lat = torch.zeros(1, 3, 16, 4, 6)
        pipe = pipeline.BindyouravatarPipeline(tr, scheduler=Sch())
        pipe(height=32, width=48, num_frames=9, num_inference_steps=2, guidance_scale=1.0, latents=lat,
             prompt_embeds=torch.ones(1, 4, 8), image_latents=torch.zeros(1, 3, 16, 4, 6),
             image_bg_latents=torch.zeros(1, 3, 16, 4, 6), output_type="latent")
        return tr
    tr = run([False, False])
    assert len(tr.graphs_seen) == 2 and "captured" in tr._graphs
    tr = run([True, False, False])
    assert [("captured" in g) for g in tr.graphs_seen] == [True, False, False] and tr._graphs == {}
    with pytest.raises(_hip.ByaError, match="timed out again"):
        run([True, True])
