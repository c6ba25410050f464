"""The engine's switch ``qkn_stats_epilogue`` (BYA_QKN_STATS_EPILOGUE=1, off by default): on a layer whose attention takes the
data-dependent score bound, the fused q|k|v launch records the q/k statistics itself instead of leaving the layer to the
projection + bya_qknorm_rope.  Modelled on test_large_qk_gains_keep_the_fast_attention_kernel (tests/test_forward_gpu.py):
SMALL_KW, 3 frames of 16 x 24, layer 1's q/k gains raised in place.  The step with the switch on equals the step with it off
bit for bit -- prediction, fallback flags, the table's maximum over its slots -- and issues one fused launch per block; and the
head-parallel sharded step (2 ranks on the one GPU, P2P, tables of 64 // W slots) with the switch on equals the unsharded step."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

WORKER_SECONDS = 420        # per spawned pair; a healthy run takes a fraction of it


class Fused:
    """Wraps ops.gemm_qkv_norm_rope: (took the launch, was given a table) per call."""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *a, **kw):
        took = self.fn(*a, **kw)
        self.calls.append((bool(took), kw.get("stats") is not None))
        return took


class Counter:
    def __init__(self, fn):
        self.fn, self.n, self.with_stats = fn, 0, 0

    def __call__(self, *a, **kw):
        self.n += 1
        self.with_stats += kw.get("stats") is not None
        return self.fn(*a, **kw)


def raise_layer1_gains(model):
    with torch.no_grad():
        model.transformer_blocks[1].attn1.norm_q.weight.mul_(2.0)
        model.transformer_blocks[1].attn1.norm_k.weight[::16].mul_(5.0)


def recorded_forward(model, gi, monkeypatch, switch):
    """One step under BYA_QKN_STATS_EPILOGUE = ``switch`` on a fresh engine, with the fused q|k|v launches recorded and the
    stand-alone q/k-norm launches counted -> (prediction, fused calls, qknorm_rope counter, flags, table maxima)."""
    from bind_your_avatar_implementation_amd import ops
    os.environ["BYA_QKN_STATS_EPILOGUE"] = switch
    try:
        model.invalidate_engine()
        model(**gi)                                                                       # builds the engine (packs weights)
    finally:
        del os.environ["BYA_QKN_STATS_EPILOGUE"]
    eng = model._engine
    assert eng.qkn_stats_epilogue is (switch == "1")
    with monkeypatch.context() as mp:
        f, n = Fused(ops.gemm_qkv_norm_rope), Counter(ops.qknorm_rope)
        mp.setattr(ops, "gemm_qkv_norm_rope", f)
        mp.setattr(ops, "qknorm_rope", n)
        ops.ATTN_VARIANTS.clear()
        out = model(**gi)[0].clone()
        variants = dict(ops.ATTN_VARIANTS)
    table = next(v for k, v in eng._ws.items() if isinstance(k, tuple) and k[0] == "qk_stats")
    return out, f.calls, n, eng._ws["qk_flags"].clone(), table.amax(0).clone(), variants


def test_switch_on_equals_switch_off_with_one_fused_launch_per_block(dev, monkeypatch):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import SMALL_KW, to_dev
    model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=4, fast=True)
    gi = to_dev(synth_inputs(batch=1, frames=3, height=16, width=24, seed=6), dev)
    blocks = len(model.transformer_blocks)
    model(**gi)
    assert model._engine.qkn_stats_epilogue is False                                      # the default
    raise_layer1_gains(model)
    off, f_off, n_off, flags_off, tab_off, var_off = recorded_forward(model, gi, monkeypatch, "0")
    bound = model._engine.score_bound
    assert bound[1] > ops.ATTN_BOUND_LIMIT and all(b <= ops.ATTN_BOUND_LIMIT for i, b in enumerate(bound) if i != 1)
    on, f_on, n_on, flags_on, tab_on, var_on = recorded_forward(model, gi, monkeypatch, "1")
    print(f"{blocks} blocks; switch off: fused {f_off}, qknorm_rope {n_off.n} ({n_off.with_stats} with a table); "
          f"switch on: fused {f_on}, qknorm_rope {n_on.n}; attention variants {var_on}")
    # switch off: every layer but layer 1 is one fused launch; layer 1 issues the projection + qknorm_rope with the table
    assert f_off == [(True, False)] * (blocks - 1) and (n_off.n, n_off.with_stats) == (1, 1)
    # switch on: one fused launch per block, layer 1's with the table, and no stand-alone q/k-norm launch
    assert [took for took, _ in f_on] == [True] * blocks and [st for _, st in f_on] == [i == 1 for i in range(blocks)]
    assert n_on.n == 0
    assert torch.equal(on, off)
    assert torch.equal(flags_on, flags_off)
    assert torch.equal(tab_on.view(torch.int32), tab_off.view(torch.int32)) and bool((tab_on > 0).all())
    assert var_on == var_off and var_on.get(("joint", "d64_device_bound_w4")) == 1


def _sp_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["BYA_QKN_STATS_EPILOGUE"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # 2 ranks share the single test GPU
    try:
        from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
        from bind_your_avatar_implementation_amd.parallel import shard_sequence
        from bind_your_avatar_implementation_amd.synth import synth_inputs
        from test_forward_gpu import SMALL_KW, to_dev
        dev = torch.device("cuda:0")
        model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
        raise_layer1_gains(model)
        inp = to_dev(synth_inputs(batch=1, frames=3, height=16, width=24, seed=3), dev)
        full = model(**inp)[0].clone()
        assert model._engine.qkn_stats_epilogue and model._engine.score_bound[1] > ops.ATTN_BOUND_LIMIT
        shard_sequence(model, dist.group.WORLD, transport="p2p")
        model(**inp)                                                  # builds the sharded engine
        f, n = Fused(ops.gemm_qkv_norm_rope), Counter(ops.qknorm_rope)
        real = ops.gemm_qkv_norm_rope, ops.qknorm_rope
        ops.gemm_qkv_norm_rope, ops.qknorm_rope = f, n
        try:
            part = model(**inp)[0].clone()
        finally:
            ops.gemm_qkv_norm_rope, ops.qknorm_rope = real
        again = model(**inp)[0]
        slots = sorted(k[1] for k in model._engine._ws if isinstance(k, tuple) and k[0] == "qk_stats")
        ret[rank] = dict(equal=bool(torch.equal(part, full)), repeat=bool(torch.equal(again, part)), fused=f.calls, qknorm=n.n,
                         slots=slots, blocks=len(model.transformer_blocks), timeouts=model._seq_p2p.timeouts(),
                         diff=float((part.float() - full.float()).abs().max()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_head_parallel_sharded_step_with_the_switch_on_equals_the_unsharded_step(dev):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    ctx = mp.spawn(_sp_worker, args=(2, 33900 + os.getpid() % 500, ret), nprocs=2, join=False)
    deadline = time.monotonic() + WORKER_SECONDS
    while not ctx.join(timeout=5):                        # (returns as soon as a worker ends; raises if one failed)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"the workers did not finish within {WORKER_SECONDS} s")
    print("sharded step, switch on:", dict(ret))
    for r in (0, 1):
        d = ret[r]
        assert d["timeouts"] == 0 and d["equal"] and d["repeat"], d
        assert d["slots"] == [64 // 2], d                                  # the table of the column-block form: 64 // W slots
        # every block one fused launch in the column-block form, layer 1's with the table; no stand-alone q/k-norm launch
        assert [took for took, _ in d["fused"]] == [True] * d["blocks"], d
        assert [st for _, st in d["fused"]] == [i == 1 for i in range(d["blocks"])] and d["qknorm"] == 0, d
