"""What ONE ``DenoiseEngine.step`` hands to the library, and in which host order: the timer bucket (shape labels on) of every
launch, ``ops.ATTN_VARIANTS`` and, on a process group, ``parallel.COLLECTIVE_CALLS`` -- for every arm of the step (switches,
fp8 / MX weights, taps, forcing, no audio, batch launches, the device score bound, the four transports of the joint
attention), against a recording taken before ``_step`` was split into stage methods (tests/golden/engine_launch_order.json).
``ops._begin`` is hooked instead of switching the timers on, so the side stream of the conditioning stays active.  The
geometry is SMALL_KW of tests/test_forward_gpu.py with 3 frames of 16 x 24; the first step of a case builds the engine and
is not recorded, the second is.

``python tests/test_engine_launch_order_gpu.py`` rewrites the recording from the engine on the path and prints, per case,
the sha256 of the prediction's bytes (device-bound cases: of ``qk_flags`` and of the statistics table's maximum too), for a
one-off comparison of two trees on one machine.  The recording pins a refactor to the code before it: regenerate it only
when a launch is MEANT to change, from the commit that is meant to be matched."""
import hashlib
import json
import os
import time

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_order.json")
WORKER_SECONDS = 420        # per spawned worker set; a healthy run takes a fraction of it
SIX = ("qkv", "out", "ff1", "ff2", "po", "ao")

# case -> (environment while the engine is built, model set-up, what the step is given)
LOCAL = {
    "default": ({}, None, None),
    "qkn_epilogue_off": ({"BYA_QKN_EPILOGUE": "0"}, None, None),
    "fused_attn_mix_off": ({"BYA_FUSED_ATTN_MIX": "0"}, None, None),
    "mix_before_projection_off": ({"BYA_MIX_BEFORE_PROJECTION": "0"}, None, None),
    "taps": ({}, None, "taps"),
    "forcing": ({}, None, "forcing"),
    "no_audio": ({}, None, "no_audio"),
    "batch_launches": ({}, lambda m: setattr(m, "batch_launches", True), None),
    "fp8_default": ({}, lambda m: m.enable_fp8_weights(), None),
    "fp8_all_fuse_qk_norm": ({}, lambda m: m.enable_fp8_weights(linears="all", fuse_qk_norm=True), None),
    "mxfp8_six": ({}, lambda m: m.enable_mx_weights("mxfp8", linears=SIX), None),
    "mxfp8_six_fused_persistent": ({}, lambda m: m.enable_mx_weights("mxfp8", linears=SIX, fuse_attention_quant=True,
                                                                       fuse_qk_norm=True, persistent_gemm=True), None),
    "mxfp6_mxfp4_persistent": ({}, lambda m: m.enable_mx_weights("mxfp6", linears=SIX, weight_format="mxfp4",
                                                                   persistent_gemm_mxfp6=True), None),
    "mxfp8_six_cross_quant_off": ({}, lambda m: m.enable_mx_weights("mxfp8", linears=SIX, fuse_cross_attention_quant=False), None),
    "device_bound": ({}, None, "gains"),
    "device_bound_stats_epilogue": ({"BYA_QKN_STATS_EPILOGUE": "1"}, None, "gains"),
}
RCCL = ("rccl_head_parallel", "rccl_allgather")
P2P = {"p2p_default": {}, "p2p_v_first_segment_mix": {"BYA_SP_OVERLAP_V": "all", "BYA_SP_SEGMENT_MIX": "1"}}
CASES = list(LOCAL) + list(RCCL) + list(P2P)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def recorded(call, group=False):
    """``call()`` with every launch's bucket recorded -> (its result, {"launches", "attn_variants"[, "collectives"]})."""
    from bind_your_avatar_implementation_amd import ops, parallel
    seq = []
    saved = ops._begin, ops._SHAPE_LABELS
    ops._begin, ops._SHAPE_LABELS = (lambda name, flops=0.0: seq.append(name)), True      # (-> None, like the timers when off)
    ops.ATTN_VARIANTS.clear()
    parallel.COLLECTIVE_CALLS.clear()
    try:
        out = call()
        torch.cuda.synchronize()
    finally:
        ops._begin, ops._SHAPE_LABELS = saved
    rec = dict(launches=seq, attn_variants={"/".join(map(str, k)): n for k, n in sorted(ops.ATTN_VARIANTS.items(), key=str)})
    if group:
        rec["collectives"] = dict(sorted(parallel.COLLECTIVE_CALLS.items()))
    return out, rec


def raise_layer1_gains(model):
    with torch.no_grad():
        model.transformer_blocks[1].attn1.norm_q.weight.mul_(2.0)
        model.transformer_blocks[1].attn1.norm_k.weight[::16].mul_(5.0)


def make_model(dev, seed=1):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from test_forward_gpu import SMALL_KW
    return BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=seed, fast=True)


def inputs(dev, batch):
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    from test_forward_gpu import to_dev
    return to_dev(synth_inputs(batch=batch, frames=3, height=16, width=24, seed=3, uncond_first=batch == 2), dev)


_MODELS = {}


def run_local(name, dev):
    """-> (record, hashes) of one unsharded case, batch 2."""
    env, setup, what = LOCAL[name]
    kind = "gains" if what == "gains" else "plain"
    model = _MODELS.get(kind)
    if model is None:
        model = _MODELS[kind] = make_model(dev)
        if kind == "gains":
            raise_layer1_gains(model)
    model.enable_fp8_weights(False)
    model.enable_mx_weights(enabled=False)
    model.batch_launches = False
    if setup is not None:
        setup(model)
    gi = inputs(dev, 2)
    if what == "no_audio":
        gi["audio_embeds"] = None
    if what == "forcing":
        lab = torch.arange(3 * 8 * 12) % 3
        forcing = torch.zeros(1, 3 * 8 * 12, 2)
        forcing[0, lab == 0, 0] = 1
        forcing[0, lab == 1, 1] = 1
        gi["routing_logits_forcing"] = forcing.to(dev, torch.bfloat16)
    os.environ.update(env)
    try:
        model.invalidate_engine()
        model(**gi)                                  # builds the engine (its switches are read here); not recorded
    finally:
        for k in env:
            del os.environ[k]
    eng = model._engine
    if what == "taps":
        call = lambda: eng.step(gi["hidden_states"], gi["encoder_hidden_states"], gi["timestep"], gi["image_rotary_emb"],
                                gi["id_cond"], gi["id_vit_hidden"], gi["audio_embeds"], gi["af_matrix"], None, taps={})
    else:
        call = lambda: model(**gi)[0]
    out, rec = recorded(call)
    hashes = dict(out=sha(out))
    if what == "gains":
        from bind_your_avatar_implementation_amd import ops
        assert eng.score_bound[1] > ops.ATTN_BOUND_LIMIT
        table = next(v for k, v in eng._ws.items() if isinstance(k, tuple) and k[0] == "qk_stats")
        hashes.update(qk_flags=sha(eng._ws["qk_flags"]), stats_max=sha(table.amax(0)))
    model.invalidate_engine()
    return rec, hashes


def _rccl_worker(rank, port, ret, name):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["BYA_SP_TRANSPORT"] = "torch"
    if name == "rccl_allgather":
        os.environ["BYA_SP_ALLGATHER"] = "1"          # exchange A in its K/V all-gather form
        os.environ["BYA_ROUTER_REPLICATED"] = "1"     # exchange B as one all-gather of the router rows
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from bind_your_avatar_implementation_amd import parallel
        model, inp = make_model(dev), inputs(dev, 1)
        parallel.FORCE_COLLECTIVES = True
        parallel.shard_sequence(model, dist.group.WORLD)
        model(**inp)                                   # builds the sharded engine; not recorded
        out, rec = recorded(lambda: model(**inp)[0], group=True)
        ret[name] = (rec, dict(out=sha(out)))
    finally:
        dist.destroy_process_group()


def _p2p_worker(rank, world, port, ret, name):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.update(P2P[name])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # 2 ranks share the single test GPU
    try:
        from bind_your_avatar_implementation_amd.parallel import shard_sequence
        dev = torch.device("cuda:0")
        model, inp = make_model(dev), inputs(dev, 1)
        shard_sequence(model, dist.group.WORLD, transport="p2p")
        model(**inp)                                   # builds the sharded engine; not recorded
        out, rec = recorded(lambda: model(**inp)[0], group=True)
        assert model._seq_p2p.timeouts() == 0
        if rank == 0:
            ret[name] = (rec, dict(out=sha(out)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def run_spawned(name):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    port = 34500 + os.getpid() % 500 + CASES.index(name)
    if name in RCCL:
        ctx = mp.spawn(_rccl_worker, args=(port, ret, name), nprocs=1, join=False)
    else:
        ctx = mp.spawn(_p2p_worker, args=(2, port, ret, name), nprocs=2, join=False)
    deadline = time.monotonic() + WORKER_SECONDS
    while not ctx.join(timeout=5):                        # (returns as soon as a worker ends; raises if one failed)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            raise RuntimeError(f"{name}: the workers did not finish within {WORKER_SECONDS} s")
    return ret[name]


def run_case(name, dev):
    return run_local(name, dev) if name in LOCAL else run_spawned(name)


def load_golden():
    """-> {case: record}: the file holds every bucket once (``names``) and a case's launches as indices into them."""
    with open(GOLDEN) as f:
        g = json.load(f)
    return {c: dict(r, launches=[g["names"][j] for j in r["launches"]]) for c, r in g["cases"].items()}


def write_golden(table):
    names = sorted({n for r in table.values() for n in r["launches"]})
    at = {n: j for j, n in enumerate(names)}
    cases = {c: dict(r, launches=[at[n] for n in r["launches"]]) for c, r in table.items()}
    with open(GOLDEN, "w") as f:                                          # one bucket, one case per line
        f.write('{"names": [\n' + ",\n".join(json.dumps(n) for n in names) + '\n],\n"cases": {\n'
                + ",\n".join(f"{json.dumps(c)}: {json.dumps(cases[c])}" for c in table) + "\n}}\n")


def _same(a, b):
    return all(a.get(k) == b.get(k) for k in ("launches", "attn_variants"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_step_issues_the_recorded_launches_in_the_recorded_order(dev, name):
    golden = load_golden()
    if name not in golden:
        pytest.fail(f"{name}: no recording (a case that could not be run when the recording was taken is left out of CASES)")
    rec, _ = run_case(name, dev)
    want = golden[name]
    got, exp = rec["launches"], want["launches"]
    first = next((j for j, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
    assert got == exp, f"{name}: {len(got)} launches against {len(exp)} recorded; first difference at {first}: " \
                       f"{got[first:first + 3]} against {exp[first:first + 3]}"
    assert rec["attn_variants"] == want["attn_variants"]
    assert rec.get("collectives") == want.get("collectives")


def test_the_recording_covers_every_case_and_every_arm_was_taken():
    """Conditions on the recording itself (no GPU work): every golden case is one that is compared, the hook saw the whole
    step, and every case ran launches the default did not."""
    golden = load_golden()
    assert sorted(golden) == sorted(CASES)
    base = golden["default"]
    for bucket in ("bya_attn_kv_mix", "bya_router_scores", "bya_router_head", ":joint"):      # (":joint": the joint attention's tag)
        assert any(bucket in n for n in base["launches"]), bucket
    for name in CASES[1:]:           # (among themselves two may agree: taps take the launches of the unfused mix)
        assert not _same(golden[name], base), f"{name} issued what the default issued"
    for name in list(RCCL) + list(P2P):
        assert golden[name]["collectives"], name


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    device = torch.device("cuda:0")
    table = {}
    for case in CASES:
        table[case], hashes = run_case(case, device)
        print(f"{case}: {len(table[case]['launches'])} launches; " + " ".join(f"{k}={v}" for k, v in hashes.items()), flush=True)
    if "--hashes-only" not in sys.argv:
        write_golden(table)
        print(f"{len(table)} cases -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
