#!/usr/bin/env python3
"""The guided step as the pipeline runs it -- the [uncond, cond] pair (B = 2) on a precomputed conditioning -- on one GPU, four
arms interleaved over ROUNDS rounds in ONE process (42 layers, 13 x 30 x 45 tokens, the pipeline_loop.py geometry):
  eager, batch_launches off | eager, batch_launches on | graph replay that recomputes the conditioning | graph replay on the cache
Prints one JSON line: per arm the per-round medians of the step time in ms, and the launches per step of the four batched kernels.
  python tools/cfg_pair_step.py [--rounds 3] [--steps 10] [--warmup 3] [--out profiles/cfg_pair_step.json]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
from bind_your_avatar_implementation_amd.pipeline import cfg_af_matrix, cfg_audio, cfg_id_cond, cfg_id_vit_hidden
from bind_your_avatar_implementation_amd.synth import synth_inputs

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
model = BindyouravatarTransformer3DModel(**bench.MODEL_KW, device=dev).init_synthetic(seed=0, fast=True)
inp = synth_inputs(batch=1, seed=0, device="cpu")
bf = lambda t: t.to(dev, torch.bfloat16)
pair = lambda t: torch.cat([bf(t)] * 2)
ident = dict(id_cond=cfg_id_cond([bf(t) for t in inp["id_cond"]], False),
             id_vit_hidden=cfg_id_vit_hidden([[bf(t) for t in l] for l in inp["id_vit_hidden"]], False),
             audio_embeds=cfg_audio(bf(inp["audio_embeds"])))
call = dict(hidden_states=pair(inp["hidden_states"]), encoder_hidden_states=pair(inp["encoder_hidden_states"]),
            timestep=torch.tensor([500, 500], device=dev), image_rotary_emb=tuple(t.to(dev) for t in inp["image_rotary_emb"]),
            af_matrix=cfg_af_matrix(bf(inp["af_matrix"]), False), **ident)


def arm(batch, graph, cache):
    """-> (median step time in ms, launches per step by label or None under replay)"""
    model.use_hip_graph, model.batch_launches = False, batch
    model.invalidate_engine()
    if cache:
        model.precompute_conditioning(ident["id_cond"], ident["id_vit_hidden"], ident["audio_embeds"], 13)
    counts = None
    if not graph:
        ops.enable_kernel_timers()
        model(**call)
        counts = {k: len(v) for k, v in ops.collect_kernel_timers().items()
                  if k.startswith(("bya_attn_kv_mix", "bya_router_scores", "bya_router_head"))}
    model.use_hip_graph = graph
    times = []
    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model(**call)
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    model.use_hip_graph = False
    model.release_conditioning()
    return statistics.median(times), counts


ARMS = {"eager_loops": (False, False, True), "eager_batch_launches": (True, False, True),
        "graph_recompute": (False, True, False), "graph_on_cache": (False, True, True)}
res = {k: {"ms": [], "launches": None} for k in ARMS}
for _ in range(a.rounds):
    for name, cfg in ARMS.items():
        ms, counts = arm(*cfg)
        res[name]["ms"].append(round(ms, 3))
        res[name]["launches"] = counts
for v in res.values():
    v["median_ms"] = statistics.median(v["ms"])
ops.check_gemm_workspace(dev)
line = json.dumps({"tool": "cfg_pair_step", "gpu": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
                   "warmup": a.warmup, "batch": 2, "arms": res})
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
