#!/usr/bin/env python3
"""The first-block step cache (model.enable_step_cache) on the bench workload -- 42 layers, 13 x 30 x 45
tokens, synthetic weights, one GPU, the guided step's [uncond, cond] pair -- in ONE process:
  1. what the cache costs on a FULL step: ms per step with threshold 0 (every step full: snapshot, probe, host read, capture)
     against cache off, interleaved over ROUNDS rounds on a precomputed conditioning; and, from one step under the kernel
     timers, the device time of each of the cache's launches;
  2. the table over a STEPS-step guided DDIM clip through the pipeline: per threshold (quantiles of the distances the
     threshold-0 clip reports, and inf under a hit cap) the steps re-used, the seconds per clip and the rel-Fro of the final
     latents against the uncached clip -- beside the fp8 and MX weight modes' drift on the same clip, for scale.
Thresholds found on random weights say nothing about a trained checkpoint: the table shows the mechanism, not a setting.
  python tools/step_cache_probe.py [--rounds 3] [--steps-timed 8] [--warmup 3] [--clip-steps 50] [--out profiles/step_cache_probe.json]"""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
from bind_your_avatar_implementation_amd.pipeline import (BindyouravatarPipeline, cfg_af_matrix, cfg_audio, cfg_id_cond,
                                                            cfg_id_vit_hidden)
from bind_your_avatar_implementation_amd.synth import synth_inputs

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps-timed", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--clip-steps", type=int, default=50)
ap.add_argument("--guidance", type=float, default=6.0)
ap.add_argument("--no-weight-modes", action="store_true", help="skip the fp8 / MX clips")
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


def cache(threshold, **kw):
    if threshold is None:
        model.enable_step_cache(0.0, enabled=False)
    else:
        model.enable_step_cache(threshold, **kw)


# ---- 1. the cost on a full step ---------------------------------------------------------------------------------------
def timed_steps(threshold):
    cache(threshold)
    times = []
    for i in range(a.warmup + a.steps_timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model(**call)
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


model.precompute_conditioning(ident["id_cond"], ident["id_vit_hidden"], ident["audio_embeds"], 13)
arms = {"cache_off": [], "threshold_0": []}
for _ in range(a.rounds):
    arms["cache_off"].append(round(timed_steps(None), 3))
    arms["threshold_0"].append(round(timed_steps(0.0), 3))
cache(0.0)
model(**call)
ops.enable_kernel_timers()
model(**call)
timers = ops.collect_kernel_timers()
launch_ms = {k: [round(t * 1e3, 4) for t in v] for k, v in timers.items() if "step_cache" in k}
step_ms_under_timers = round(sum(sum(v) for v in timers.values()) * 1e3, 3)
model.release_conditioning()
off, on = statistics.median(arms["cache_off"]), statistics.median(arms["threshold_0"])
n = call["hidden_states"].shape[0] * (226 + 13 * 30 * 45) * model.inner_dim
full_step = {"ms_per_step": arms, "median_ms": {"cache_off": off, "threshold_0": on}, "added_ms": round(on - off, 3),
             "added_fraction": round((on - off) / off, 5), "spread_ms": {k: round(max(v) - min(v), 3) for k, v in arms.items()},
             "launch_ms_one_step_under_kernel_timers": launch_ms, "sum_of_all_launches_ms_that_step": step_ms_under_timers,
             "stream_elements": n, "bytes_by_shape": {"snapshot": 4 * n, "probe": 10 * n, "capture": 6 * n},
             "note": "threshold 0: every step is full and pays the snapshot copy, the probe (pass + finish), the host's read of "
                     "the two sums (one synchronisation, mid-step) and the capture; the kernel timers serialise the side stream, "
                     "so their figures are per-launch device times, not the step's"}
print(json.dumps({"full_step": full_step}), flush=True)

# ---- 2. the table over a guided clip ----------------------------------------------------------------------------------
lat = bf(inp["hidden_states"][:, :, :16]).contiguous()
img = bf(inp["hidden_states"][:, :, 16:32]).contiguous()
pipe = BindyouravatarPipeline(model)
kw = dict(height=480, width=720, num_frames=49, num_inference_steps=a.clip_steps, guidance_scale=a.guidance,
          prompt_embeds=bf(inp["encoder_hidden_states"]), negative_prompt_embeds=torch.zeros_like(bf(inp["encoder_hidden_states"])),
          image_latents=img, image_bg_latents=img, id_vit_hidden=[[bf(t) for t in l] for l in inp["id_vit_hidden"]],
          id_cond=[bf(t) for t in inp["id_cond"]], audio_embs=bf(inp["audio_embeds"]), af_matrix=bf(inp["af_matrix"]),
          output_type="latent")


def clip():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = pipe(**kw, latents=lat.clone()).frames
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def rel_fro(x, y):
    return ((x.double() - y.double()).norm() / y.double().norm()).item()


cache(None)
pipe(**dict(kw, num_inference_steps=2), latents=lat.clone())            # warm-up: every shape of the clip
want, s_off = clip()
rows = [{"mode": "cache off", "steps_reused": 0, "seconds_per_clip": round(s_off, 3), "rel_fro_vs_cache_off": 0.0}]
cache(0.0)
got, s0 = clip()
d0 = model.step_cache_stats()["distances"]
rows.append({"mode": "threshold 0", "steps_reused": 0, "seconds_per_clip": round(s0, 3), "rel_fro_vs_cache_off": rel_fro(got, want),
             "bit_equal_to_cache_off": bool(torch.equal(got, want))})
finite = sorted(d for d in d0 if math.isfinite(d))
quantile = lambda q: finite[min(len(finite) - 1, int(q * len(finite)))]
settings = [(f"threshold = q{int(100 * q)} of the threshold-0 distances", quantile(q), None) for q in (0.25, 0.5, 0.75)]
settings.append(("threshold inf, max_consecutive_hits 1", math.inf, 1))
settings.append(("threshold inf, max_consecutive_hits 3", math.inf, 3))
for name, thr, cap in settings:
    cache(thr, max_consecutive_hits=cap)
    got, s = clip()
    st = model.step_cache_stats()
    assert st["steps"] == a.clip_steps == st["full"] + st["reused"]
    rows.append({"mode": name, "threshold": thr if math.isfinite(thr) else "inf", "max_consecutive_hits": cap,
                 "steps_reused": st["reused"], "seconds_per_clip": round(s, 3), "rel_fro_vs_cache_off": rel_fro(got, want),
                 "finite": bool(torch.isfinite(got.float()).all())})
    print(json.dumps(rows[-1]), flush=True)
cache(None)
if not a.no_weight_modes:
    for name, on_, off_ in (("fp8 weights (default Linears), cache off", lambda: model.enable_fp8_weights(), lambda: model.enable_fp8_weights(False)),
                            ("mxfp8 weights (default Linears), cache off", lambda: model.enable_mx_weights("mxfp8"),
                             lambda: model.enable_mx_weights(enabled=False))):
        on_()
        pipe(**dict(kw, num_inference_steps=2), latents=lat.clone())
        got, s = clip()
        off_()
        rows.append({"mode": name, "steps_reused": 0, "seconds_per_clip": round(s, 3), "rel_fro_vs_cache_off": rel_fro(got, want)})
        print(json.dumps(rows[-1]), flush=True)
ops.check_gemm_workspace(dev)
line = json.dumps({"tool": "step_cache_probe", "gpu": torch.cuda.get_device_name(0), "workload": "bench.MODEL_KW, 13 x 30 x 45 tokens, "
                   "[uncond, cond] pair, synthetic weights", "rounds": a.rounds, "steps_timed": a.steps_timed, "warmup": a.warmup,
                   "full_step": full_step, "clip": {"steps": a.clip_steps, "guidance": a.guidance, "scheduler": "DDIM",
                                                    "distances_at_threshold_0": ["inf" if math.isinf(d) else d for d in d0],
                                                    "rows": rows},
                   "caveat": "synthetic (random) weights: the thresholds and drifts say nothing about a trained checkpoint"})
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
