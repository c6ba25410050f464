"""mxfp6 (e2m3) activations with mxfp6 or mxfp4 weights on the PERSISTENT 256 x 256 MX kernel (bya_gemm_mx_call, kernel = 17 =
BYA_MX_KERNEL_FP6 + 1) against the tiled 256 x 256 / 128 x 128 kernels that run them otherwise (kernel = 1: without the flag
mxfp6 stays tiled), on one GPU, one process:
  1. the four MX Linears of a DiT block (q|k|v 9216 x 3072, to_out 3072 x 3072, ff.net.0 12288 x 3072 + GELU, ff.net.2
     3072 x 12288) with the bf16 epilogue, ff.net.0 with the quantising epilogue (to mxfp6) and q|k|v with the q/k-norm + RoPE
     epilogue, at 17776 and 2222 rows, for both weight formats, two arms in interleaved rounds (every arm once per round; every
     round kept):
       (a) tiled:  kernel = 1 -- the tiled kernel, whose machine code is the parent's (profiles/isa_fingerprint_*.txt): the
                   reference for time,
       (b) p256:   kernel = 17 -- the persistent kernel's e2m3 instance,
     with the output bytes of the two arms compared in the same run ((a) = (b) is the claim);
  2. the headline 42-layer steps of enable_mx_weights("mxfp6") and enable_mx_weights("mxfp6", weight_format="mxfp4")
     (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) with persistent_gemm_mxfp6 off / on, in interleaved rounds of
     5 timed steps, and whether the two outputs are bit-identical.
Nothing is promised about time: the file reports every round.
usage: python tools/mx_p256_fp6_probe.py [out.json] [--gemm-only]
(default out: profiles/mx_p256_fp6_probe.json)"""
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
FMT = "mxfp6"
TEXT, K_SCALE = 226, 0.18
ARMS = {"tiled": 1, "p256": 17}
W_FORMATS = ("mxfp6", "mxfp4")
# name: (N, K, epilogue)
LAUNCHES = {"qkv": (9216, 3072, "bf16"), "out": (3072, 3072, "bf16"), "ff1": (12288, 3072, "gelu"), "ff2": (3072, 12288, "bf16"),
            "ff1_quant": (12288, 3072, "quant"), "qkv_fused": (9216, 3072, "qkn")}


def best_us(fn, inner=10):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def launch_section(rounds=3):
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for (name, (N, K, epi)), M, wf in itertools.product(LAUNCHES.items(), (17776, 2222), W_FORMATS):
        w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
        wq = ops.quantize_mx(w, wf)
        ac, asc = ops.quantize_mx(torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16), FMT)
        b = torch.randn(N, device=dev, generator=g).to(torch.bfloat16)
        kw = dict(bias=b)
        if epi == "gelu":
            kw["act"] = "gelu_tanh"
        if epi == "qkn":
            qw, qb, kw_, kb = ((torch.randn(64, device=dev, generator=g) * 0.3 + (1 if i % 2 == 0 else 0)).to(torch.bfloat16)
                               for i in range(4))
            ang = torch.rand(M - TEXT, 64, device=dev, generator=g) * 6.3
            kw.update(split=(N // 3, M * (N // 3)),
                      norm=dict(qw=qw, qb=qb, kw=kw_, kb=kb, cos=torch.cos(ang).contiguous(), sin=torch.sin(ang).contiguous(),
                                text_rows=TEXT, eps=1e-6, k_scale=K_SCALE))
        bufs, fns, paths = {}, {}, {}
        for arm, kernel in ARMS.items():
            if epi == "quant":
                o = torch.full((M, ops.mx_code_bytes(N, FMT)), 0xAA, dtype=torch.uint8, device=dev)
                akw = dict(kw, act="gelu_tanh", out_scales=torch.full((M, N // 32), 0xAA, dtype=torch.uint8, device=dev), out_fmt=FMT)
                bufs[arm] = (o, akw["out_scales"])
            else:
                o = torch.full((3, M, N // 3) if epi == "qkn" else (M, N), float("nan"), dtype=torch.bfloat16, device=dev)
                akw = kw
                bufs[arm] = (o,)
            args = (ac, asc, *wq, o[0] if epi == "qkn" else o, kernel, FMT, wf)
            paths[arm] = ops.gemm_mx_call_plan(*args, **akw)["path"]
            fns[arm] = (lambda args=args, akw=akw: ops.gemm_mx_call(*args, **akw))
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        raw = lambda t: t.view(torch.int16) if t.dtype == torch.bfloat16 else t
        same = {f"{x}={y}": all(bool(torch.equal(raw(p), raw(q))) for p, q in zip(bufs[x], bufs[y]))
                for x, y in itertools.combinations(ARMS, 2)}
        us = {k: [] for k in ARMS}
        for _ in range(rounds):                                          # interleaved: every arm once per round
            for k in ARMS:
                us[k].append(round(best_us(fns[k]), 1))
        entry = {"M": M, "N": N, "K": K, "w_fmt": wf, "epilogue": epi, "paths": paths, "bytes_identical": same}
        for k in ARMS:
            entry[k + "_us_rounds"] = us[k]
            entry[k + "_us"] = min(us[k])
            entry[k + "_pflops"] = round(2.0 * M * N * K / min(us[k]) * 1e-9, 3)
        entry["p256_over_tiled"] = round(min(us["p256"]) / min(us["tiled"]), 3)
        entry["every_p256_round_beats_every_tiled_round"] = max(us["p256"]) < min(us["tiled"])
        entry["every_p256_round_loses_to_every_tiled_round"] = min(us["p256"]) > max(us["tiled"])
        out[f"{name}@{M}x{wf}"] = entry
        print(f"{name}@{M}x{wf}", json.dumps(entry), flush=True)
        del w, wq, ac, asc, bufs, fns
        torch.cuda.empty_cache()
    return out


def step_section(steps=5, warmup=2, rounds=3):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    kw = dict(num_attention_heads=48, attention_head_dim=64, in_channels=48, out_channels=16, num_layers=42,
              use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True, is_train_face=True,
              cross_attn_interval=2, local_face_scale=1.0, is_train_audio=True, audio_attn_interval=1,
              sample_height=60, sample_width=90, sample_frames=49)
    model = BindyouravatarTransformer3DModel(**kw, device=dev).init_synthetic(seed=0, fast=True)
    d = synth_inputs(batch=1, frames=13, height=60, width=90, n_id=2, seed=0, device="cpu")
    inp = {k: (v.to(dev, torch.bfloat16) if torch.is_tensor(v) and v.is_floating_point() else
               (v.to(dev) if torch.is_tensor(v) else v)) for k, v in d.items()}
    inp["image_rotary_emb"] = tuple(t.to(dev, torch.float32) for t in d["image_rotary_emb"])
    inp["id_cond"] = [t.to(dev, torch.bfloat16) for t in d["id_cond"]]
    inp["id_vit_hidden"] = [[t.to(dev, torch.bfloat16) for t in l] for l in d["id_vit_hidden"]]
    both = {}
    for wf in W_FORMATS:
        both[f"mxfp6_x_{wf}"] = one_step_section(model, inp, wf, steps, warmup, rounds)
    return both


def one_step_section(model, inp, wf, steps, warmup, rounds):
    res, outs = {}, {}
    for rnd in range(rounds):                                            # rounds x {off, on}, interleaved
        for pg in (False, True):
            model.enable_mx_weights(FMT, weight_format=wf, persistent_gemm_mxfp6=pg)
            for _ in range(warmup):
                model(return_dict=False, denoise_step=0, **inp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                o = model(return_dict=False, denoise_step=0, **inp)[0]
            torch.cuda.synchronize()
            sec = (time.perf_counter() - t0) / steps
            arm = "persistent_gemm_mxfp6_on" if pg else "persistent_gemm_mxfp6_off"
            outs[arm] = o.clone()
            r = res.setdefault(arm, {"ms_per_step_rounds": []})
            r["ms_per_step_rounds"].append(round(sec * 1e3, 1))
            r["ms_per_step"] = min(r["ms_per_step_rounds"])
            print(wf, rnd, arm, json.dumps(r), flush=True)
    res["bit_identical"] = bool(torch.equal(outs["persistent_gemm_mxfp6_on"], outs["persistent_gemm_mxfp6_off"]))
    res["every_on_round_beats_every_off_round"] = \
        max(res["persistent_gemm_mxfp6_on"]["ms_per_step_rounds"]) < min(res["persistent_gemm_mxfp6_off"]["ms_per_step_rounds"])
    return res


def main():
    argv = sys.argv[1:]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "mx_p256_fp6_probe.json"))
    result = {"device": torch.cuda.get_device_name(0), "launch": launch_section()}
    if "--gemm-only" not in argv:
        result["step"] = step_section()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
