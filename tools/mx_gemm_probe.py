"""MX weights (enable_mx_weights) against bf16 and per-row fp8, on one GPU:
  1. GEMM TFLOP/s of bf16 (bya_gemm_bf16), per-row fp8 (bya_gemm_fp8), mxfp8 and mxfp6 (bya_gemm_mx) at the DiT Linear
     shapes 17776 x {9216, 3072, 12288, 3072} x {3072, 3072, 3072, 12288} and the same at 2222 rows, each as a fraction of
     its dense peak (MI355X_MICROARCH.md: bf16 2.5, e4m3 5, e2m3 10 PFLOP/s), plus the activation quantisers' time;
  2. the headline step (49 x 480 x 720 -> 13 x 60 x 90 latents, 42 layers, 2 identities, eager) in steps/s per mode: three
     interleaved rounds of 5 timed steps each, the best round kept;
  3. the 42-layer output drift of each mode against the bf16 engine (rel. Frobenius; random-init weights).
--fp4: the same three sections for e2m1 weights (enable_mx_weights(fmt, weight_format="mxfp4"), bya_gemm_mx_mixed) against
same-format weights, for both activation formats: GEMM time per shape in interleaved rounds, the step of the four MX modes
in interleaved rounds, and each mode's drift against the bf16 engine (profiles/mx_fp4_probe.json).
usage: python tools/mx_gemm_probe.py [out.json] [--gemm-only] [--fp4]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
PEAK = {"bf16": 2500.0, "fp8": 5000.0, "mxfp8": 5000.0, "mxfp6": 10000.0}
SHAPES = [("qkv", 9216, 3072, None, False), ("attn_out", 3072, 3072, None, True), ("ff1", 12288, 3072, "gelu_tanh", False),
          ("ff2", 3072, 12288, None, True)]


def best_us(fn, reps=3, inner=10):
    best = 1e30
    for _ in range(reps):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / inner * 1e3)
    return best


def fp4_gemm_section(rounds=3):
    """bya_gemm_mx_mixed with e2m1 weights next to bya_gemm_mx on the same activations; fraction of the ACTIVATION format's
    peak (at which rate the mixed instruction issues is one of the things this measures)."""
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for M in (17776, 2222):
        for name, N, K, act, has_res in SHAPES:
            a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
            b = torch.randn(N, device=dev, generator=g).to(torch.bfloat16)
            res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16) if has_res else None
            c = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            wq = {f: ops.quantize_mx(w, f) for f in ("mxfp8", "mxfp6", "mxfp4")}
            runs = {}
            for f in ("mxfp8", "mxfp6"):
                ac, asc = ops.quantize_mx(a, f)
                for wf in (f, "mxfp4"):
                    wc, wsc = wq[wf]
                    runs[f if wf == f else f + "*mxfp4"] = (
                        lambda ac=ac, asc=asc, wc=wc, wsc=wsc, f=f, wf=wf:
                        ops.gemm_mx(ac, asc, wc, wsc, c, f, bias=b, res=res, act=act, w_fmt=wf))
            entry = {"M": M, "N": N, "K": K}
            flop = 2.0 * M * N * K
            us = {mode: 1e30 for mode in runs}
            for _ in range(rounds):                                  # interleaved: every mode once per round
                for mode, fn in runs.items():
                    us[mode] = min(us[mode], best_us(fn, reps=1))
            for mode in runs:
                tf = flop / us[mode] * 1e-6
                entry[mode] = {"us": round(us[mode], 1), "tflops": round(tf, 1),
                               "frac_of_peak": round(tf / PEAK[mode.split("*")[0]], 3)}
            key = f"{name}@{M}"
            out[key] = entry
            print(key, json.dumps(entry), flush=True)
            del a, w, res, c, wq, runs
            torch.cuda.empty_cache()
    return out


def gemm_section():
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for M in (17776, 2222):
        for name, N, K, act, has_res in SHAPES:
            a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
            b = torch.randn(N, device=dev, generator=g).to(torch.bfloat16)
            res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16) if has_res else None
            c = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            a8, sa = ops.quantize_rows_fp8(a)
            w8, sw = ops.quantize_rows_fp8(w)
            mx = {f: (ops.quantize_mx(a, f), ops.quantize_mx(w, f)) for f in ("mxfp8", "mxfp6")}
            runs = {"bf16": lambda: ops.gemm(a, w, c, bias=b, res=res, act=act),
                    "fp8": lambda: ops.gemm_fp8(a8, sa, w8, sw, c, bias=b, res=res, act=act)}
            for f in ("mxfp8", "mxfp6"):
                (ac, asc), (wc, wsc) = mx[f]
                runs[f] = (lambda ac=ac, asc=asc, wc=wc, wsc=wsc, f=f:
                           ops.gemm_mx(ac, asc, wc, wsc, c, f, bias=b, res=res, act=act))
            entry = {"M": M, "N": N, "K": K}
            flop = 2.0 * M * N * K
            for mode, fn in runs.items():
                us = best_us(fn)
                tf = flop / us * 1e-6
                entry[mode] = {"us": round(us, 1), "tflops": round(tf, 1), "frac_of_peak": round(tf / PEAK[mode], 3)}
            # the activation quantisers (what the fused LayerNorm saves in front of q|k|v and ff.net.0)
            entry["quantise_us"] = {"fp8_rows": round(best_us(lambda: ops.quantize_rows_fp8(a, a8, sa)), 1)}
            for f in ("mxfp8", "mxfp6"):
                (ac, asc), _ = mx[f]
                entry["quantise_us"][f] = round(best_us(lambda ac=ac, asc=asc, f=f: ops.quantize_mx(a, f, ac, asc)), 1)
            key = f"{name}@{M}"
            out[key] = entry
            print(key, json.dumps(entry), flush=True)
            del a, w, res, c, a8, w8, mx
            torch.cuda.empty_cache()
    return out


def step_section(steps=5, warmup=2, rounds=3, fp4=False):
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
    modes = {"bf16": lambda: None, "fp8": lambda: model.enable_fp8_weights(),
             "mxfp8": lambda: model.enable_mx_weights("mxfp8"), "mxfp6": lambda: model.enable_mx_weights("mxfp6")}
    if fp4:
        modes = {"bf16": lambda: None}
        for f in ("mxfp8", "mxfp6"):
            modes[f] = lambda f=f: model.enable_mx_weights(f)
            modes[f + "*mxfp4"] = lambda f=f: model.enable_mx_weights(f, weight_format="mxfp4")
    res, outs = {}, {}
    # rounds x modes, interleaved (each mode rebuilds its engine every round); the best round per mode is kept
    for rnd in range(rounds):
        for mode, enable in modes.items():
            model.enable_fp8_weights(False)
            model.enable_mx_weights(enabled=False)
            enable()
            for _ in range(warmup):
                model(return_dict=False, denoise_step=0, **inp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                o = model(return_dict=False, denoise_step=0, **inp)[0]
            torch.cuda.synchronize()
            sec = (time.perf_counter() - t0) / steps
            outs[mode] = o.float().clone()
            r = res.setdefault(mode, {"ms_per_step_rounds": []})
            r["ms_per_step_rounds"].append(round(sec * 1e3, 1))
            r["ms_per_step"] = min(r["ms_per_step_rounds"])
            r["steps_per_s"] = round(1e3 / r["ms_per_step"], 3)
            if mode != "bf16":
                ref = outs["bf16"]
                r["drift_vs_bf16_42_layers"] = float((outs[mode] - ref).norm() / ref.norm())
            print(rnd, mode, json.dumps(r), flush=True)
    # per-kernel time of the two MX steps' GEMMs and quantisers (kernel timers: one extra step each)
    for mode in (("mxfp6*mxfp4", "mxfp8*mxfp4") if fp4 else ("fp8", "mxfp6")):
        model.enable_fp8_weights(mode == "fp8")
        model.enable_mx_weights(enabled=False)
        if mode != "fp8":
            modes[mode]()
        model(return_dict=False, denoise_step=0, **inp)
        ops.enable_kernel_timers()
        model(return_dict=False, denoise_step=0, **inp)
        torch.cuda.synchronize()
        kt = ops.collect_kernel_timers()
        res[mode]["kernel_ms_per_step"] = {k: round(sum(v) * 1e3, 2) for k, v in kt.items()
                                           if k.startswith(("bya_gemm", "bya_quantize", "bya_layernorm"))}
        print(mode, json.dumps(res[mode]["kernel_ms_per_step"]), flush=True)
    return res


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    fp4 = "--fp4" in sys.argv
    result = {"device": torch.cuda.get_device_name(0), "gemm": fp4_gemm_section() if fp4 else gemm_section()}
    if "--gemm-only" not in sys.argv:
        result["step"] = step_section(fp4=fp4)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
