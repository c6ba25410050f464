"""The persistent 256 x 256 MX GEMM (csrc/gemm_mx_v4.hip; option mx_kernel = 1) against the 128 x 128 kernel of csrc/gemm_mx.hip
(option 0: the reference for time) for mxfp8 activations x mxfp8 weights, on one GPU, one process:
  1. the four DiT Linear shapes at 17776 and 2222 rows, plain epilogue (bias; to_out and ff.net.2 with gates + residual) and,
     for ff.net.0, the quantising one (bias + GELU), in three interleaved rounds, EVERY round kept; the per-row fp8 persistent
     kernel (bya_gemm_fp8) on the same shapes in the same rounds as the ceiling; the plan each arm took; whether the two MX
     kernels wrote the same bytes;
  2. the headline 42-layer mxfp8 step (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) with
     enable_mx_weights(persistent_gemm=...) on and off, in interleaved rounds of 5 timed steps, and whether the outputs are
     bit-identical.
usage: python tools/mx_p256_probe.py [out.json] [--gemm-only]     (default out: profiles/mx_p256_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
F = "mxfp8"
# name -> (N, K, epilogue)
SHAPES = {"qkv": (9216, 3072, "bias"), "to_out": (3072, 3072, "gate_res"), "ff1": (12288, 3072, "gelu"),
          "ff2": (3072, 12288, "gate_res")}


def time_us(fn, inner=10):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def gemm_section(rounds=3):
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for M in (17776, 2222):
        for name, (N, K, epi) in SHAPES.items():
            a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
            b = torch.randn(N, device=dev, generator=g).to(torch.bfloat16)
            gate = torch.randn(2, N, device=dev, generator=g).to(torch.bfloat16)
            res = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
            ac, asc = ops.quantize_mx(a, F)
            wc, wsc = ops.quantize_mx(w, F)
            a8, sa8 = ops.quantize_rows_fp8(a)
            w8, sw8 = ops.quantize_rows_fp8(w)
            kw = dict(bias=b)
            if epi == "gate_res":
                kw.update(res=res, gate0=gate[0], gate1=gate[1], gate_split=226)
            elif epi == "gelu":
                kw.update(act="gelu_tanh")
            c = {o: torch.empty(M, N, dtype=torch.bfloat16, device=dev) for o in (0, 1, "fp8")}
            arms = {}

            def mx(o, c=c, ac=ac, asc=asc, wc=wc, wsc=wsc, kw=kw):
                with ops.options(mx_kernel=o):
                    ops.gemm_mx(ac, asc, wc, wsc, c[o], F, **kw)

            arms["t128"] = lambda mx=mx: mx(0)
            arms["p256"] = lambda mx=mx: mx(1)
            arms["fp8_p256"] = lambda c=c, a8=a8, sa8=sa8, w8=w8, sw8=sw8, kw=kw: ops.gemm_fp8(a8, sa8, w8, sw8, c["fp8"], **kw)
            with ops.options(mx_kernel=1):
                plan = ops.gemm_mx_plan(ac, asc, wc, wsc, c[1], F, **kw)["path"]
            entry = {"M": M, "N": N, "K": K, "epilogue": epi, "plan_at_option_1": plan,
                     "fp8_plan": ops.gemm_fp8_plan(a8, sa8, w8, sw8, c["fp8"], **kw)["path"]}
            arms["t128"]()
            arms["p256"]()
            entry["bytes_identical"] = bool(torch.equal(c[0].view(torch.int16), c[1].view(torch.int16)))
            if epi == "gelu":                                            # ff.net.0 also with the quantising epilogue
                q = {o: (torch.empty(M, N, dtype=torch.uint8, device=dev), torch.empty(M, N // 32, dtype=torch.uint8, device=dev))
                     for o in (0, 1)}

                def mxq(o, q=q, ac=ac, asc=asc, wc=wc, wsc=wsc, b=b):
                    with ops.options(mx_kernel=o):
                        ops.gemm_mx_quant(ac, asc, wc, wsc, *q[o], F, out_fmt=F, bias=b, act="gelu_tanh")

                arms["t128_quant"] = lambda mxq=mxq: mxq(0)
                arms["p256_quant"] = lambda mxq=mxq: mxq(1)
                arms["t128_quant"]()
                arms["p256_quant"]()
                entry["quant_bytes_identical"] = bool(torch.equal(q[0][0], q[1][0]) and torch.equal(q[0][1], q[1][1]))
            us = {k: [] for k in arms}
            for _ in range(rounds):                                      # interleaved: every arm once per round
                for k, fn in arms.items():
                    us[k].append(round(time_us(fn), 1))
            entry["us_rounds"] = us
            flop = 2.0 * M * N * K
            entry["tflops_best"] = {k: round(flop / min(v) / 1e6, 0) for k, v in us.items()}
            entry["p256_over_t128_rounds"] = [round(p / t, 3) for p, t in zip(us["p256"], us["t128"])]
            entry["p256_faster_than_every_t128_round"] = max(us["p256"]) < min(us["t128"])
            if "p256_quant" in us:
                entry["p256_quant_over_t128_quant_rounds"] = [round(p / t, 3) for p, t in zip(us["p256_quant"], us["t128_quant"])]
            out[f"{name}@{M}"] = entry
            print(f"{name}@{M}", json.dumps(entry), flush=True)
            del a, w, res, c, arms
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
    res, outs = {}, {}
    for rnd in range(rounds):
        for on in (False, True):
            model.enable_mx_weights(F, persistent_gemm=on)
            for _ in range(warmup):
                model(return_dict=False, denoise_step=0, **inp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                o = model(return_dict=False, denoise_step=0, **inp)[0]
            torch.cuda.synchronize()
            arm = "persistent_gemm" if on else "t128"
            outs[arm] = o.clone()
            res.setdefault(arm, {"ms_per_step_rounds": []})["ms_per_step_rounds"].append(
                round((time.perf_counter() - t0) / steps * 1e3, 1))
            print(rnd, arm, json.dumps(res[arm]), flush=True)
    res["bit_identical"] = bool(torch.equal(outs["t128"], outs["persistent_gemm"]))
    return res


def main():
    argv = sys.argv[1:]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "mx_p256_probe.json"))
    result = {"device": torch.cuda.get_device_name(0), "gemm": gemm_section()}
    if "--gemm-only" not in argv:
        result["step"] = step_section()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
