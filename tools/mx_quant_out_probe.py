"""ff.net.0 with the quantising epilogue (bya_gemm_mx_quant) against ff.net.0 + the standalone 12288-wide quantiser, on one
GPU, one process:
  1. the fused launch next to the pair (bya_gemm_mx(_mixed) + GELU, then bya_quantize_mx) at 17776 and 2222 rows, for every
     activation / weight format pair, in interleaved rounds (every arm once per round, the best round kept); the pair is the
     path of enable_mx_weights(fuse_activation_quant=False) bit for bit and the reference for time;
  2. the headline 42-layer step (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) of each MX mode with the switch
     on and off, in interleaved rounds of 5 timed steps, and whether the two outputs are bit-identical.
usage: python tools/mx_quant_out_probe.py [out.json] [--gemm-only] [--modes mxfp6,mxfp8*mxfp4]
(default out: profiles/mx_quant_out_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
PAIRS = [("mxfp8", "mxfp8"), ("mxfp8", "mxfp4"), ("mxfp6", "mxfp6"), ("mxfp6", "mxfp4")]
N, K = 12288, 3072                                                     # ff.net.0


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


def gemm_section(rounds=3):
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for M in (17776, 2222):
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
        b = torch.randn(N, device=dev, generator=g).to(torch.bfloat16)
        c = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        wq = {f: ops.quantize_mx(w, f) for f in ("mxfp8", "mxfp6", "mxfp4")}
        arms, same = {}, {}
        for f, wf in PAIRS:
            ac, asc = ops.quantize_mx(a, f)
            wc, wsc = wq[wf]
            oc = torch.empty(M, ops.mx_code_bytes(N, f), dtype=torch.uint8, device=dev)
            osc = torch.empty(M, N // 32, dtype=torch.uint8, device=dev)
            rc, rsc = torch.empty_like(oc), torch.empty_like(osc)
            name = f if wf == f else f + "*" + wf

            def pair(ac=ac, asc=asc, wc=wc, wsc=wsc, f=f, wf=wf, rc=rc, rsc=rsc):
                ops.gemm_mx(ac, asc, wc, wsc, c, f, bias=b, act="gelu_tanh", w_fmt=wf)
                ops.quantize_mx(c, f, rc, rsc)

            def gemm_only(ac=ac, asc=asc, wc=wc, wsc=wsc, f=f, wf=wf):
                ops.gemm_mx(ac, asc, wc, wsc, c, f, bias=b, act="gelu_tanh", w_fmt=wf)

            def fused(ac=ac, asc=asc, wc=wc, wsc=wsc, f=f, wf=wf, oc=oc, osc=osc):
                ops.gemm_mx_quant(ac, asc, wc, wsc, oc, osc, f, w_fmt=wf, out_fmt=f, bias=b, act="gelu_tanh")

            pair()
            fused()
            same[name] = bool(torch.equal(oc, rc) and torch.equal(osc, rsc))
            path = ops.gemm_mx_quant_plan(ac, asc, wc, wsc, oc, osc, f, w_fmt=wf, out_fmt=f, bias=b, act="gelu_tanh")["path"]
            arms[name] = {"pair": pair, "gemm_only": gemm_only, "fused": fused, "path": path}
        us = {name: {"pair": 1e30, "gemm_only": 1e30, "fused": 1e30} for name in arms}
        for _ in range(rounds):                                          # interleaved: every arm once per round
            for name, arm in arms.items():
                for k in ("pair", "gemm_only", "fused"):
                    us[name][k] = min(us[name][k], best_us(arm[k]))
        for name in arms:
            u = us[name]
            entry = {"M": M, "N": N, "K": K, "path": arms[name]["path"], "bytes_identical": same[name],
                     "pair_us": round(u["pair"], 1), "gemm_bf16_out_us": round(u["gemm_only"], 1),
                     "fused_us": round(u["fused"], 1), "fused_over_pair": round(u["fused"] / u["pair"], 3)}
            out[f"ff1@{M}:{name}"] = entry
            print(f"ff1@{M}:{name}", json.dumps(entry), flush=True)
        del a, w, c, wq, arms
        torch.cuda.empty_cache()
    return out


def step_section(modes, steps=5, warmup=2, rounds=3):
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
    for rnd in range(rounds):                                            # rounds x modes x {off, on}, interleaved
        for mode in modes:
            f, _, wf = mode.partition("*")
            for fuse in (False, True):
                model.enable_mx_weights(f, weight_format=wf or None, fuse_activation_quant=fuse)
                for _ in range(warmup):
                    model(return_dict=False, denoise_step=0, **inp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    o = model(return_dict=False, denoise_step=0, **inp)[0]
                torch.cuda.synchronize()
                sec = (time.perf_counter() - t0) / steps
                arm = "fused" if fuse else "two_launches"
                outs[(mode, arm)] = o.clone()
                r = res.setdefault(mode, {}).setdefault(arm, {"ms_per_step_rounds": []})
                r["ms_per_step_rounds"].append(round(sec * 1e3, 1))
                r["ms_per_step"] = min(r["ms_per_step_rounds"])
                print(rnd, mode, arm, json.dumps(r), flush=True)
            res[mode]["bit_identical"] = bool(torch.equal(outs[(mode, "fused")], outs[(mode, "two_launches")]))
    return res


def main():
    argv = sys.argv[1:]
    modes = ["mxfp8", "mxfp8*mxfp4", "mxfp6", "mxfp6*mxfp4"]
    if "--modes" in argv:
        i = argv.index("--modes")
        modes = argv[i + 1].split(",")
        del argv[i:i + 2]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "mx_quant_out_probe.json"))
    result = {"device": torch.cuda.get_device_name(0), "gemm": gemm_section()}
    if "--gemm-only" not in argv:
        result["step"] = step_section(modes)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
