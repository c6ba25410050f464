"""The joint attention with the MX epilogue (bya_attn_fwd_mx) against the joint attention + the standalone 3072-wide quantiser,
on one GPU, one process:
  1. the fused launch next to the pair (bya_attn_fwd into bf16, then bya_quantize_mx) at 17776 rows x 48 heads and at a rank's
     2222 rows x 6 heads against 17776 keys, for both output formats, in interleaved rounds (every arm once per round, every
     round kept); the pair is the path of enable_mx_weights(fuse_attention_quant=False) bit for bit and the reference for time;
  2. the headline 42-layer step (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) of each MX mode with the switch
     off and on, in interleaved rounds of 5 timed steps, and whether the two outputs are bit-identical.
usage: python tools/mx_attn_out_probe.py [out.json] [--attn-only | --step-only] [--modes mxfp6,mxfp8*mxfp4]
(default out: profiles/mx_attn_out_probe.json; a section that is not run keeps what the file already holds, so the two
sections can run as two commands, each under its own time limit)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = [("joint@17776x48", 17776, 17776, 48), ("rank@2222x6", 2222, 17776, 6)]


def time_us(fn, inner=5):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def attn_section(rounds=3):
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    for label, Sq, Skv, H in SHAPES:
        W = H * 64
        q = (torch.randn(1, Sq, W, device=dev, generator=g) * 0.6).to(torch.bfloat16)
        k = (torch.randn(1, Skv, W, device=dev, generator=g) * 0.6).to(torch.bfloat16)
        v = torch.randn(1, Skv, W, device=dev, generator=g).to(torch.bfloat16)
        o = torch.empty(1, Sq, W, dtype=torch.bfloat16, device=dev)
        kw = dict(heads=H, tag="joint", prescaled=True, score_bound=48.0)     # the engine's launch: static bound, stream-K where it pays
        arms, same, keys = {}, {}, {}
        for f in ("mxfp8", "mxfp6"):
            oc = torch.empty(1, Sq, ops.mx_code_bytes(W, f), dtype=torch.uint8, device=dev)
            osc = torch.empty(1, Sq, W // 32, dtype=torch.uint8, device=dev)
            rc, rsc = torch.empty_like(oc), torch.empty_like(osc)

            def pair(f=f, rc=rc, rsc=rsc):
                ops.self_attention(q, k, v, o, **kw)
                ops.quantize_mx(o, f, rc, rsc)

            def fused(f=f, oc=oc, osc=osc):
                ops.self_attention(q, k, v, None, mx_out=(oc, osc, f), **kw)

            pair()
            fused()
            same[f] = bool(torch.equal(oc, rc) and torch.equal(osc, rsc))
            keys[f] = ops.attention_plan_key(ops.attention_plan(
                None, head_dim=64, heads=H, nb1=1, nb2=1, Sq=Sq, Skv=Skv, q_strides=(Sq * W, 0, W), k_strides=(Skv * W, 0, W),
                v_strides=(Skv * W, 0, W), scale=1.0, prescaled=True, score_bound=48.0, mx_out=(oc, osc, f)))
            arms[f] = {"pair": pair, "fused": fused}
        arms["bf16"] = {"attention_only": lambda: ops.self_attention(q, k, v, o, **kw)}
        us = {}
        for _ in range(rounds):                                          # interleaved: every arm once per round
            for name, arm in arms.items():
                for a, fn in arm.items():
                    us.setdefault((name, a), []).append(round(time_us(fn), 1))
        for f in ("mxfp8", "mxfp6"):
            p, fu = us[(f, "pair")], us[(f, "fused")]
            entry = {"Sq": Sq, "Skv": Skv, "heads": H, "plan": keys[f], "bytes_identical": same[f], "pair_us_rounds": p,
                     "attention_bf16_out_us_rounds": us[("bf16", "attention_only")], "fused_us_rounds": fu,
                     "fused_over_pair": round(min(fu) / min(p), 3)}
            out[f"{label}:{f}"] = entry
            print(f"{label}:{f}", json.dumps(entry), flush=True)
        del q, k, v, o, arms
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
                model.enable_mx_weights(f, weight_format=wf or None, fuse_attention_quant=fuse)
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
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "mx_attn_out_probe.json"))
    result = json.load(open(out_path)) if os.path.exists(out_path) else {}
    result["device"] = torch.cuda.get_device_name(0)
    if "--step-only" not in argv:
        result["attention"] = attn_section()
    if "--attn-only" not in argv:
        result["step"] = step_section(modes)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
