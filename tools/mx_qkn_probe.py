"""The MX q|k|v projection with the q/k LayerNorm + RoPE in its epilogue (bya_gemm_mx_qkv_norm_rope) against the projection +
the standalone bya_qknorm_rope, on one GPU, one process:
  1. the fused launch next to the pair (bya_gemm_mx(_mixed) with n_split, then bya_qknorm_rope on q and k) at 17776 and 2222
     rows, for every activation / weight format pair, in interleaved rounds (every arm once per round; every round kept, the
     best shown), with the bytes of both compared in the same run; the pair is the path of
     enable_mx_weights(fuse_qk_norm=False) bit for bit and the reference for time;
  2. the headline 42-layer step (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) of each MX mode with the switch
     off and on, in interleaved rounds of 5 timed steps, and whether the two outputs are bit-identical.
usage: python tools/mx_qkn_probe.py [out.json] [--gemm-only] [--modes mxfp6,mxfp8*mxfp4]
(default out: profiles/mx_qkn_probe.json)"""
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
N, K, WIDTH = 9216, 3072, 3072                                         # attn1.to_q|k|v
TEXT, K_SCALE = 226, 0.18


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
    wq = None
    for M in (17776, 2222):
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        if wq is None:
            w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
            wq = {f: ops.quantize_mx(w, f) for f in ("mxfp8", "mxfp6", "mxfp4")}
        b = torch.randn(N, device=dev, generator=g).to(torch.bfloat16)
        qw, qb, kw, kb = ((torch.randn(64, device=dev, generator=g) * 0.3 + (1 if i % 2 == 0 else 0)).to(torch.bfloat16)
                          for i in range(4))
        ang = torch.rand(M - TEXT, 64, device=dev, generator=g) * 6.3
        cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
        two = torch.empty(3, M, WIDTH, dtype=torch.bfloat16, device=dev)
        one = torch.empty_like(two)
        split = (WIDTH, M * WIDTH)
        norm = (qw, qb, kw, kb, cos, sin)
        arms, same = {}, {}
        for f, wf in PAIRS:
            ac, asc = ops.quantize_mx(a, f)
            wc, wsc = wq[wf]
            name = f if wf == f else f + "*" + wf

            def gemm_only(ac=ac, asc=asc, wc=wc, wsc=wsc, f=f, wf=wf):
                ops.gemm_mx(ac, asc, wc, wsc, two[0], f, bias=b, split=split, w_fmt=wf)

            def pair(gemm_only=gemm_only):
                gemm_only()
                ops.qknorm_rope(two[0], two[1], *norm, heads=WIDTH // 64, text_rows=TEXT, eps=1e-6, k_scale=K_SCALE)

            def fused(ac=ac, asc=asc, wc=wc, wsc=wsc, f=f, wf=wf):
                assert ops.gemm_mx_qkv_norm_rope(ac, asc, wc, wsc, one[0], b, split, *norm, TEXT, eps=1e-6, k_scale=K_SCALE,
                                                 fmt=f, w_fmt=wf)

            two.zero_()
            one.fill_(float("nan"))
            pair()
            fused()
            same[name] = bool(torch.equal(one, two))
            path = ops.gemm_mx_qkv_norm_rope_plan(ac, asc, wc, wsc, one[0], b, split, *norm, TEXT, eps=1e-6, k_scale=K_SCALE,
                                                  fmt=f, w_fmt=wf)["path"]
            arms[name] = {"pair": pair, "gemm_only": gemm_only, "fused": fused, "path": path}
        us = {name: {"pair": [], "gemm_only": [], "fused": []} for name in arms}
        for _ in range(rounds):                                          # interleaved: every arm once per round
            for name, arm in arms.items():
                for k in ("pair", "gemm_only", "fused"):
                    us[name][k].append(round(best_us(arm[k]), 1))
        for name in arms:
            u = us[name]
            entry = {"M": M, "N": N, "K": K, "path": arms[name]["path"], "bytes_identical": same[name],
                     "pair_us_rounds": u["pair"], "gemm_alone_us_rounds": u["gemm_only"], "fused_us_rounds": u["fused"],
                     "pair_us": min(u["pair"]), "gemm_alone_us": min(u["gemm_only"]), "fused_us": min(u["fused"]),
                     "fused_over_pair": round(min(u["fused"]) / min(u["pair"]), 3),
                     "every_fused_round_beats_every_pair_round": max(u["fused"]) < min(u["pair"])}
            out[f"qkv@{M}:{name}"] = entry
            print(f"qkv@{M}:{name}", json.dumps(entry), flush=True)
        del a, arms, two, one
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
                model.enable_mx_weights(f, weight_format=wf or None, fuse_qk_norm=fuse)
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
    for r in res.values():
        r["every_fused_round_beats_every_two_launch_round"] = \
            max(r["fused"]["ms_per_step_rounds"]) < min(r["two_launches"]["ms_per_step_rounds"])
    return res


def main():
    argv = sys.argv[1:]
    modes = ["mxfp8", "mxfp8*mxfp4", "mxfp6", "mxfp6*mxfp4"]
    if "--modes" in argv:
        i = argv.index("--modes")
        modes = argv[i + 1].split(",")
        del argv[i:i + 2]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "mx_qkn_probe.json"))
    result = {"device": torch.cuda.get_device_name(0), "gemm": gemm_section()}
    if "--gemm-only" not in argv:
        result["step"] = step_section(modes)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
