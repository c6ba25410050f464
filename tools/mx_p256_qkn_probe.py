"""The MX q|k|v projection with the q/k LayerNorm + RoPE in its epilogue on the PERSISTENT 256 x 256 kernel
(bya_gemm_mx_qkv_norm_rope_on, kernel = 1) against what the two switches of enable_mx_weights("mxfp8", ...) ran before they
composed, on one GPU, one process:
  1. q|k|v 9216 x 3072 with bias and 226 text rows, mxfp8, at 17776 and 2222 rows, three arms in interleaved rounds (every arm
     once per round; every round kept):
       (a) tiled_fused:  the fused launch on the 128 x 128 kernel (kernel = 0: persistent_gemm + fuse_qk_norm before),
       (b) p256_pair:    bya_gemm_mx under option mx_kernel = 1, then bya_qknorm_rope (persistent_gemm alone),
       (c) p256_fused:   the fused launch on the persistent kernel (kernel = 1),
     with the bytes of q, k, v compared across the arms in the same run.  (a) and (b) are the references for time;
  2. the headline 42-layer mxfp8 step (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) with persistent_gemm=True
     and fuse_qk_norm off / on, in interleaved rounds of 5 timed steps, and whether the two outputs are bit-identical.
usage: python tools/mx_p256_qkn_probe.py [out.json] [--gemm-only]
(default out: profiles/mx_p256_qkn_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
FMT = "mxfp8"
N, K, WIDTH = 9216, 3072, 3072                                         # attn1.to_q|k|v
TEXT, K_SCALE = 226, 0.18
ARMS = ("tiled_fused", "p256_pair", "p256_fused")


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
    w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    wc, wsc = ops.quantize_mx(w, FMT)
    for M in (17776, 2222):
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        b = torch.randn(N, device=dev, generator=g).to(torch.bfloat16)
        qw, qb, kw, kb = ((torch.randn(64, device=dev, generator=g) * 0.3 + (1 if i % 2 == 0 else 0)).to(torch.bfloat16)
                          for i in range(4))
        ang = torch.rand(M - TEXT, 64, device=dev, generator=g) * 6.3
        norm = (qw, qb, kw, kb, torch.cos(ang).contiguous(), torch.sin(ang).contiguous())
        ac, asc = ops.quantize_mx(a, FMT)
        bufs = {k: torch.full((3, M, WIDTH), float("nan"), dtype=torch.bfloat16, device=dev) for k in ARMS}
        split = (WIDTH, M * WIDTH)

        def fused(buf, kernel):
            assert ops.gemm_mx_qkv_norm_rope(ac, asc, wc, wsc, buf[0], b, split, *norm, TEXT, eps=1e-6, k_scale=K_SCALE, fmt=FMT,
                                             kernel=kernel)

        def p256_pair():
            with ops.options(mx_kernel=1):
                ops.gemm_mx(ac, asc, wc, wsc, bufs["p256_pair"][0], FMT, bias=b, split=split)
            ops.qknorm_rope(bufs["p256_pair"][0], bufs["p256_pair"][1], *norm, heads=WIDTH // 64, text_rows=TEXT, eps=1e-6,
                            k_scale=K_SCALE)

        fns = {"tiled_fused": lambda: fused(bufs["tiled_fused"], 0), "p256_pair": p256_pair,
               "p256_fused": lambda: fused(bufs["p256_fused"], 1)}
        plan = lambda kernel: ops.gemm_mx_qkv_norm_rope_plan(ac, asc, wc, wsc, bufs["p256_fused"][0], b, split, *norm, TEXT,
                                                             eps=1e-6, k_scale=K_SCALE, fmt=FMT, kernel=kernel)["path"]
        with ops.options(mx_kernel=1):
            pair_path = ops.gemm_mx_plan(ac, asc, wc, wsc, bufs["p256_pair"][0], FMT, bias=b, split=split)["path"]
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        i16 = lambda t: t.view(torch.int16)
        same = {k: bool(torch.equal(i16(bufs[k]), i16(bufs["p256_pair"]))) and not bool(torch.isnan(bufs[k]).any())
                for k in ARMS}
        us = {k: [] for k in ARMS}
        for _ in range(rounds):                                          # interleaved: every arm once per round
            for k in ARMS:
                us[k].append(round(best_us(fns[k]), 1))
        entry = {"M": M, "N": N, "K": K, "paths": {"tiled_fused": plan(0), "p256_pair": pair_path, "p256_fused": plan(1)},
                 "bytes_identical_to_p256_pair": same}
        for k in ARMS:
            entry[k + "_us_rounds"] = us[k]
            entry[k + "_us"] = min(us[k])
        for ref in ("tiled_fused", "p256_pair"):
            entry["p256_fused_over_" + ref] = round(min(us["p256_fused"]) / min(us[ref]), 3)
            entry["every_p256_fused_round_beats_every_" + ref + "_round"] = max(us["p256_fused"]) < min(us[ref])
            entry["every_p256_fused_round_loses_to_every_" + ref + "_round"] = min(us["p256_fused"]) > max(us[ref])
        out[f"qkv@{M}"] = entry
        print(f"qkv@{M}", json.dumps(entry), flush=True)
        del a, ac, asc, bufs, fns
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
    for rnd in range(rounds):                                            # rounds x {off, on}, interleaved
        for fuse in (False, True):
            model.enable_mx_weights(FMT, persistent_gemm=True, fuse_qk_norm=fuse)
            for _ in range(warmup):
                model(return_dict=False, denoise_step=0, **inp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                o = model(return_dict=False, denoise_step=0, **inp)[0]
            torch.cuda.synchronize()
            sec = (time.perf_counter() - t0) / steps
            arm = "persistent_fused" if fuse else "persistent_two_launches"
            outs[arm] = o.clone()
            r = res.setdefault(arm, {"ms_per_step_rounds": []})
            r["ms_per_step_rounds"].append(round(sec * 1e3, 1))
            r["ms_per_step"] = min(r["ms_per_step_rounds"])
            print(rnd, arm, json.dumps(r), flush=True)
    res["bit_identical"] = bool(torch.equal(outs["persistent_fused"], outs["persistent_two_launches"]))
    res["every_fused_round_beats_every_two_launch_round"] = \
        max(res["persistent_fused"]["ms_per_step_rounds"]) < min(res["persistent_two_launches"]["ms_per_step_rounds"])
    return res


def main():
    argv = sys.argv[1:]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "mx_p256_qkn_probe.json"))
    result = {"device": torch.cuda.get_device_name(0), "launch": launch_section()}
    if "--gemm-only" not in argv:
        result["step"] = step_section()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
