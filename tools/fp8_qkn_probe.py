"""The fp8 q|k|v projection with the q/k LayerNorm + RoPE in its epilogue (bya_gemm_fp8_qkv_norm_rope) against the projection +
the standalone bya_qknorm_rope, on one GPU, one process:
  1. the fused launch next to the pair (bya_gemm_fp8 with n_split, then bya_qknorm_rope on q and k) at 17776 x 9216 x 3072 and
     2222 x 9216 x 3072, and at 2222 x 6144 x 3072 for q | k alone, in interleaved rounds (every arm once per round; every
     round kept, the best shown), device events, warmed up, with the bytes of both compared in the same run and the plan's
     path per arm; the pair is the path of enable_fp8_weights(fuse_qk_norm=False) bit for bit and the reference for time;
  2. the headline 42-layer step (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) with fp8 weights and the switch
     off and on, in interleaved rounds of 5 timed steps, and whether the two outputs are bit-identical.
usage: python tools/fp8_qkn_probe.py [out.json] [--gemm-only] [--rounds N]
(default out: profiles/fp8_qkn_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
K, WIDTH = 3072, 3072                                                  # attn1.to_q|k|v
TEXT, K_SCALE = 226, 0.18
SHAPES = [(17776, 3), (2222, 3), (2222, 2)]                            # (rows, tensors): q | k | v, or q | k alone


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
    w = (torch.randn(3 * WIDTH, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    w8_all, sw_all = ops.quantize_rows_fp8(w)
    b_all = torch.randn(3 * WIDTH, device=dev, generator=g).to(torch.bfloat16)
    qw, qb, kw, kb = ((torch.randn(64, device=dev, generator=g) * 0.3 + (1 if i % 2 == 0 else 0)).to(torch.bfloat16)
                      for i in range(4))
    for M, tensors in SHAPES:
        N = tensors * WIDTH
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        a8, sa = ops.quantize_rows_fp8(a)
        w8, sw, b = w8_all[:N].contiguous(), sw_all[:N].contiguous(), b_all[:N].contiguous()
        ang = torch.rand(M - TEXT, 64, device=dev, generator=g) * 6.3
        cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
        two = torch.empty(tensors, M, WIDTH, dtype=torch.bfloat16, device=dev)
        one = torch.empty_like(two)
        split = (WIDTH, M * WIDTH)
        norm = (qw, qb, kw, kb, cos, sin)

        def gemm_only():
            ops.gemm_fp8(a8, sa, w8, sw, two[0], bias=b, split=split)

        def pair():
            gemm_only()
            ops.qknorm_rope(two[0], two[1], *norm, heads=WIDTH // 64, text_rows=TEXT, eps=1e-6, k_scale=K_SCALE)

        def fused():
            assert ops.gemm_fp8_qkv_norm_rope(a8, sa, w8, sw, one[0], b, split, *norm, TEXT, eps=1e-6, k_scale=K_SCALE,
                                              tensors=tensors)

        two.zero_()
        one.fill_(float("nan"))
        pair()
        fused()
        torch.cuda.synchronize()
        same = bool(torch.equal(one, two))
        paths = {"pair": ops.gemm_fp8_plan(a8, sa, w8, sw, two[0], bias=b, split=split)["path"],
                 "fused": ops.gemm_fp8_qkv_norm_rope_plan(a8, sa, w8, sw, one[0], b, split, *norm, TEXT, eps=1e-6,
                                                          k_scale=K_SCALE, tensors=tensors)["path"]}
        arms = {"pair": pair, "gemm_only": gemm_only, "fused": fused}
        u = {k: [] for k in arms}
        for _ in range(rounds):                                          # interleaved: every arm once per round
            for k, fn in arms.items():
                u[k].append(round(best_us(fn), 1))
        entry = {"M": M, "N": N, "K": K, "tensors": tensors, "path": paths, "bytes_identical": same,
                 "pair_us_rounds": u["pair"], "gemm_alone_us_rounds": u["gemm_only"], "fused_us_rounds": u["fused"],
                 "pair_us": min(u["pair"]), "gemm_alone_us": min(u["gemm_only"]), "fused_us": min(u["fused"]),
                 "fused_over_pair": round(min(u["fused"]) / min(u["pair"]), 3),
                 "every_fused_round_beats_every_pair_round": max(u["fused"]) < min(u["pair"])}
        name = f"{'qkv' if tensors == 3 else 'qk'}@{M}"
        out[name] = entry
        print(name, json.dumps(entry), flush=True)
        del a, a8, two, one
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
            model.enable_fp8_weights(fuse_qk_norm=fuse)
            for _ in range(warmup):
                model(return_dict=False, denoise_step=0, **inp)
            torch.cuda.synchronize()
            assert model._engine.fp8_fuse_qk_norm is fuse
            t0 = time.perf_counter()
            for _ in range(steps):
                o = model(return_dict=False, denoise_step=0, **inp)[0]
            torch.cuda.synchronize()
            sec = (time.perf_counter() - t0) / steps
            arm = "fused" if fuse else "two_launches"
            outs[arm] = o.clone()
            r = res.setdefault(arm, {"ms_per_step_rounds": []})
            r["ms_per_step_rounds"].append(round(sec * 1e3, 1))
            r["ms_per_step"] = min(r["ms_per_step_rounds"])
            print(rnd, arm, json.dumps(r), flush=True)
        res["bit_identical"] = bool(torch.equal(outs["fused"], outs["two_launches"]))
    # (what the comparison rests on: layers that ask for the norm statistics keep the two launches under either switch)
    res["layers_with_norm_statistics"] = sum(1 for b in model._engine.score_bound
                                             if b > ops.ATTN_BOUND_LIMIT and model._engine.device_bound)
    res["every_fused_round_beats_every_two_launch_round"] = \
        max(res["fused"]["ms_per_step_rounds"]) < min(res["two_launches"]["ms_per_step_rounds"])
    return res


def main():
    argv = sys.argv[1:]
    rounds = 3
    if "--rounds" in argv:
        i = argv.index("--rounds")
        rounds = max(3, int(argv[i + 1]))
        del argv[i:i + 2]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "fp8_qkn_probe.json"))
    result = {"device": torch.cuda.get_device_name(0), "gemm": gemm_section(rounds)}
    if "--gemm-only" not in argv:
        result["step"] = step_section(rounds=rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
