"""The two cross-attention output projections as MX Linears, fed by the kv-mix epilogue that writes MX codes
(bya_attn_kv_mix_mx), on one GPU, one process:
  1. per to_out shape (perceiver: 16 heads of 128 -> 3072 x 2048; audio: 48 heads of 64 -> 3072 x 3072) at 17550 rows (one
     GPU) and 2194 rows (a rank of 8), for both formats, in interleaved rounds (every arm once per round, every round kept):
       bf16:  kv-mix (bf16 z) + the bf16 GEMM                      -- the step as it stands
       pair:  kv-mix (bf16 z) + bya_quantize_mx + the MX GEMM      -- fuse_cross_attention_quant=False, the reference for time
       fused: kv-mix writing MX codes + the MX GEMM
     and the producer launches alone (kv-mix bf16, kv-mix + quantiser, fused kv-mix); the bytes of pair and fused are compared
     in the same run;
  2. the headline 42-layer step (49 x 480 x 720 -> 13 x 60 x 90 latents, 2 identities, eager) of each MX mode with the default
     four Linears and with ("po", "ao") added, in interleaved rounds of timed steps, and each arm's 42-layer drift from the
     bf16 engine of the same run.
usage: python tools/mx_cross_out_probe.py [out.json] [--kernel-only | --step-only] [--modes mxfp6,mxfp8,mxfp8+p,mxfp6+p]
(default out: profiles/mx_cross_out_probe.json; a section that is not run keeps what the file already holds; "+p" = the
mode's persistent-GEMM switch)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
BF = torch.bfloat16
# label, head_dim, heads, n_id, (n_grp, Sq) at 17550 rows, at 2194 rows (one launch over the rank's rows), N of to_out, audio?
SHAPES = [("perceiver.to_out", 128, 16, 2, (1, 17550), (1, 2194), 3072, False),
          ("audio.to_out", 64, 48, 2, (13, 1350), (1, 2194), 3072, True)]
SIX = ("qkv", "out", "ff1", "ff2", "po", "ao")


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


def kernel_section(rounds=3):
    out = {}
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    for label, D, H, n_id, big, small, N, audio in SHAPES:
        E = H * D
        for grp, Sq in (big, small):
            M = grp * Sq
            q, k, v = rn(grp, Sq, E).to(BF), rn(n_id, grp, 32, E).to(BF), rn(n_id, grp, 32, E).to(BF)
            r = torch.sigmoid(rn(M, n_id)).to(BF)
            af = torch.roll(torch.eye(n_id), 1, dims=1).to(BF).to(dev) if audio else None
            w = (rn(N, E) * E ** -0.5).to(BF)
            bias = rn(N).to(BF) if audio else None
            x = rn(M, N).to(BF)
            ws = torch.empty(M, dtype=torch.float32, device=dev)
            z, y = torch.empty(grp, Sq, E, dtype=BF, device=dev), torch.empty(M, N, dtype=BF, device=dev)
            kw = dict(head_dim=D, heads=H, n_id=n_id, n_grp=grp, Sq=Sq, Skv=32, q_strides=(Sq * E, E),
                      k_strides=(grp * 32 * E, 32 * E, E), v_strides=(grp * 32 * E, 32 * E, E), scale=D ** -0.5)
            epi = dict(bias=bias, res=x, bias_rowscale=ws) if audio else dict(res=x, alpha=0.5)

            def mix_bf16():
                ops.attn_kv_mix(q, k, v, r, af, z, ws, z_strides=(Sq * E, E), **kw)

            arms = {("bf16", "producer"): mix_bf16,
                    ("bf16", "chain"): lambda: (mix_bf16(), ops.gemm(z.view(M, E), w, y, **epi)),
                    ("bf16", "gemm"): lambda: ops.gemm(z.view(M, E), w, y, **epi)}
            same = {}
            for f in ("mxfp8", "mxfp6"):
                wc, wsc = ops.quantize_mx(w, f)
                pc, ps = ops.quantize_mx(z.view(M, E), f)
                fc, fs = torch.empty_like(pc), torch.empty_like(ps)

                def pair_prod(f=f, pc=pc, ps=ps):
                    mix_bf16()
                    ops.quantize_mx(z.view(M, E), f, pc, ps)

                def fused_prod(f=f, fc=fc, fs=fs):
                    ops.attn_kv_mix(q, k, v, r, af, None, ws, mx_out=(fc, fs, f), **kw)

                def mx_gemm(c, s, f=f, wc=wc, wsc=wsc):
                    ops.gemm_mx(c, s, wc, wsc, y, f, **epi)

                pair_prod()
                fused_prod()
                same[f] = bool(torch.equal(pc, fc) and torch.equal(ps, fs))
                arms[(f, "pair_producer")] = pair_prod
                arms[(f, "fused_producer")] = fused_prod
                arms[(f, "gemm")] = lambda pc=pc, ps=ps, mx_gemm=mx_gemm: mx_gemm(pc, ps)
                arms[(f, "pair_chain")] = lambda pair_prod=pair_prod, pc=pc, ps=ps, mx_gemm=mx_gemm: (pair_prod(), mx_gemm(pc, ps))
                arms[(f, "fused_chain")] = lambda fused_prod=fused_prod, fc=fc, fs=fs, mx_gemm=mx_gemm: (fused_prod(), mx_gemm(fc, fs))
            us = {}
            for _ in range(rounds):                                      # interleaved: every arm once per round
                for key, fn in arms.items():
                    us.setdefault(key, []).append(round(time_us(fn), 1))
            for f in ("mxfp8", "mxfp6"):
                entry = {"rows": M, "n_grp": grp, "Sq": Sq, "heads": H, "head_dim": D, "N": N, "K": E, "bytes_identical": same[f],
                         "kv_mix_bf16_us_rounds": us[("bf16", "producer")], "pair_producer_us_rounds": us[(f, "pair_producer")],
                         "fused_producer_us_rounds": us[(f, "fused_producer")],
                         "gemm_bf16_us_rounds": us[("bf16", "gemm")], "gemm_mx_us_rounds": us[(f, "gemm")],
                         "bf16_chain_us_rounds": us[("bf16", "chain")], "pair_chain_us_rounds": us[(f, "pair_chain")],
                         "fused_chain_us_rounds": us[(f, "fused_chain")],
                         "fused_over_pair_producer": round(min(us[(f, "fused_producer")]) / min(us[(f, "pair_producer")]), 3),
                         "fused_chain_over_bf16_chain": round(min(us[(f, "fused_chain")]) / min(us[("bf16", "chain")]), 3)}
                out[f"{label}@{M}:{f}"] = entry
                print(f"{label}@{M}:{f}", json.dumps(entry), flush=True)
            del arms, q, k, v, z, y, x, w
            torch.cuda.empty_cache()
    return out


def step_section(modes, steps=3, warmup=2, rounds=3):
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    kw = dict(num_attention_heads=48, attention_head_dim=64, in_channels=48, out_channels=16, num_layers=42,
              use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True, is_train_face=True,
              cross_attn_interval=2, local_face_scale=1.0, is_train_audio=True, audio_attn_interval=1,
              sample_height=60, sample_width=90, sample_frames=49)
    model = BindyouravatarTransformer3DModel(**kw, device=dev).init_synthetic(seed=0, fast=True)
    d = synth_inputs(batch=1, frames=13, height=60, width=90, n_id=2, seed=0, device="cpu")
    inp = {k: (v.to(dev, BF) if torch.is_tensor(v) and v.is_floating_point() else
               (v.to(dev) if torch.is_tensor(v) else v)) for k, v in d.items()}
    inp["image_rotary_emb"] = tuple(t.to(dev, torch.float32) for t in d["image_rotary_emb"])
    inp["id_cond"] = [t.to(dev, BF) for t in d["id_cond"]]
    inp["id_vit_hidden"] = [[t.to(dev, BF) for t in l] for l in d["id_vit_hidden"]]

    def timed():
        for _ in range(warmup):
            model(return_dict=False, denoise_step=0, **inp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            o = model(return_dict=False, denoise_step=0, **inp)[0]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, o.float()

    rel = lambda a, b: float((a - b).norm() / b.norm())
    res = {"bf16": {"ms_per_step_rounds": []}}
    ref = None
    for rnd in range(rounds):                                            # rounds x (bf16, modes x {four, six}), interleaved
        model.enable_mx_weights(enabled=False)
        ms, o = timed()
        ref = o if ref is None else ref
        res["bf16"]["ms_per_step_rounds"].append(round(ms, 1))
        for mode in modes:
            f, _, p = mode.partition("+")
            sw = {} if not p else ({"persistent_gemm": True} if f == "mxfp8" else {"persistent_gemm_mxfp6": True})
            for arm, lin in (("default_four", None), ("with_po_ao", SIX)):
                model.enable_mx_weights(f, linears=lin, **sw)
                ms, o = timed()
                r = res.setdefault(mode, {}).setdefault(arm, {"ms_per_step_rounds": []})
                r["ms_per_step_rounds"].append(round(ms, 1))
                r["ms_per_step"] = min(r["ms_per_step_rounds"])
                r["drift_vs_bf16_engine"] = round(rel(o, ref), 5)
                print(rnd, mode, arm, json.dumps(r), flush=True)
    res["bf16"]["ms_per_step"] = min(res["bf16"]["ms_per_step_rounds"])
    return res


def main():
    argv = sys.argv[1:]
    modes = ["mxfp6", "mxfp8", "mxfp8+p", "mxfp6+p"]
    if "--modes" in argv:
        i = argv.index("--modes")
        modes = argv[i + 1].split(",")
        del argv[i:i + 2]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "mx_cross_out_probe.json"))
    result = json.load(open(out_path)) if os.path.exists(out_path) else {}
    result["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)

    def save():
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)

    if "--step-only" not in argv:
        result["kernels"] = kernel_section()
        save()
    if "--kernel-only" not in argv:
        result["step"] = step_section(modes)
        save()


if __name__ == "__main__":
    main()
