"""What recording the q/k score-bound statistics in the fused q|k|v projection's epilogue costs and buys
(the *_stats entry points; engine switch BYA_QKN_STATS_EPILOGUE), bf16 weights, one GPU, one process.  Per shape three arms,
alternated in one process after warm-up (every arm once per round, device events around ``inner`` launches, the MEDIAN of the
rounds reported and every round kept):
  (a) pair          the projection (bya_gemm_bf16 with n_split) + bya_qknorm_rope with statistics: what a layer that needs the
                    data-dependent bound runs with the switch off;
  (b) fused_stats   bya_gemm_qkv_norm_rope with statistics: the same layer with the switch on;
  (c) fused         bya_gemm_qkv_norm_rope without statistics: what every other layer runs.
(b) - (c) is the price of the statistics, (a) - (b) what the switch buys.  Shapes: 17776 x 3072 -> 9216 dense (one GPU), 8888
rows in the column-block form of 2 ranks, 2222 rows in that of 8 ranks (tables of 64 // W slots, as the engine makes them).
The tables are zeroed once per arm, outside the timed window (a maximum into a raised entry costs what one into a zero does);
the outputs and the tables' maxima of (a) and (b) are compared in the same run.
usage: python tools/qkn_stats_probe.py [out.json] [--rounds N]        (default out: profiles/qkn_stats_probe.json)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from bind_your_avatar_implementation_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
K, WIDTH, TEXT, K_SCALE = 3072, 3072, 226, 0.18
SHAPES = [(17776, 1), (8888, 2), (2222, 8)]                            # (rows of this rank, ranks W: column blocks of WIDTH / W)


def per_launch_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def main():
    argv = sys.argv[1:]
    rounds = 7
    if "--rounds" in argv:
        i = argv.index("--rounds")
        rounds = max(3, int(argv[i + 1]))
        del argv[i:i + 2]
    out_path = next((a for a in argv if not a.startswith("--")), os.path.join(ROOT, "profiles", "qkn_stats_probe.json"))
    g = torch.Generator(device=dev).manual_seed(0)
    w = (torch.randn(3 * WIDTH, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    b = torch.randn(3 * WIDTH, device=dev, generator=g).to(torch.bfloat16)
    qw, qb, kw, kb = ((torch.randn(64, device=dev, generator=g) * 0.3 + (1 if i % 2 == 0 else 0)).to(torch.bfloat16) for i in range(4))
    result = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "shapes": {}}
    for M, W in SHAPES:
        Dl, slots, heads = WIDTH // W, max(1, 64 // W), WIDTH // 64
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        ang = torch.rand(M - TEXT, 64, device=dev, generator=g) * 6.3
        norm = (qw, qb, kw, kb, torch.cos(ang).contiguous(), torch.sin(ang).contiguous())
        two = torch.zeros(3 * W, M, Dl, dtype=torch.bfloat16, device=dev)
        one, plain = torch.zeros_like(two), torch.zeros_like(two)
        split = (Dl, M * Dl)
        t_pair, t_fused = (torch.zeros(slots, 2, heads, dtype=torch.float32, device=dev) for _ in range(2))

        def pair():
            ops.gemm(a, w, two[0], bias=b, split=split)
            ops.qknorm_rope(two[:W], two[W:2 * W], *norm, heads=Dl // 64, text_rows=TEXT, eps=1e-6, k_scale=K_SCALE, stats=t_pair)

        def fused_stats():
            assert ops.gemm_qkv_norm_rope(a, w, one[0], b, split, *norm, TEXT, eps=1e-6, k_scale=K_SCALE, stats=t_fused)

        def fused():
            assert ops.gemm_qkv_norm_rope(a, w, plain[0], b, split, *norm, TEXT, eps=1e-6, k_scale=K_SCALE)

        arms = {"pair": pair, "fused_stats": fused_stats, "fused": fused}
        for fn in arms.values():                                       # warm-up: every arm's kernels loaded, caches in their steady state
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(one, two)) and bool(torch.equal(plain, two))
        same_table = bool(torch.equal(t_pair.amax(0).view(torch.int32), t_fused.amax(0).view(torch.int32)))
        plan = ops.gemm_qkv_norm_rope_plan(a, w, one[0], b, split, *norm, TEXT, eps=1e-6, k_scale=K_SCALE, stats=t_fused)
        inner = 10 if M > 4000 else 30
        us = {k: [] for k in arms}
        for _ in range(rounds):                                        # alternated: every arm once per round
            for k, fn in arms.items():
                us[k].append(round(per_launch_us(fn, inner), 1))
        med = {k: round(statistics.median(v), 1) for k, v in us.items()}
        entry = {"M": M, "N": 3 * WIDTH, "K": K, "ranks": W, "n_split": Dl, "slots": slots, "plan": ops.plan_key(plan),
                 "outputs_bit_identical": same, "table_maxima_bit_identical": same_table,
                 "a_pair_us": med["pair"], "b_fused_stats_us": med["fused_stats"], "c_fused_us": med["fused"],
                 "price_of_statistics_us_b_minus_c": round(med["fused_stats"] - med["fused"], 1),
                 "switch_buys_us_a_minus_b": round(med["pair"] - med["fused_stats"], 1),
                 "rounds_us": us}
        result["shapes"][f"{M}x{3 * WIDTH}x{K}/W{W}"] = entry
        print(json.dumps(entry), flush=True)
        del a, two, one, plain
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
