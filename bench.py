#!/usr/bin/env python3
"""Headline benchmark: denoise-steps/sec of the Bind-Your-Avatar hot path on MI355X.

A "step" = one ``BindyouravatarTransformer3DModel.forward`` (reference models/transformer.py:615-964) on
synthetic inputs of BASELINE.json configs[1]: 49 frames x 480 x 720 (13 x 30 x 45 latent tokens + 226 text
tokens), 2 talking characters (2 ID embeddings + 2 audio streams), bf16, batch 1, all 42 DiT layers, 21 face
routing layers, 42 audio layers, random-init weights of the real architecture (8.6 B parameters).
Inputs are resident in HBM when the timed region starts; step-invariant conditioning (face extractor, audio
projector) is RECOMPUTED every step exactly like the reference does (no cached outputs).

  python bench.py --gpus N --steps K --warmup W            (N > 1: launched through torch.distributed.run)

N > 1 shards the token axis of the same step across ranks (sequence parallel: head-parallel all-to-all around the joint
attention, sharded Embedding Router): total work is fixed => "scaling": "strong".  Before anything is timed every rank runs
the UNSHARDED step once on its own GPU and the sharded step must reproduce it -- bit for bit with the two summation-order
switches off (library options gemm_splitk = 0, attn_streamk = 0), to bf16 noise in the default mode -- after enough warm-up steps that
every receive buffer has been re-used; a transport that fails moves ALL ranks one rung down the ladder
p2p (coarse receive buffers) -> p2p-fine (fine-grained) -> torch.distributed, and the line says which rung ran.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline (``value``,
``ms_per_step``, ...).  ``--full`` adds what is measured or checked beside it: the board calibration, ``roofline`` for
the dominant kernel BY TIME (the GEMM kernel: half of the step; measured live with HIP events on the launch stream in a
second pass), ``attn_roofline`` for the joint attention beside it, the fp8-weights and large-q/k-gain variants,
``cpu_baseline`` (the CPU oracle timed on this box's host cores, rank 0, N = 1), and for N > 1 the CFG pair (N >= 4) and
the P2P exchange probe.  The ``--no-*`` switches leave single pieces of that out.

``--dump-outputs DIR`` writes what the last timed step returned (the noise prediction) as ``DIR/noise_pred.npy`` in fp32;
weights and inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

# timer buckets (ops._begin names) of the Embedding Router's launches
ROUTER_TIMERS = ("bya_rowgemm512", "bya_router_group_attn", "bya_router_group_attn_out", "bya_router_mlp_fused", "bya_attn_tiny",
                 "bya_attn_fwd:other", "bya_router_scores", "bya_router_head")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MODEL_KW = dict(num_attention_heads=48, attention_head_dim=64, in_channels=48, out_channels=16, num_layers=42,
                use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True,
                is_train_face=True, cross_attn_interval=2, local_face_scale=1.0, is_train_audio=True,
                audio_attn_interval=1)
TFLOP_PER_STEP = 443.9          # algorithmic, BASELINE.md section 2 (B = 1)
ATTN_TFLOP_PER_LAUNCH = 4 * 17776 ** 2 * 3072 / 1e12     # joint self-attention, one layer, B = 1
PEAK_BF16_TFLOPS = 2500.0       # dense bf16 MFMA peak, MI355X_MICROARCH.md "Chip-level parameters"


CONFIG0_TFLOP = 12.1            # one DiT block + every injection at 17776 tokens
BLOCK_TFLOP = 7.9               # one CogVideoXBlock at 17776 tokens


def cpu_baseline(threads, config0=False):
    """Bounded CPU sample on this box's host cores (baseline only -- never the thing measured).

    Default (about 30 s): the oracle's CogVideoXBlock (7.9 of the 443.9 TFLOP of a step) at 17776 tokens in bf16, one
    warm-up + one timed forward, extrapolated linearly by FLOPs.
    ``config0`` (--cpu-baseline-config0; SURVEY.md section 8d form, minutes: one bf16 forward took 133 s on the 256-core
    host of the round-2 GPU box, profiles/README.md): BASELINE configs[0] -- ONE DiT block with every injection (face
    perceiver + Embedding Router + masked combine, audio cross-attention + combine, LocalFacialExtractor, audio
    projector, patch embed / head), 1 face + 1 audio stream -- through the oracle's restatement of transformer.forward,
    bf16 warm-up + up to 3 timed and one fp32 forward."""
    torch.set_num_threads(threads)
    if not config0:
        from oracle.model import CogVideoXBlock
        from oracle.layers import get_3d_rotary_pos_embed
        with torch.no_grad():
            blk = CogVideoXBlock(dim=3072, num_attention_heads=48, attention_head_dim=64, time_embed_dim=512,
                                 attention_bias=True).to(torch.bfloat16).eval()
            hid = torch.randn(1, 17550, 3072).to(torch.bfloat16)
            enc = torch.randn(1, 226, 3072).to(torch.bfloat16)
            temb = torch.randn(1, 512).to(torch.bfloat16)
            rope = get_3d_rotary_pos_embed(64, ((0, 0), (30, 45)), (30, 45), 13)
            ts = []
            for _ in range(2):
                t0 = time.time()
                blk(hid, enc, temb, rope)
                ts.append(time.time() - t0)
        dt = ts[1]
        return {"value": 1.0 / (dt * TFLOP_PER_STEP / BLOCK_TFLOP), "unit": "steps/s", "cores": threads, "kind": "port",
                "block_forward_s": {"bf16_warmup": round(ts[0], 2), "bf16": round(ts[1], 2)},
                "sample": f"1 CogVideoXBlock forward ({BLOCK_TFLOP} of {TFLOP_PER_STEP} TFLOP/step) at 17776 tokens, bf16, "
                          f"oracle restatement on torch CPU, {dt:.1f} s after one warm-up; extrapolated linearly by FLOPs "
                          f"to a full step (the config-0 form with every injection: --cpu-baseline-config0)"}
    from oracle.model import OracleTransformer
    from bind_your_avatar_implementation_amd.synth import synth_inputs
    kw = dict(MODEL_KW, num_layers=1, cross_attn_interval=1)
    with torch.device("meta"):
        orc = OracleTransformer(**kw)
    orc = orc.to_empty(device="cpu")
    with torch.no_grad():
        for name, t in orc.state_dict().items():
            if t.is_floating_point():
                if t.dim() == 1 and name.endswith("weight"):
                    t.fill_(1.0)
                elif t.dim() == 1:
                    t.zero_()
                else:
                    t.normal_(0.0, 0.02)
    orc.eval()
    inp = synth_inputs(batch=1, seed=0)
    inp["id_cond"][1].zero_()
    for t in inp["id_vit_hidden"][1]:
        t.zero_()
    inp["audio_embeds"][:, 1] = 0                    # 1 face + 1 audio stream (second stream zero-filled)

    def cast(dt):
        out = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
        out["id_cond"] = [t.to(dt) for t in inp["id_cond"]]
        out["id_vit_hidden"] = [[t.to(dt) for t in l] for l in inp["id_vit_hidden"]]
        out["image_rotary_emb"] = inp["image_rotary_emb"]
        return out

    times = {"bf16": [], "fp32": []}
    with torch.no_grad():
        o16, i16 = orc.to(torch.bfloat16), cast(torch.bfloat16)
        t0 = time.time()
        o16(**i16)                                    # warm-up (thread pools, oneDNN primitive caches)
        warm = time.time() - t0
        for _ in range(3):
            t0 = time.time()
            o16(**i16)
            times["bf16"].append(time.time() - t0)
        o32, i32 = orc.float(), cast(torch.float32)
        t0 = time.time()
        o32(**i32)
        times["fp32"].append(time.time() - t0)
    dt = sorted(times["bf16"])[len(times["bf16"]) // 2]
    return {"value": 1.0 / (dt * TFLOP_PER_STEP / CONFIG0_TFLOP), "unit": "steps/s", "cores": threads, "kind": "port",
            "config0_forward_s": {"bf16_warmup": round(warm, 2), "bf16": [round(t, 2) for t in times["bf16"]],
                                  "fp32": [round(t, 2) for t in times["fp32"]]},
            "sample": f"BASELINE configs[0]: 1 DiT block + all injections (1 face + 1 audio stream), 17776 tokens, oracle "
                      f"restatement on torch CPU, bf16 median {dt:.1f} s over 3 timed runs after a warm-up "
                      f"({CONFIG0_TFLOP} of {TFLOP_PER_STEP} TFLOP/step); value = extrapolated linearly by FLOPs"}


def committed_config0_baseline():
    """The SURVEY 8(d) form of the CPU baseline (BASELINE configs[0]: one DiT block with every injection through the oracle's
    transformer.forward, minutes of CPU) is not re-run by the default invocation; the newest committed run of
    ``bench.py --cpu-baseline-config0`` on a GPU box's host (profiles/r*_cpu_baseline_config0.json) is quoted beside the
    bounded sample instead."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "history", "r*_cpu_baseline_config0.json")) +
                   glob.glob(os.path.join(ROOT, "profiles", "r*_cpu_baseline_config0.json")))
    if not files:
        return None
    try:
        with open(files[-1]) as f:
            d = json.load(f)
        cb = d.get("cpu_baseline", d)
        return {"file": os.path.relpath(files[-1], ROOT), "value": cb["value"], "unit": cb["unit"], "cores": cb["cores"],
                "config0_forward_s": cb.get("config0_forward_s"), "sample": cb.get("sample")}
    except Exception:                                        # noqa: BLE001
        return None


def pmc_traffic(world, *kernels):
    """Bytes per launch at the L2's memory side for the first of ``kernels`` found in the newest committed rocprofv3
    PMC summary (profiles/r*_pmc_traffic.json: 2 x FETCH_SIZE + WRITE_SIZE in separate passes, MI355X_MICROARCH.md section
    HBM); single-GPU only.  Collected by tools/run_pmc.sh, not inside this run."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "history", "r*_pmc_traffic.json")) +
                   glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    if world != 1 or not files:
        return None
    with open(files[-1]) as f:
        d = json.load(f)
    for k in kernels:
        if k in d:
            return d[k]["hbm_bytes_per_launch"]
    return None


DUMP_BYTES = 64 << 20


def dump_outputs(directory, arrays):
    """``arrays`` (name -> tensor) as ``directory/<name>.npy`` in fp32.  Above DUMP_BYTES in all, each array is replaced by
    the same seeded sample of its flattened elements (sorted indices from a fixed generator) in every run."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    share = DUMP_BYTES // (4 * len(arrays))
    for name, t in arrays.items():
        a = t.detach().float().cpu()
        if a.numel() > share:
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:share].sort().values
            a = a.reshape(-1)[idx]
        np.save(os.path.join(directory, f"{name}.npy"), a.numpy())


def self_launch(n):
    """One rank per GPU through ``python -m torch.distributed.run`` (the command shape the driver itself uses), rendezvous
    on 127.0.0.1 and a free port; every argument of this invocation is passed on.  Returns the child's exit code."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=42, help="debug only: anything but 42 is not the headline config")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-config0", action="store_true",
                    help="time the config-0 form (1 block + every injection) instead of the block alone: minutes of CPU")
    ap.add_argument("--no-kernel-timers", action="store_true")
    ap.add_argument("--graph", action="store_true", help="replay the step from a captured hipGraph (N = 1; N > 1 on the P2P rungs does by default)")
    ap.add_argument("--eager", action="store_true", help="N > 1: keep the timed steps eager (default on the P2P rungs: hipGraph replay)")
    ap.add_argument("--no-calibration", action="store_true", help="skip the board calibration (bare-MFMA loop, ~0.7 s) before the timed region")
    ap.add_argument("--no-cfg-pair-variant", action="store_true",
                    help="N >= 4: skip the extra measurement of the CFG pair (batch 2 on 2 x N/2 ranks) beside the headline")
    ap.add_argument("--latent-hw", type=int, nargs=2, default=[60, 90], metavar=("H", "W"),
                    help="latent height / width; anything but 60 90 (= 480x720) is not the headline config")
    ap.add_argument("--batch", type=int, default=1, help="2 = the CFG pair of BASELINE config 3 (not the headline)")
    ap.add_argument("--latent-frames", type=int, default=13, help="25 = the 97-frame clip of BASELINE config 4 (not the headline)")
    ap.add_argument("--identities", type=int, default=2, help="3 = BASELINE config 4's character count (not the headline)")
    ap.add_argument("--no-fp8-variant", action="store_true", help="skip the extra fp8-weights measurement beside the headline")
    ap.add_argument("--launch-check", action="store_true",
                    help="only prove that the N ranks start and meet (gloo all-reduce, no GPU): CPU test of the self-launch")
    ap.add_argument("--qk-gain", type=float, default=1.0,
                    help="multiply every attn1.norm_q / norm_k weight by G (synthetic weights have gain 1): above ~2.7 the worst-case "
                         "score bound of a layer exceeds 90 and the joint attention takes its bound from the data (not the headline)")
    ap.add_argument("--no-qk-gain-variant", action="store_true", help="skip the extra large-q/k-gain measurement beside the headline")
    ap.add_argument("--fp8-weights", action="store_true",
                    help="BASELINE config 5's weight format: e4m3 operands in the DiT Linears (not the headline, which is bf16)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what stands beside the headline: board calibration, per-kernel event pass and "
                         "rooflines, fp8-weights and large-q/k-gain variants, CPU baseline, N >= 4 CFG pair, P2P exchange probe")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's output as DIR/noise_pred.npy (fp32; a seeded sample above 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.cpu_baseline_config0 and not args.full:
        ap.error("--cpu-baseline-config0 is part of --full")
    if not args.full:
        # a plain run does only what its headline figure needs
        args.no_calibration = args.no_kernel_timers = args.no_fp8_variant = args.no_qk_gain_variant = True
        args.no_cpu_baseline = args.no_cfg_pair_variant = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves, as a CHILD process (this process has
        # not touched the GPU yet and never will: it only relays the child's output and exit code).
        sys.exit(self_launch(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node must equal --gpus")
    if args.launch_check:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([rank + 1.0])
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"launch_check": world, "rank_sum": t.item()}), flush=True)
        dist.destroy_process_group()
        return
    # BYA_BENCH_SHARE_GPU=1 (test hook, tests/test_forward_gpu.py): all ranks on GPU 0 with a gloo process group -- how the
    # builder's one-GPU box exercises the N > 1 code path of this file; never a measurement
    share = os.environ.get("BYA_BENCH_SHARE_GPU") == "1"
    if share:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
    from bind_your_avatar_implementation_amd.synth import synth_inputs

    lh, lw = args.latent_hw
    lt, nid = args.latent_frames, args.identities
    kw = dict(MODEL_KW, num_layers=args.layers, sample_height=lh, sample_width=lw, sample_frames=(lt - 1) * 4 + 1)
    model = BindyouravatarTransformer3DModel(**kw, device=dev).init_synthetic(seed=0, fast=True)
    if args.fp8_weights:
        model.enable_fp8_weights()

    def scale_qk_gains(g):
        with torch.no_grad():
            for blk in model.transformer_blocks:
                blk.attn1.norm_q.weight.mul_(g)
                blk.attn1.norm_k.weight.mul_(g)
    if args.qk_gain != 1.0:
        scale_qk_gains(args.qk_gain)

    def make_inputs(batch):
        d = synth_inputs(batch=batch, frames=lt, height=lh, width=lw, n_id=nid, seed=0, device="cpu", uncond_first=batch == 2)
        d = {k: (v.to(dev, torch.bfloat16) if torch.is_tensor(v) and v.is_floating_point() else
                 (v.to(dev) if torch.is_tensor(v) else v)) for k, v in d.items()}
        d["image_rotary_emb"] = tuple(t.to(dev, torch.float32) for t in d["image_rotary_emb"])
        d["id_cond"] = [t.to(dev, torch.bfloat16) for t in d["id_cond"]]
        d["id_vit_hidden"] = [[t.to(dev, torch.bfloat16) for t in l] for l in d["id_vit_hidden"]]
        return d

    inp = make_inputs(args.batch)

    def step():
        return model(return_dict=False, denoise_step=0, **inp)[0]

    def timed_alone(fn, n):
        """seconds per call on THIS rank's GPU, no barrier (the unsharded references of an N > 1 run); -> (s, last output)"""
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            o = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, o

    # ---- what THIS board sustains (round 6): a loop of nothing but the GEMM's MFMA on gaussian operands, ~0.7 s, before any
    # warm-up.  The pool's boxes differ by +-3 % in the clock they hold under load; `frac_of_board` reads the same kernels
    # against the board they ran on, `frac` (the headline) against the spec peak.
    calibration = None if args.no_calibration else ops.board_calibration(dev)

    # strict summation order = options gemm_splitk = 0, attn_streamk = 0 of the library (ops.strict_summation)
    if share and world > 1:
        # Split-K tails and the stream-K attention hand partial sums between workgroups of ONE launch and count on the whole
        # grid being resident (one workgroup per CU on a GPU the process owns).  Processes that time-slice one GPU break
        # that: two half-resident grids wait for each other until the bounded hand-off gives up (counted, and fatal below).
        # The one-GPU rehearsal therefore runs everything in the unsplit mode; what it rehearses is the exchange code.
        ops.set_option("gemm_splitk", 0)
        ops.set_option("attn_streamk", 0)
    strict_mode = ops.strict_summation

    transport_note, validation = None, None
    if world > 1:
        os.environ.setdefault("BYA_SP_VERIFY", "1")     # every sharded step trades a checksum of its gathered prediction (engine.verify_exchanges)
        from bind_your_avatar_implementation_amd.parallel import TRANSPORTS, shard_cfg, shard_sequence
        # ---- the reference every transport has to reproduce: the UNSHARDED step, on this rank's own GPU
        with strict_mode():
            step()
            ref_strict = step().clone()
        torch.cuda.synchronize()
        # ---- the same node's UNSHARDED step in the default mode, timed on every rank's own GPU: what the N-rank number is a
        # speed-up OF (a line from one box of the pool cannot be divided by a line from another: +-3 %)
        n_ref = max(1, min(3, args.steps))
        unsharded_s, _ = timed_alone(step, n_ref)
        cfg_variant = world >= 4 and world % 2 == 0 and args.batch == 1 and not args.no_cfg_pair_variant
        unsharded_b2_s, ref_b2, inp2 = None, None, None
        if cfg_variant:
            # the reference's real workload is the CFG pair (models/pipeline_bindyouravatar.py:897,924-933): batch 2 on 2 x N/2
            # ranks, measured after the headline, against the batch-2 step of one GPU measured here
            inp2 = make_inputs(2)
            unsharded_b2_s, ref_b2 = timed_alone(lambda: model(return_dict=False, denoise_step=0, **inp2)[0], max(1, min(2, args.steps)))
            ref_b2 = ref_b2.clone()
        model.invalidate_engine()              # (drops the unsharded workspace)
        fake = os.environ.get("BYA_BENCH_FAKE_MISMATCH", "")           # test hook: "1" = both P2P rungs fail, or a list of rungs
        fake = set(TRANSPORTS[:2]) if fake == "1" else set(f for f in fake.split(",") if f)

        def everyone(flag):
            got = [None] * world
            dist.all_gather_object(got, bool(flag))               # (object collective: works on RCCL and on gloo alike)
            return all(got)

        def shard(rung):
            if args.batch == 2:
                shard_cfg(model, dist.group.WORLD, transport=rung)      # [uncond, cond] on two halves of the ranks
            else:
                shard_sequence(model, dist.group.WORLD, transport=rung)
            return getattr(model, "_seq_transport", "torch") if getattr(model, "_seq_world", 1) > 1 else "none (CFG pair only)"

        rung = os.environ.get("BYA_SP_TRANSPORT") or TRANSPORTS[0]
        tried = []
        while True:
            ran = shard(rung)
            p2p = getattr(model, "_seq_p2p", None)
            reuse = max(3, args.warmup)        # every receive buffer is written, consumed and written again before the comparison
            with strict_mode():
                for _ in range(reuse):
                    out = step()
            torch.cuda.synchronize()
            exact = bool(torch.equal(out, ref_strict)) and (p2p is None or p2p.timeouts() == 0)
            if ran in fake:
                exact = False
            ok = everyone(exact)
            tried.append({"transport": ran, "bit_identical_to_unsharded_step": ok, "steps_before_comparison": reuse})
            if ok:
                break
            if ran == "torch" or ran.startswith("none"):
                raise SystemExit(f"the sharded step differs from the unsharded one on every transport ({tried}): no result")
            rung = TRANSPORTS[TRANSPORTS.index(ran) + 1]
        if len(tried) > 1:
            transport_note = (f"{', '.join(t['transport'] for t in tried[:-1])} failed the comparison with the unsharded step on "
                              f"this node; running on {tried[-1]['transport']}")
        # ---- default mode (stream-K attention; until the end of round 6 also split-K GEMM tails): same numbers up to fp32 summation order
        for _ in range(max(1, args.warmup)):
            out = step()
        torch.cuda.synchronize()
        # (the bit-identity above is the test; this one only says that the default mode computes the same step.  Which tiles are
        # split along K and which attention items along the keys depends on the row / head count, so sharded-default and
        # unsharded-strict differ by fp32 summation order in bf16 activations: 6e-3 after 2 layers, 1.1e-2 after 42 -- the
        # 42-layer bf16 step itself is 1.8e-2 from its fp32 oracle.  Bound: 3e-2.)
        bound = 3e-2
        diff = ((out.float() - ref_strict.float()).norm() / ref_strict.float().norm()).item()
        noise_ok = everyone(diff <= bound and (getattr(model, "_seq_p2p", None) is None or model._seq_p2p.timeouts() == 0))
        validation = {"reference": "the unsharded step on every rank's own GPU (library options gemm_splitk = 0, attn_streamk = 0)",
                      "rungs": tried, "default_mode_rel_fro_vs_reference": diff, "default_mode_bound": bound}
        if share:
            validation["ranks_share_one_gpu"] = "rehearsal of the N > 1 code path, split-K / stream-K off throughout: not a measurement"
        if not noise_ok:
            raise SystemExit(f"the sharded step in its default mode is not within bf16 summation noise of the unsharded step: {validation}")
        del ref_strict
        if args.full and getattr(model, "_seq_p2p", None) is not None:
            # what the push kernel does to the links of THIS node: one all-to-all of the packed q|k|v exchange's size, every
            # rank's figure (diagnostic, outside the timed region)
            probe = model._seq_p2p.exchange_probe(mbytes_per_peer=max(1, 40 // model._seq_p2p.world))
            got = [None] * world
            dist.all_gather_object(got, probe if getattr(model, "_seq_world", 1) > 1 else None)
            validation["p2p_exchange_probe"] = {"per_rank": got, "what": "one all-to-all launch of that many bytes to the peers, us per exchange"
                                                + ("; ranks share one GPU: local copies" if share else "")}
    else:
        for _ in range(args.warmup):
            out = step()
        torch.cuda.synchronize()

    # N > 1 on a P2P rung: the timed steps replay from a hipGraph by default (the exchanges are ordinary kernels; ~3000 launches
    # per rank-step otherwise ride on the host).  The per-kernel event pass below stays eager (events cannot be recorded inside
    # a replayed graph).
    graph = (args.graph and world == 1) or (world > 1 and getattr(model, "_seq_p2p", None) is not None and args.batch == 1
                                            and (args.graph or not args.eager))
    if graph:
        model.use_hip_graph = True
        if world == 1:
            args.no_kernel_timers = True      # (N = 1 --graph: an A/B run, no second pass)
        for _ in range(max(1, args.warmup)):
            out = step()
        torch.cuda.synchronize()
    ops.ATTN_VARIANTS.clear()
    assert torch.isfinite(out.float()).all(), "non-finite output"

    def timed_region():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            o = step()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        return time.perf_counter() - t0, o

    dt, out = timed_region()
    if world == 1 and ops.heal_handoffs(dev):
        # a split-K / stream-K hand-off timed out inside the timed steps (something else holds CUs of this GPU): the library is
        # in its unsplit mode now (ops.heal_handoffs); the K steps are timed again in that mode and the line says so
        for _ in range(max(1, args.warmup)):
            step()
        dt, out = timed_region()
    # (a P2P wait that gave up poisons the step's output with NaN; check_gemm_workspace below raises on the same condition)
    assert torch.isfinite(out.float()).all(), "non-finite output after the timed steps"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"noise_pred": out})      # before any later pass re-uses the engine's buffers
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    # Per-kernel HIP-event timing runs in a SECOND pass of the same K steps: an event pair around every one of the
    # ~3000 launches of a step costs ~5 % of wall time, which must not leak into `value`.
    ktimes = {}
    launch = "hipGraph replay" if (getattr(model, "use_hip_graph", False) and model._graph_capturable()) else "eager"
    if not args.no_kernel_timers:
        if getattr(model, "use_hip_graph", False):
            model.use_hip_graph = False
            step()
        ops.enable_kernel_timers()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        ktimes = ops.collect_kernel_timers()
    ops.check_gemm_workspace()        # no split-K / stream-K hand-off and no P2P wait of the run timed out (raises otherwise: the numbers would be void)

    # ---- N >= 4: the CFG pair beside the headline -- batch 2 as [uncond, cond] on two halves of the ranks, each half
    # sequence-parallel over N/2 (parallel.shard_cfg), against the batch-2 step one GPU of this node ran above
    cfg_pair, calibrations, unsharded_all = None, None, None
    if world > 1:
        got = [None] * world
        dist.all_gather_object(got, (calibration, unsharded_s, unsharded_b2_s))
        calibrations, unsharded_all = [g[0] for g in got], [g[1] for g in got]
        if cfg_variant:
            model.use_hip_graph = False
            shard_cfg(model, dist.group.WORLD, transport=tried[-1]["transport"])
            step2 = lambda: model(return_dict=False, denoise_step=0, **inp2)[0]
            for _ in range(max(2, args.warmup)):
                out2 = step2()
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out2 = step2()
            torch.cuda.synchronize()
            dist.barrier()
            t = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            d2 = ((out2.float() - ref_b2.float()).norm() / ref_b2.float().norm()).item()
            ops.check_gemm_workspace()
            b2 = [g[2] for g in got]
            cfg_pair = {"parallelism": f"CFG batch split x2, each half sequence-parallel x{world // 2}", "batch": 2,
                        "ms_per_step": t.item() / args.steps * 1e3, "steps_per_s": args.steps / t.item(),
                        "unsharded_batch2_step_ms_same_node": sum(b2) / len(b2) * 1e3,
                        "speedup_vs_unsharded_batch2_same_node": (sum(b2) / len(b2)) / (t.item() / args.steps),
                        "rel_fro_vs_unsharded_batch2_step": d2, "launch": "eager",
                        "transport": getattr(model, "_seq_transport", "torch")}
            if not (d2 <= 3e-2):
                raise SystemExit(f"the CFG pair on 2 x {world // 2} ranks is not within bf16 summation noise of the batch-2 step: {cfg_pair}")

    headline = (lh, lw, lt, nid) == (60, 90, 13, 2) and args.batch == 1 and not args.fp8_weights and args.qk_gain == 1.0
    if rank == 0:
        sec_per_step = dt / args.steps
        value = 1.0 / sec_per_step
        res = {
            "metric": "denoise-steps/sec", "value": value, "unit": "steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": sec_per_step * 1e3, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None,
            "dtype": "fp8 (e4m3 operands, fp32 accumulate) in the DiT Linears, bf16 elsewhere" if args.fp8_weights else "bf16",
            "data": "synthetic",
            "latent_frames_per_sec": lt * value,
            "mfma_roofline_frac_whole_step": (TFLOP_PER_STEP * (args.layers / 42) * value / (world * PEAK_BF16_TFLOPS)
                                              if headline else None),
            "config": {"workload": ("BASELINE.json configs[1]: full transformer.forward, 49x480x720 (13x30x45 latent "
                                    "tokens + 226 text), 2 characters (2 ID + 2 audio), batch 1, random-init 8.6B-param "
                                    "architecture") if headline else
                                   (f"NOT the headline config: full transformer.forward, {(lt - 1) * 4 + 1}x{lh * 8}x{lw * 8} "
                                    f"({lt}x{lh // 2}x{lw // 2} latent tokens + 226 text), {nid} characters, batch {args.batch}"
                                    + (", fp8 weights" if args.fp8_weights else "")
                                    + (f", q/k-LayerNorm gains x{args.qk_gain:g}" if args.qk_gain != 1.0 else "")),
                       "layers": args.layers, "tokens": 226 + lt * (lh // 2) * (lw // 2), "batch": args.batch,
                       "launch": launch,
                       "parallelism": "single GPU" if world == 1 else
                       (f"CFG batch split x2, each half sequence-parallel x{world // 2}" if args.batch == 2 else
                        f"sequence-parallel x{world} (head-parallel exchange around the joint attention, sharded "
                        f"Embedding Router)") + ("; exchanges = P2P push kernels over hipIpc-mapped peer buffers"
                                                 + (" (fine-grained receive buffers)" if getattr(model, "_seq_transport", "") == "p2p-fine" else "")
                                                 if getattr(model, "_seq_p2p", None) is not None else
                                                 "; exchanges = torch.distributed collectives (RCCL)")},
        }
        res["handoff_mode"] = ops.HANDOFF_MODE.get(
            dev.index, ("split-K GEMM tails + " if ops.get_option("gemm_splitk") else "") +
            ("stream-K joint attention" + ("" if ops.get_option("gemm_splitk") else " (default: the GEMMs cut no tile along K)")
             if ops.get_option("attn_streamk") else "no hand-offs (options gemm_splitk = attn_streamk = 0)"))
        if calibration is not None:
            res["board_calibration_tflops"] = calibration
            res["board_calibration"] = ("bare v_mfma_f32_16x16x32_bf16 loop, gaussian bf16 operands in registers, 256 CUs x 1 wave per SIMD, "
                                        "~0.35 s timed after an equal warm-up launch (ops.board_calibration); spec peak "
                                        f"{PEAK_BF16_TFLOPS:.0f}")
            if headline:
                res["mfma_roofline_frac_of_board_whole_step"] = TFLOP_PER_STEP * (args.layers / 42) * value / (world * calibration)
        if world > 1:
            res["board_calibration_tflops_per_rank"] = calibrations
            mean_un = sum(unsharded_all) / len(unsharded_all)
            res["unsharded_step_ms_same_node"] = mean_un * 1e3
            res["unsharded_step_ms_per_rank"] = [u * 1e3 for u in unsharded_all]
            res["speedup_vs_unsharded_same_node"] = mean_un / sec_per_step
            res["unsharded_step_note"] = (f"the unsharded batch-{args.batch} step in the default mode, eager, {n_ref} timed after one warm-up on "
                                          "every rank's own GPU before the model was sharded; mean over the ranks")
            if cfg_pair is not None:
                res["cfg_pair_variant"] = cfg_pair
        if world > 1:
            res["config"]["transport"] = getattr(model, "_seq_transport", "torch") if getattr(model, "_seq_world", 1) > 1 else "torch (CFG pair exchange only)"
            res["config"]["validated_against_unsharded_step"] = validation
        if transport_note:
            res["config"]["transport_note"] = transport_note
        if ktimes:
            # MFMA work the engine actually ISSUES (sum over every timed launch that carries a FLOP count: GEMMs, attentions,
            # row GEMMs) against the reference-algorithmic 443.9: the engine projects the perceiver / audio queries once
            # instead of per identity and routes before the two out-projections, so it executes less than the reference's
            # algorithm counts -- `mfma_roofline_frac_whole_step` prices the algorithm, `mfma_executed_frac` the matrix pipes
            exe = sum(ops.kernel_timer_flops().values()) / 1e12 / args.steps
            res["executed_tflop_per_step"] = exe
            res["mfma_executed_frac"] = exe * value / PEAK_BF16_TFLOPS          # (N > 1: rank 0's share against ONE GPU's peak)
            tot = {k: sum(v) for k, v in ktimes.items()}
            per_step = {k: tot[k] / args.steps for k in tot}
            res["kernel_ms_per_step"] = {k: round(v * 1e3, 3) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])}
            # the Embedding Router's share (every launch of MultiIPRouter.forward: scores, the four ST blocks, head)
            res["router_ms_per_step"] = round(1e3 * sum(per_step.get(k, 0.0) for k in ROUTER_TIMERS), 3)
            res["attention_variants"] = {f"{tag}:{var}": n for (tag, var), n in sorted(ops.ATTN_VARIANTS.items())}
            attn = [t for t in ktimes.get("bya_attn_fwd:joint", [])]
            attn_roof = None
            if attn:
                avg = sum(attn) / len(attn)
                tokens = 226 + lt * (lh // 2) * (lw // 2)
                shards = world // 2 if (args.batch == 2 and world > 1) else world       # ranks sharing one sample's attention
                per_launch = 4 * tokens ** 2 * 3072 / 1e12 * (args.batch if world == 1 else 1)
                ach = per_launch / max(shards, 1) / avg
                jv = sorted(v for (tag, v), n in ops.ATTN_VARIANTS.items() if tag == "joint" and n)
                attn_roof = {"kernel": f"joint {tokens}-token self-attention, softmax variant(s): " + ", ".join(jv),
                             "bound": "mfma", "achieved": ach, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                             "frac": ach / PEAK_BF16_TFLOPS,
                             "traffic": pmc_traffic(world, *(("attn_joint_w4_kernel<true>", "attn_joint_w4_kernel<false>", "attn_joint_w4_kernel") if any("w4" in v for v in jv) else ()),
                                                    "attn_fwd_kernel_d64_prescaled"),
                             "avg_launch_ms": avg * 1e3, "launches": len(attn),
                             "ms_per_step": sum(attn) / args.steps * 1e3}
            gemm = ktimes.get("bya_gemm_bf16", [])
            gemm_roof = None
            if gemm:
                gflop = ops.kernel_timer_flops().get("bya_gemm_bf16", 0.0)
                small = ktimes.get("bya_gemm_bf16_small_m", [])
                sflop = ops.kernel_timer_flops().get("bya_gemm_bf16_small_m", 0.0)
                all_ach = (gflop + sflop) / 1e12 / (sum(gemm) + sum(small))
                # FIXED NAMES, every round: `frac` / `achieved` = every Linear of the step (the definition of rounds 1-3, and of
                # round 4's `all_linears_frac`); `token_stream_frac` = the Linears with >= 1024 rows only (round 4's `frac`): the
                # step-invariant conditioning's small-row Linears stream their weights and are HBM-bound, not MFMA-bound
                gemm_roof = {"kernel": "bya_gemm_bf16, every Linear of the step (gemm256p_kernel 256x256 tiles + gemm128p_kernel 128x256 tiles "
                                       "for the rows behind the last full round; the conditioning's Linears with < 1024 rows against 2048..49152-wide weights -- "
                                       "weight-streaming, HBM-bound -- are counted in `frac` and listed in `small_m_linears`; "
                                       "`token_stream_frac` leaves them out; `traffic` is gemm256p_kernel's, per launch of that kernel)",
                             "small_m_linears": {"launches": len(small), "ms_per_step": sum(small) / args.steps * 1e3,
                                                 "tflop_per_step": sflop / 1e12 / args.steps},
                             "bound": "mfma", "achieved": all_ach, "peak": PEAK_BF16_TFLOPS,
                             "unit": "TFLOP/s", "frac": all_ach / PEAK_BF16_TFLOPS,
                             "all_linears_frac": all_ach / PEAK_BF16_TFLOPS,
                             "token_stream_frac": gflop / 1e12 / sum(gemm) / PEAK_BF16_TFLOPS,
                             "traffic": pmc_traffic(world, "gemm256p_kernel<false, false, false>", "gemm256p_kernel<false, false>", "gemm256p_kernel<false>", "gemm256p_kernel", "gemm256_kernel"),
                             "launches": len(gemm) + len(small),
                             "avg_launch_ms": (sum(gemm) + sum(small)) / (len(gemm) + len(small)) * 1e3,
                             "tflop_per_launch_avg": (gflop + sflop) / 1e12 / (len(gemm) + len(small)),
                             "ms_per_step": (sum(gemm) + sum(small)) / args.steps * 1e3}
            # headline = the kernel that dominates the step's time (the GEMM kernel when both were timed)
            cands = [r for r in (gemm_roof, attn_roof) if r]
            for r in cands:                           # the same kernels against what THIS board sustains (board_calibration_tflops)
                r["frac_of_board"] = r["achieved"] / calibration if calibration else None
            if cands:
                cands.sort(key=lambda r: -r["ms_per_step"])
                res["roofline"] = cands[0]
                if len(cands) > 1:
                    res["attn_roofline" if cands[1] is attn_roof else "gemm_roofline"] = cands[1]
        if world == 1 and headline and not args.no_fp8_variant:
            # Beside the headline, never in it: the same step with BASELINE configs[4]'s weight format (e4m3 operands in
            # the big DiT Linears and the two 3072-wide query projections), same box, same process, same inputs.
            try:
                model.enable_fp8_weights()
                step()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(3):
                    step()
                torch.cuda.synchronize()
                sec8 = (time.perf_counter() - t1) / 3
                res["fp8_weights_variant"] = {"value": 1.0 / sec8, "unit": "steps/s", "ms_per_step": sec8 * 1e3, "steps": 3,
                                              "dtype": "fp8 (e4m3 operands, fp32 accumulate) in the four DiT Linears of every block, bf16 elsewhere",
                                              "note": "not the headline metric (which is bf16); parity: tests/test_fp8_gpu.py"}
                if not args.no_kernel_timers:
                    ops.enable_kernel_timers()
                    step()
                    torch.cuda.synchronize()
                    fl8, kt8 = ops.kernel_timer_flops().get("bya_gemm_fp8", 0.0), ops.collect_kernel_timers()
                    t8 = sum(kt8.get("bya_gemm_fp8", []))
                    if t8 > 0:
                        res["fp8_weights_variant"]["gemm_fp8_roofline"] = {
                            "kernel": "bya_gemm_fp8 (gemm256p_fp8_kernel, persistent 256x256 tiles, one wave per SIMD: v_mfma_f32_16x16x128_f8f6f4, e4m3; the four DiT Linears)",
                            "bound": "mfma", "achieved": fl8 / t8 / 1e12, "peak": 5000.0, "unit": "TFLOP/s",
                            "frac": fl8 / t8 / 1e12 / 5000.0, "launches": len(kt8["bya_gemm_fp8"]), "ms_per_step": t8 * 1e3,
                            "quantiser_ms_per_step": (sum(kt8.get("bya_quantize_rows_fp8", [])) +
                                                      sum(kt8.get("bya_layernorm_fp8", []))) * 1e3}
            except Exception as e:                        # noqa: BLE001  (an extra, never a reason to lose the headline line)
                res["fp8_weights_variant"] = {"error": str(e)[:200]}
            finally:
                model.enable_fp8_weights(False)
        if world == 1 and headline and not args.no_qk_gain_variant:
            # Beside the headline, never in it: the same step with every q/k-LayerNorm gain doubled (a stand-in for a trained
            # checkpoint's learned gains, reference models/transformer.py:200-209; the synthetic gains are N(1, 0.1)): the
            # worst-case score bound of a layer goes from ~20 to ~78.  Round 4's limit of 48 sent such a checkpoint to the
            # running-maximum kernel (-9 % on 36 % of the step) without saying so; the hand-placed kernel computes P = exp2(s)
            # with no offset, so it is safe to 90.  Above that (non-uniform gains: tests/test_forward_gpu.py) the bound comes
            # from the data, per head.
            try:
                scale_qk_gains(2.0)
                ops.ATTN_VARIANTS.clear()
                step()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(3):
                    o3 = step()
                torch.cuda.synchronize()
                sec3 = (time.perf_counter() - t1) / 3
                res["large_qk_gain_variant"] = {
                    "value": 1.0 / sec3, "unit": "steps/s", "ms_per_step": sec3 * 1e3, "steps": 3, "qk_gain": 2.0,
                    "worst_case_score_bound": max(model._engine.score_bound),
                    "attention_variants": {f"{tag}:{var}": n for (tag, var), n in sorted(ops.ATTN_VARIANTS.items()) if tag == "joint"},
                    "heads_on_the_running_maximum_kernel_last_layer": int(model._engine._ws["qk_flags"][:48].sum().item())
                    if "qk_flags" in (model._engine._ws or {}) else None,
                    "finite": bool(torch.isfinite(o3.float()).all()),
                    "note": "not the headline metric; parity: tests/test_forward_gpu.py::test_large_qk_gains_keep_the_fast_attention_kernel"}
            except Exception as e:                        # noqa: BLE001  (an extra, never a reason to lose the headline line)
                res["large_qk_gain_variant"] = {"error": str(e)[:200]}
            finally:
                scale_qk_gains(0.5)
        if world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(os.cpu_count() or 1, config0=args.cpu_baseline_config0)
            ref0 = committed_config0_baseline()
            if ref0 and not args.cpu_baseline_config0:
                res["cpu_baseline"]["config0_reference"] = ref0
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
