"""The sharded step with the audio kv-mix as ONE launch over a segment table (engine.sp_segment_mix, BYA_SP_SEGMENT_MIX;
ops.attn_kv_mix_segments) against the same step with one launch per partial frame: 2 ranks on the one GPU, hw (18, 22) -- 297
video + 226 text rows, shards that differ by a row, rank 1 holding parts of all three frames --, p2p transport; the outputs
bit for bit, both within the sharded test's bound of the unsharded step, the launches counted per entry point, a hipGraph
replay of the switched-on step; bf16 and with the audio out-projection an MX Linear (the MX-output entry)."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

WORKER_SECONDS = 420        # per spawned pair; a healthy run takes a fraction of it


def _worker(rank, world, port, ret, mx):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["BYA_SP_SEGMENT_MIX"] = "0"
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)      # 2 ranks share the single test GPU
    try:
        from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
        from bind_your_avatar_implementation_amd.parallel import shard_sequence
        from bind_your_avatar_implementation_amd.synth import synth_inputs
        from test_forward_gpu import SMALL_KW, to_dev
        dev = torch.device("cuda:0")
        hw = (18, 22)
        model = BindyouravatarTransformer3DModel(**dict(SMALL_KW, sample_height=hw[0], sample_width=hw[1]), device=dev)
        model.init_synthetic(seed=1, fast=True)
        inp = to_dev(synth_inputs(batch=1, frames=3, height=hw[0], width=hw[1], seed=3, n_id=2), dev)
        if mx:
            model.enable_mx_weights("mxfp8", linears=("qkv", "out", "ff1", "ff2", "ao"))
        full = model(**inp)[0].clone()
        shard_sequence(model, dist.group.WORLD, transport="p2p")

        def counted_step(switch):
            os.environ["BYA_SP_SEGMENT_MIX"] = switch
            model.invalidate_engine()
            model(**inp)                                  # builds the engine of this setting
            assert model._engine.sp_segment_mix is (switch == "1")
            ops.enable_kernel_timers()
            try:
                out = model(**inp)[0].clone()
            finally:
                times = ops.collect_kernel_timers()
            return out, {k: len(v) for k, v in times.items() if k.startswith("bya_attn_kv_mix")}

        off, n_off = counted_step("0")
        on, n_on = counted_step("1")
        segs = model._engine  # (the engine of the switched-on setting stays: the graph below replays it)
        model.use_hip_graph = True
        model(**inp)                                      # capture
        graphed = [model(**inp)[0].clone() for _ in range(2)]
        model.use_hip_graph = False
        assert segs is model._engine and model._seq_p2p.timeouts() == 0
        n_layers = len(model.transformer_blocks)
        ret[rank] = dict(
            off_vs_full=float((off.float() - full.float()).abs().max()), on_vs_full=float((on.float() - full.float()).abs().max()),
            on_equals_off=bool(torch.equal(on, off)), graph_equals_eager=all(bool(torch.equal(g, on)) for g in graphed),
            n_off=n_off, n_on=n_on, audio_layers=len(range(0, n_layers, SMALL_KW["audio_attn_interval"])),
            face_layers=len(range(0, n_layers, SMALL_KW["cross_attn_interval"])), batch=1)
    finally:
        dist.destroy_process_group()


def _spawn(fn, args, nprocs):
    """mp.spawn with a time limit for the workers: past it they are killed and the test fails (no retry)."""
    import torch.multiprocessing as mp
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + WORKER_SECONDS
    while not ctx.join(timeout=5):                        # (returns as soon as a worker ends; raises if one failed)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"the workers did not finish within {WORKER_SECONDS} s")


@pytest.mark.parametrize("mx", [False, True], ids=["bf16", "mxfp8-ao"])
def test_one_segmented_launch_per_layer_equals_the_launches_per_partial_frame(dev, mx):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    _spawn(_worker, (2, 32300 + os.getpid() % 1000 + 17 * mx, ret, mx), 2)
    print("segmented audio kv-mix, 2 ranks:", dict(ret))
    seg, per = ("bya_attn_kv_mix_mx_seg", "bya_attn_kv_mix_mx") if mx else ("bya_attn_kv_mix_seg", "bya_attn_kv_mix")
    for r in (0, 1):
        d = ret[r]
        assert d["on_equals_off"] and d["graph_equals_eager"], d
        assert d["off_vs_full"] <= 2e-2 and d["on_vs_full"] <= 2e-2, d        # the bound of the sharded test in test_forward_gpu.py
        audio, face = d["audio_layers"] * d["batch"], d["face_layers"] * d["batch"]
        assert audio == 2 and face == 1
        # switch on: one segmented launch per audio layer and sample, none per partial frame; the face path is what it was
        # (its out-projection stays bf16 in both parametrisations: one bya_attn_kv_mix launch per face layer)
        assert d["n_on"].get(seg, 0) == audio, d
        assert d["n_on"].get("bya_attn_kv_mix", 0) == face and d["n_on"].get("bya_attn_kv_mix_mx", 0) == 0, d
        assert set(d["n_on"]) <= {seg, "bya_attn_kv_mix"}, d
        # switch off: no segmented launch, at least one launch per audio layer
        assert not any(k.endswith("_seg") for k in d["n_off"]), d
        assert d["n_off"].get(per, 0) - (0 if mx else face) >= audio, d
    # (rank 0 holds the text rows and 35 video rows of frame 0: one segment; rank 1's rows span all three frames)
    assert max(ret[r]["n_off"].get(per, 0) - (0 if mx else 1) for r in (0, 1)) > 2, dict(ret)
