"""BYA_SP_VERIFY=all on the sharded denoise step: every exchange of the step -- the q|k|v heads, heads -> rows, every router
repartition, the mods gather, the output gather and the canary's own 8-byte exchange -- carries its checksums and is verified
behind its wait, eager and from a replayed hipGraph, and the step still computes exactly what the unsharded step computes.
Two ranks on the one GPU, modelled on test_sharded_step_checksum_catches_a_stale_receive_buffer (tests/test_forward_gpu.py)."""
import os

import pytest
import torch

from test_forward_gpu import SMALL_KW, to_dev

pytestmark = pytest.mark.gpu


def _verify_all_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["BYA_SP_VERIFY"] = "all"
    os.environ["BYA_P2P_TIMEOUT"] = "2"                # seconds: a wait that gives up does so quickly
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops, parallel
        from bind_your_avatar_implementation_amd.parallel import shard_sequence
        from bind_your_avatar_implementation_amd.synth import synth_inputs
        dev = torch.device("cuda:0")
        model = BindyouravatarTransformer3DModel(**SMALL_KW, device=dev).init_synthetic(seed=1, fast=True)
        inp = to_dev(synth_inputs(batch=1, frames=3, height=16, width=24, seed=3), dev)
        full = model(**inp)[0].clone()
        shard_sequence(model, dist.group.WORLD, transport="p2p")
        g = model._seq_p2p
        assert g is not None and g.verify and model._seq_transport == "p2p"
        if g.timeouts():                               # (the set-up's self-test ran verified as well)
            ret[rank] = ("timeout", g.timeouts())
            return
        counted0, pushes0, verifies0 = parallel.COLLECTIVE_CALLS.get("p2p_exchange", 0), g.pushes, g.verifies
        outs = [model(**inp)[0].clone() for _ in range(2)]
        counted, pushes, verifies = parallel.COLLECTIVE_CALLS["p2p_exchange"] - counted0, g.pushes - pushes0, g.verifies - verifies0
        if g.timeouts():
            ret[rank] = ("timeout", g.timeouts())
            return
        model.use_hip_graph = True                     # every verify launch is captured with the step
        model(**inp)                                   # capture
        outs += [model(**inp)[0].clone() for _ in range(2)]
        model.use_hip_graph = False
        same = all(bool(torch.equal(o, full)) for o in outs)
        timeouts = g.timeouts()
        clean = True
        try:
            ops.check_gemm_workspace()
        except Exception:                              # noqa: BLE001
            clean = False
        ret[rank] = (same, g.exchange_mismatches(), g.mismatches(), timeouts, (counted, pushes, verifies), clean)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sharded_step_with_every_exchange_verified_equals_the_unsharded_step(dev):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_verify_all_worker, args=(2, 31700 + os.getpid() % 1000, ret), nprocs=2, join=True)
    print(dict(ret))
    for r in (0, 1):
        assert ret[r][0] != "timeout", ret[r]
        same, log, mism, timeouts, (counted, pushes, verifies), clean = ret[r]
        assert same and log == [] and mism == 0 and timeouts == 0 and clean, ret[r]
        # one verify launch per exchange launch, whoever issued it (the step's own counter and the group's agree)
        assert verifies == pushes == counted > 0, ret[r]
