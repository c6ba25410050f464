#!/usr/bin/env python3
"""What does BYA_SP_VERIFY=all cost per exchange?  N processes on ONE GPU (hipIpc-mapped buffers; local HBM, no link), each
with two P2PGroups on the same process group -- verification off and on -- timed with ``P2PGroup.exchange_probe`` in the
same run, alternating, at the size of the packed q|k|v exchange (6 MB per peer) and at 64 KB per peer (the fixed cost).
Prints one JSON line per group size: the median over the rounds of every rank's microseconds per exchange, rank 0's shown.

    python tools/p2p_verify_cost.py [N ...]        (default: 2 8)"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 7


def worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bind_your_avatar_implementation_amd.p2p import P2PGroup
        res = {}
        for label, mb in (("6 MB per peer", 6), ("64 KB per peer", 1 / 16)):
            # (a pair of groups per size: the probe's receive buffer has one name and therefore one shape per group)
            groups = {"off": P2PGroup(dist.group.WORLD, dev, verify=False), "on": P2PGroup(dist.group.WORLD, dev, verify=True)}
            for g in groups.values():
                g.wait_limit_ms = 10000
            us = {"off": [], "on": []}
            for _ in range(ROUNDS):
                for mode, g in groups.items():
                    dist.barrier()
                    us[mode].append(g.exchange_probe(mbytes_per_peer=mb, reps=10)["us"])
                if any(g.timeouts() for g in groups.values()):        # a wait gave up: nothing else is started on the GPU
                    ret[rank] = {"timeouts": [g.timeouts() for g in groups.values()]}
                    return
            res[label] = {m: round(statistics.median(v), 1) for m, v in us.items()}
            res[label]["all rounds"] = us
            res["mismatches"] = res.get("mismatches", []) + groups["on"].exchange_mismatches()
            res["verify launches"] = res.get("verify launches", 0) + groups["on"].verifies
        ret[rank] = res
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    for world in [int(a) for a in sys.argv[1:]] or [2, 8]:
        ret = mp.Manager().dict()
        mp.spawn(worker, args=(world, 34100 + os.getpid() % 500 + world, ret), nprocs=world, join=True)
        r0 = dict(ret[0])
        if "timeouts" in r0:
            print(json.dumps({"processes": world, **r0}), flush=True)
            raise SystemExit(1)
        line = {"processes": world, "mismatches": r0["mismatches"], "verify_launches": r0["verify launches"]}
        for label in ("6 MB per peer", "64 KB per peer"):
            line[label] = {"us_verify_off": r0[label]["off"], "us_verify_on": r0[label]["on"],
                           "us_verify_on_worst_rank": max(dict(ret[r])[label]["on"] for r in range(world)),
                           "us_verify_off_worst_rank": max(dict(ret[r])[label]["off"] for r in range(world)),
                           "rounds_rank0": r0[label]["all rounds"]}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
