"""The P2P exchange engine (bya_p2p_push / bya_p2p_wait + p2p.py) with several processes sharing the ONE test GPU: peer
buffers are mapped through hipIpc exactly as they are across the GPUs of a node (xGMI is then the path the stores take;
here it is the local HBM).  Checks the protocol, not link speed: scatter/gather lists, uneven pieces, an empty piece,
sequence numbers over many exchanges on a reused buffer, the side-stream form, and replay inside a hipGraph."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, ret, mode):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bind_your_avatar_implementation_amd.p2p import P2PGroup
        g = P2PGroup(dist.group.WORLD, dev, mem="fine" if mode == "fine" else "coarse")
        if mode == "fine":
            assert g.ctrl_kind == "fine"                 # this platform hands out fine-grained memory: the flags live in it
            g.self_test(rounds=8, elems=64 * 1024)
            mode = "plain"
        # an uneven all-to-all with TWO pieces per destination (like q|k|v blocks): rank r sends to rank j
        #   piece A: (r + 1) * 1000 + 8 * j elements, piece B: 4096 elements, values encode (iteration, r, j, piece)
        nA = lambda r, j: ((r + 1) * 1000 + 8 * j) // 8 * 8
        nB = 4096
        recvA = g.symmetric("recvA", (sum(nA(r, rank) for r in range(world)),), torch.bfloat16, zero=True)
        recvB = g.symmetric("recvB", (world, nB), torch.bfloat16, zero=True)
        sendA = [torch.zeros(nA(rank, j), dtype=torch.bfloat16, device=dev) for j in range(world)]
        sendB = torch.zeros(world, nB, dtype=torch.bfloat16, device=dev)
        empty = torch.zeros(0, dtype=torch.bfloat16, device=dev)
        pieces = []
        for j in range(world):
            offA = sum(nA(r, j) for r in range(rank))
            pieces += [(sendA[j], j, "recvA", offA), (sendB[j], j, "recvB", rank * nB), (empty, j, "recvB", 0)]
        ch = g.channel("a2a", pieces)

        def fill(it):
            for j in range(world):
                sendA[j].fill_(float((it % 50) + rank * 0.5 + j * 0.125))
                sendB[j].fill_(float(-(it % 50) - rank * 0.5 - j * 0.125))

        def expect(it):
            a = torch.cat([torch.full((nA(r, rank),), float((it % 50) + r * 0.5 + rank * 0.125)) for r in range(world)])
            b = torch.stack([torch.full((nB,), float(-(it % 50) - r * 0.5 - rank * 0.125)) for r in range(world)])
            return a.to(torch.bfloat16), b.to(torch.bfloat16)

        ok = True
        if mode in ("plain", "side"):
            for it in range(16 if world > 4 else 40):
                fill(it)
                if mode == "side":
                    ch.push(side=True)
                    junk = torch.randn(512, 512, device=dev) @ torch.randn(512, 512, device=dev)     # independent work underneath
                    ch.wait()
                else:
                    ch.exchange()
                a, b = expect(it)
                got_a, got_b = recvA.clone(), recvB.clone()          # consumer kernels, stream-ordered behind the wait
                # the NEXT push may only overwrite recvA/B on the peers after they consumed this one: a second channel
                # (consumed -> ready) carries that dependency here, like the attention output exchange does in the step
                g.channel("ack", [(empty, j, "recvB", 0) for j in range(world)]).exchange()
                ok &= bool(torch.equal(got_a.cpu(), a)) and bool(torch.equal(got_b.cpu(), b))
        else:                                                         # the exchange inside a replayed hipGraph
            fill(0)
            ack = g.channel("ack", [(empty, j, "recvB", 0) for j in range(world)])
            got_a, got_b = torch.empty_like(recvA), torch.empty_like(recvB)
            ch.exchange()
            ack.exchange()
            torch.cuda.synchronize()
            dist.barrier()
            graph = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with torch.cuda.graph(graph, stream=s):
                    ch.push(side=(mode == "graph_side"))
                    ch.wait()
                    got_a.copy_(recvA)
                    got_b.copy_(recvB)
                    ack.exchange()
            torch.cuda.current_stream().wait_stream(s)
            for it in range(1, 25):
                fill(it)
                graph.replay()
                torch.cuda.synchronize()
                a, b = expect(it)
                ok &= bool(torch.equal(got_a.cpu(), a)) and bool(torch.equal(got_b.cpu(), b))
        ret[rank] = (ok, g.timeouts(), g.pushes)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,mode", [(2, "plain"), (4, "side"), (8, "plain"), (2, "graph"), (4, "graph_side"), (4, "fine")])
def test_p2p_exchange_between_processes_on_one_gpu(dev, world, mode):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, 32100 + os.getpid() % 500 + world * 7 + len(mode), ret, mode), nprocs=world, join=True)
    print(dict(ret))
    for r in range(world):
        ok, timeouts, pushes = ret[r]
        assert ok and timeouts == 0 and pushes > 0, (r, ret[r])


def _timeout_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["BYA_P2P_TIMEOUT"] = "0.3"                # seconds
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bind_your_avatar_implementation_amd import _hip, ops
        from bind_your_avatar_implementation_amd.p2p import P2PGroup
        g = P2PGroup(dist.group.WORLD, dev)
        n = 4096
        recv = g.symmetric("r", (world, n), torch.bfloat16, zero=True)
        send = torch.full((world, n), float(rank + 1), dtype=torch.bfloat16, device=dev)
        ch = g.channel("x", [(send[j], j, "r", rank * n) for j in range(world)])
        ch2 = g.channel("y", [(send[j], j, "r", rank * n) for j in range(world)])       # a second exchange of the "step"
        ch.exchange()                                     # a healthy exchange first
        out = torch.ones(1000, dtype=torch.bfloat16, device=dev)
        g.poison(out)
        torch.cuda.synchronize()
        healthy = (g.timeouts() == 0, bool((out == 1).all()))
        dist.barrier()
        # rank 1 "falls behind": it never pushes its second exchange; rank 0's wait gives up after the limit
        if rank == 0:
            ch.exchange()
            g.poison(out)
            torch.cuda.synchronize()
            # ... and from then on no wait of the GROUP polls its limit again (the advisor's round-5 finding: ~280 exchanges per
            # rank-step, each bounded separately, made a dead peer stall every step for hours): 40 exchanges on ANOTHER channel
            # whose peer never pushes return at once -- 40 x 0.3 s otherwise
            import time
            t0 = time.time()
            for _ in range(40):
                ch2.exchange()
            torch.cuda.synchronize()
            fast = time.time() - t0 < 3.0
            raised = False
            try:
                ops.check_gemm_workspace()
            except _hip.ByaError:
                raised = True
            # a retired group (a rung of the transport ladder that was left) no longer fails the run at its end
            g.close()
            clean = True
            try:
                ops.check_gemm_workspace()
            except _hip.ByaError:
                clean = False
            ret[rank] = (healthy, g.timeouts(), bool(torch.isnan(out.float()).all()), raised, clean, fast)
        else:
            ret[rank] = (healthy, 0, True, True, True, True)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_p2p_wait_that_gives_up_is_loud(dev):
    """A wait whose peer never pushes gives up after BYA_P2P_TIMEOUT seconds (wall clock) instead of hanging the GPU, and
    that is not silent: the channel's time-out word is sticky, ``bya_p2p_poison`` turns the step's output into NaN, and
    ``ops.check_gemm_workspace`` (pipeline end, bench end) raises -- until the group is retired (``close``: what the transport
    ladder does with a rung it leaves).  After the first time-out the group's later waits return without polling."""
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_timeout_worker, args=(2, 32700 + os.getpid() % 200, ret), nprocs=2, join=True)
    print(dict(ret))
    for r in (0, 1):
        assert ret[r][0] == (True, True), ret[r]          # healthy run: no time-out, output untouched
    assert ret[0][1] > 0 and ret[0][2] and ret[0][3] and ret[0][4], ret[0]
    assert ret[0][5], "waits behind the group's first time-out polled their limit again"


@pytest.mark.gpu
def test_bench_two_ranks_validates_against_the_unsharded_step_and_walks_the_ladder(tmp_path):
    """bench.py with N > 1: every rank runs the UNSHARDED step on its own GPU first; the sharded step must reproduce it bit
    for bit (strict summation order, after enough steps that every receive buffer has been re-used) before anything is
    timed, else ALL ranks move one rung down the transport ladder p2p -> p2p-fine -> torch.distributed and the line says so.
    Exercised with both ranks on the one GPU (BYA_BENCH_SHARE_GPU=1: gloo process group): once as it is, once with the
    both P2P rungs failing in turn (BYA_BENCH_FAKE_MISMATCH=1: p2p -> p2p-fine -> torch, every rung walked)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--layers", "2", "--steps", "1", "--warmup", "1",
            "--full", "--no-cpu-baseline", "--no-fp8-variant", "--no-kernel-timers"]
    for fake, want in (("", "p2p"), ("1", "torch")):
        env = dict(os.environ, BYA_BENCH_SHARE_GPU="1", BYA_BENCH_FAKE_MISMATCH=fake, HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
        r = subprocess.run(base, env=env, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, (r.stdout[-800:], r.stderr[-1500:])
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["value"] > 0
        cfg = d["config"]
        assert cfg["transport"] == want, cfg
        val = cfg["validated_against_unsharded_step"]
        assert [t["transport"] for t in val["rungs"]][-1] == want and val["rungs"][-1]["bit_identical_to_unsharded_step"]
        assert val["default_mode_rel_fro_vs_reference"] <= val["default_mode_bound"]
        # (r6) what the line needs to be read on its own: the board's calibration, and the same node's unsharded step
        assert d["board_calibration_tflops"] > 0 and len(d["board_calibration_tflops_per_rank"]) == 2
        assert d["unsharded_step_ms_same_node"] > 0 and len(d["unsharded_step_ms_per_rank"]) == 2
        assert abs(d["speedup_vs_unsharded_same_node"] - d["unsharded_step_ms_same_node"] / d["ms_per_step"]) < 1e-6
        assert cfg["launch"] == ("hipGraph replay" if want == "p2p" else "eager")      # the P2P rungs replay by default
        if want == "p2p":
            assert "P2P push kernels" in cfg["parallelism"] and "transport_note" not in cfg and len(val["rungs"]) == 1
        else:
            assert "torch.distributed collectives" in cfg["parallelism"] and "p2p, p2p-fine failed" in cfg["transport_note"]
            assert [t["transport"] for t in val["rungs"]] == ["p2p", "p2p-fine", "torch"]
