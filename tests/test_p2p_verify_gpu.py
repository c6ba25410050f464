"""The exchange verification of the P2P engine (BYA_SP_VERIFY=all / P2PGroup(verify=True)) on the GPU: the push kernel's
VERIFY instances sum what they copy, the records travel to the receiver, bya_p2p_verify sums the receive buffers behind the
wait and logs what differs.  All checks exact (integer sums, torch.equal).  One process sending to itself through the full
table / flag / wait / verify path, then two processes on the one GPU (hipIpc-mapped buffers, as across a node).  Every wait
here has a 2 s limit, and a test that sees a time-out ends without starting anything else on the GPU."""
import os

import pytest
import torch

from test_p2p_verify_cpu import checksum, piece_words

pytestmark = pytest.mark.gpu

KEY = ("vx", "four pieces", 4099)


@pytest.fixture
def group(dev, tmp_path):
    """A 1-rank gloo group on a FileStore, and a verifying P2PGroup on it; both retired afterwards (a group that has logged a
    mismatch must not fail the end-of-run check of a later test).  Nothing of them may be left for a LATER garbage collection:
    a P2PGroup and its channels refer to each other, and the group holds the gloo process group -- the spawning tests start a
    ``multiprocessing.Manager``, a FORKED child of this process, and a collection that runs there would destroy a process
    group whose threads do not exist in the child.  So the cycle is broken and collected here, in the process that owns it."""
    import gc
    import torch.distributed as dist
    from bind_your_avatar_implementation_amd.p2p import P2PGroup
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    g = None
    try:
        g = P2PGroup(dist.group.WORLD, dev, verify=True)
        g.wait_limit_ms = 2000
        yield g
    finally:
        if g is not None:
            torch.cuda.synchronize()
            g.close()
            g._channels.clear()
            g.group = None
        g = None
        dist.destroy_process_group()
        gc.collect()


class FourPieces:
    """One channel whose four pieces take every branch of the copy loop: 4099 bf16 contiguous (16-byte body + 2-byte tail);
    37 rows x 520 bytes at pitches 1040 / 1560 (rows grouped into one chunk); one row of 40 000 bf16 (80 000 bytes: cut at
    64 KiB); 26 int16 from an odd word on (the narrow loop)."""

    def __init__(self, g, dev):
        self.g, self.dev = g, dev
        self.recv = [g.symmetric("r0", (4104,), torch.bfloat16, zero=True), g.symmetric("r1", (37, 780), torch.bfloat16, zero=True),
                     g.symmetric("r2", (40000,), torch.bfloat16, zero=True), g.symmetric("r3", (64,), torch.int16, zero=True)]
        self.src = [torch.zeros(4099, dtype=torch.int16, device=dev), torch.zeros(37, 520, dtype=torch.int16, device=dev),
                    torch.zeros(40000, dtype=torch.int16, device=dev), torch.zeros(64, dtype=torch.int16, device=dev)]
        bf = lambda t: t.view(torch.bfloat16)
        self.sent = [bf(self.src[0]), bf(self.src[1])[:, :260], bf(self.src[2]), self.src[3][1:27]]
        self.pieces = [(self.sent[0], 0, "r0", 0), (self.sent[1], 0, "r1", 12, 780), (self.sent[2], 0, "r2", 0), (self.sent[3], 0, "r3", 3)]
        assert self.sent[3].data_ptr() % 4 == 2 and self.sent[1].stride(0) * 2 == 1040
        self.where = [lambda r: r[:4099], lambda r: r.view(-1)[12:12 + 36 * 780 + 260].as_strided((37, 260), (780, 1)),
                      lambda r: r, lambda r: r[3:29]]
        self.gen = torch.Generator(device="cpu").manual_seed(11)

    def channel(self):
        return self.g.channel(KEY, self.pieces)

    def fill(self):
        """A new payload; -> the sums the records must carry (numpy restatement, from the host copy)."""
        want = []
        for s, t in zip(self.src, self.sent):
            s.copy_(torch.randint(-32768, 32767, s.shape, dtype=torch.int16, generator=self.gen))
            want.append(checksum(piece_words(t.cpu())))
        return want

    def arrived(self):
        return all(torch.equal(w(r).view(torch.int16), t.view(torch.int16)) for w, r, t in zip(self.where, self.recv, self.sent))

    def record_sums(self, ch):
        rec = ch.records()[0]
        assert [p["buffer"] for p in rec["pieces"]] == ["r0", "r1", "r2", "r3"]
        assert [(p["dst_byte_offset"], p["row_bytes"], p["rows"]) for p in rec["pieces"]] == [(0, 8198, 1), (24, 520, 37), (0, 80000, 1), (6, 52, 1)]
        assert rec["pieces"][1]["dst_pitch"] == 1560
        return rec["sequence"], [(p["A"], p["B"]) for p in rec["pieces"]]


def _clean_rounds(g, fp, rounds=3):
    ch = fp.channel()
    seq0 = fp.record_sums(ch)[0] if g.pushes else 0
    for it in range(rounds):
        want = fp.fill()
        if it % 2:
            ch.push().wait().verify()
        else:
            ch.exchange()
        assert g.timeouts() == 0, "a wait gave up: nothing else is started on the GPU"
        seq, got = fp.record_sums(ch)
        assert fp.arrived()
        assert got == want, (it, got, want)
        assert seq == seq0 + it + 1
    assert g.exchange_mismatches() == [] and g.exchange_mismatch_count() == 0
    g.check()


def test_records_carry_the_checksums_and_a_tampered_piece_is_named(group, dev):
    from bind_your_avatar_implementation_amd import _hip, ops
    g, fp = group, FourPieces(group, dev)
    _clean_rounds(g, fp)
    assert g.verifies >= g.pushes == 3                    # every exchange and every push / wait pair ends with a verify launch
    ops.enable_kernel_timers()                            # the verify launch has a timer bucket of its own
    fp.fill()
    fp.channel().exchange()
    timers = ops.collect_kernel_timers()
    assert list(timers) == ["bya_p2p_verify"] and len(timers["bya_p2p_verify"]) == 1
    assert g.timeouts() == 0, "a wait gave up: nothing else is started on the GPU"
    out = torch.ones(1000, dtype=torch.bfloat16, device=dev)
    g.poison(out)
    assert bool((out == 1).all())
    # memory itself changes behind the wait: ONE element of the 2-D piece
    ch = fp.channel()
    want = fp.fill()
    ch.push().wait()                                      # (the wait's own verify launch: still clean)
    assert g.timeouts() == 0, "a wait gave up: nothing else is started on the GPU"
    assert g.exchange_mismatches() == []
    fp.recv[1].view(torch.int16)[5, 12 + 17] += 1
    ch.verify()
    log = g.exchange_mismatches()
    assert len(log) == 1 and g.exchange_mismatch_count() == 1, log
    e = log[0]
    assert (e["key"], e["sender"], e["piece"], e["buffer"], e["reread_matches"], e["kind"]) == (KEY, 0, 1, "r1", 0, "sums differ"), e
    assert e["sequence"] == 5 and e["want"] == want[1] and e["got"] != want[1]
    got = checksum(piece_words(fp.where[1](fp.recv[1]).cpu()))
    assert e["got"] == got and got != want[1]             # the receiver summed what its buffer holds now
    with pytest.raises(_hip.ByaError, match="four pieces") as err:
        g.check()
    assert "1 piece(s)" in str(err.value) and "piece 1 from rank 0" in str(err.value)
    with pytest.raises(_hip.ByaError, match="four pieces"):
        ops.check_gemm_workspace()                        # the end-of-run check picks it up through check()
    g.poison(out)
    assert bool(torch.isnan(out.float()).all())
    assert g.mismatches() == 0 and g.timeouts() == 0      # word 38 and the time-out words keep their meaning


@pytest.mark.parametrize("groups", [16, 128])
def test_sums_do_not_depend_on_the_grid(group, dev, lib_options, groups):
    """BYA_P2P_GROUPS (workgroups of a push): the option accepts 16..1024 -- its lowest value and the default.  The four pieces
    are 5 chunks; a second channel of 48 chunks makes the two settings launch different grids."""
    lib_options(p2p_groups=groups)
    g, fp = group, FourPieces(group, dev)
    _clean_rounds(g, fp)
    big = g.symmetric("big", (24, 40960), torch.bfloat16, zero=True)
    src = torch.randint(-32768, 32767, (24, 40000), dtype=torch.int16).to(dev)
    ch = g.channel(("vx", "big"), [(src.view(torch.bfloat16), 0, "big", 64, 40960)])
    assert ch.cur[2] == 48
    for it in range(2):
        (ch.push().wait() if it else ch.exchange())
        assert g.timeouts() == 0, "a wait gave up: nothing else is started on the GPU"
        p = ch.records()[0]["pieces"]
        assert len(p) == 1 and (p[0]["A"], p[0]["B"]) == checksum(piece_words(src.cpu()))
        assert torch.equal(big.view(torch.int16)[:, 64:40064], src)
    assert g.exchange_mismatches() == []


def test_exchange_and_verify_replay_from_a_graph(group, dev):
    g, fp = group, FourPieces(group, dev)
    _clean_rounds(g, fp, rounds=1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            ch = fp.channel().exchange()                  # the exchange launch + the verify launch
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    verifies = g.verifies
    for it in range(3):
        want = fp.fill()
        graph.replay()
        assert g.timeouts() == 0, "a wait gave up: nothing else is started on the GPU"
        seq, got = fp.record_sums(ch)
        assert fp.arrived() and got == want and seq == 2 + it          # sequence numbers live on the device: a replay advances them
    assert g.exchange_mismatches() == [] and g.verifies == verifies
    g.check()


def _two_rank_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bind_your_avatar_implementation_amd.p2p import P2PGroup
        g = P2PGroup(dist.group.WORLD, dev, verify=True)
        g.wait_limit_ms = 2000
        # rank j's receive buffer has ITS shape: [world * R rows, C_j]; rank r's rows land in rows [r * R, (r + 1) * R) of it:
        # a strided source (200 of 256 columns) and a contiguous source scattered to the pitched rows, two pieces per pair
        R = 19
        C = lambda j: 264 + 16 * j
        rx = g.symmetric("rx", (world * R, C(rank)), torch.bfloat16, zero=True)
        s1 = torch.zeros(world, R, 256, dtype=torch.int16, device=dev)
        s2 = torch.zeros(world, R, 40, dtype=torch.int16, device=dev)
        bf = lambda t: t.view(torch.bfloat16)
        pieces = []
        for j in range(world):
            pieces += [(bf(s1[j])[:, :200], j, "rx", rank * R * C(j) + 8, C(j)), (bf(s2[j]), j, "rx", rank * R * C(j) + 216, C(j))]
        key = ("vx", "two ranks")
        ch = g.channel(key, pieces)
        empty = torch.zeros(0, dtype=torch.bfloat16, device=dev)
        ack = g.channel(("vx", "ack"), [(empty, j, "rx", 0) for j in range(world)])
        cols = torch.arange(256, dtype=torch.int32, device=dev)
        rows = torch.arange(R, dtype=torch.int32, device=dev)[:, None]

        def payload(it, r, j):                            # what rank r sends rank j in round `it`: every word its own value
            v = (it * 7919 + r * 1009 + j * 101 + rows * 257 + cols) % 65536 - 32768
            return v.to(torch.int16)

        def fill(it):
            for j in range(world):
                s1[j].copy_(payload(it, rank, j))
                s2[j].copy_(payload(it + 50, rank, j)[:, :40])

        def arrived(it, got):
            ok = True
            for r in range(world):
                blk = got.view(torch.int16)[r * R:(r + 1) * R]
                ok &= bool(torch.equal(blk[:, 8:208], payload(it, r, rank)[:, :200]))
                ok &= bool(torch.equal(blk[:, 216:256], payload(it + 50, r, rank)[:, :40]))
            return ok

        ok, it = True, 0
        for it in range(3):                               # eager: the one-launch and the two-launch form
            fill(it)
            (ch.push().wait() if it % 2 else ch.exchange())
            got = rx.clone()
            ack.exchange()                                # "consumed": the peer may overwrite rx
            ok &= arrived(it, got)
        if g.timeouts():                                  # a wait gave up: report, start nothing else on the GPU
            ret[rank] = ("timeout", g.timeouts())
            return
        got = torch.empty_like(rx)
        torch.cuda.synchronize()
        dist.barrier()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                g.channel(key, pieces).exchange()
                got.copy_(rx)
                ack.exchange()
        torch.cuda.current_stream().wait_stream(s)
        for it in range(3, 6):
            fill(it)
            graph.replay()
            torch.cuda.synchronize()
            ok &= arrived(it, got)
        clean = (ok, g.exchange_mismatches(), g.timeouts())
        if clean[2]:
            ret[rank] = ("timeout", clean[2])
            return
        dist.barrier()
        # rank 1 alone finds ONE element of what rank 0 sent it changed behind the wait
        fill(6)
        ch.push().wait()
        if rank == 1:
            rx.view(torch.int16)[4, 216 + 7] += 1         # row 4 of rank 0's block: its SECOND piece
        ch.verify()
        ack.exchange()
        raised = ""
        try:
            g.check()
        except Exception as e:                            # noqa: BLE001  (the text travels to the parent)
            raised = str(e)
        ret[rank] = (clean, g.exchange_mismatches(), g.timeouts(), raised, g.verifies, g.pushes)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_name_the_sender_and_the_piece(dev):
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(_two_rank_worker, args=(2, 33300 + os.getpid() % 500, ret), nprocs=2, join=True)
    print(dict(ret))
    for r in (0, 1):
        assert ret[r][0] != "timeout", ret[r]
        clean, log, timeouts, raised, verifies, pushes = ret[r]
        assert clean == (True, [], 0) and timeouts == 0, ret[r]
        assert verifies >= pushes > 0
    assert ret[0][1] == [] and ret[0][3] == ""
    log = ret[1][1]
    assert len(log) == 1, log
    e = log[0]
    assert (e["key"], e["sender"], e["piece"], e["buffer"], e["reread_matches"]) == (("vx", "two ranks"), 0, 1, "rx", 0), e
    assert e["got"][0] == (e["want"][0] + 1) % 2 ** 64
    assert "two ranks" in ret[1][3] and "piece 1 from rank 0" in ret[1][3]
