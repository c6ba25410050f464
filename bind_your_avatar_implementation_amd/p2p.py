"""P2P exchange engine, host side: the exchanges of the sharded denoise step as PUSH kernels that store straight into
the peers' HBM over xGMI (``bya_p2p_push`` / ``bya_p2p_wait`` / ``bya_p2p_exchange``, csrc/comm.hip, include/bya.h).

The reference has no inference parallelism; BASELINE.json asks for it.  Round 3 issued every
exchange through ``torch.distributed`` (RCCL): ~360 collectives per rank-step at ~20 us each, none of which can be
captured in a hipGraph on this stack.  Here an exchange is ONE ordinary kernel launch whatever its scatter/gather list,
and the whole sharded step replays as a graph.

``P2PGroup(group, device, mem)``    one per process group; collective (every rank constructs it at the same point).
                                    ``mem`` = kind of the RECEIVE buffers: "coarse" (ordinary device memory, cached in the
                                    L2s, made coherent by the acquire at the end of every wait) or "fine" (fine-grained:
                                    coherent by construction, slower to read).  The control block (flags a running kernel
                                    polls while peers store into them) is fine-grained whenever the platform hands it out.
``.symmetric(name, shape, dtype)``  a buffer every rank allocates under the same name: returns the local tensor; the peers'
                                    copies are mapped into this process through hipIpc (torch's CUDA storage sharing for
                                    coarse memory, ``bya_p2p_ipc_*`` for the other kinds); handles traded ONCE over the
                                    process group (any backend: gloo works)
``.channel(key, pieces)``          the channel (control block, sequence counters) of the logical exchange ``key``, bound to
                                    the copy table of ``pieces`` = [(src, peer, name, offset)], "copy the contiguous local
                                    tensor ``src`` to element ``offset`` of buffer ``name`` on rank ``peer``"; one table per
                                    set of source addresses (workspaces change, captured graphs own theirs)
``Channel.exchange()``             push + wait as ONE launch on the current stream
``Channel.push(side) / .wait()``   the two halves (``side``: the push runs on the group's side stream behind the work
                                    already enqueued; call ``.wait()`` where the data is needed)
``.poison(out)``                   last launch of a sharded step: NaN over ``out`` if any wait of this group ever gave up
``P2PGroup(verify=True)``          (BYA_SP_VERIFY=all) a diagnostic mode: every exchange carries per-piece checksums to the
                                    receiver, which sums its own receive buffers behind the wait (``Channel.verify``) and logs
                                    exchange, sender and piece of whatever differs (``.exchange_mismatches()``, ``.check()``)

All ranks of the group must issue the same sequence of ``symmetric`` calls and, per channel, the same sequence of
exchanges (sequence numbers live in device memory, one pair per channel).  One process per GPU in production; the tests
run several processes on ONE GPU -- hipIpc maps a peer's buffer of the same device just the same.
"""
import collections
import ctypes
import os
import weakref

import torch
import torch.distributed as dist

from . import _hip

MAX_CHANNELS = 256
CTRL_WORDS = 64
CHUNK = 64 * 1024
KINDS = {"coarse": 0, "fine": 1, "uncached": 2}
TABLES_PER_CHANNEL = 4           # copy tables kept per channel besides the ones a captured graph owns
LIVE_GROUPS = weakref.WeakSet()  # every P2PGroup of this process (ops.check_gemm_workspace asks each for timed-out waits)
_RETIRED = []                    # buffers of closed groups (P2PGroup.close: never freed while peers might still store into them)
# exchange verification (BYA_SP_VERIFY=all; BYA_P2P_VERIFY_* of include/bya.h)
VERIFY_PIECES, VERIFY_BUFS, REC_WORDS, REC_PIECE = 8, 1024, 128, 7
LOG_ENTRIES, LOG_ENTRY0, LOG_ENTRY = 64, 16, 16
LOG_WORDS = LOG_ENTRY0 + LOG_ENTRY * LOG_ENTRIES + VERIFY_PIECES * 32 * 4
LOG_KINDS = {0: "sums differ", 1: "no record of this sequence number", 2: "record names memory outside the receiver's buffers"}


def verify_mode_from_env():
    """BYA_SP_VERIFY=all: every exchange of every group is verified (``P2PGroup(verify=None)`` asks here)."""
    return os.environ.get("BYA_SP_VERIFY", "0") == "all"


def _piece_rows(grp, pieces):
    """The non-empty pieces of a ``_build_table`` list as (source address, peer, buffer name, byte offset in that buffer, row
    bytes, rows, source pitch, destination pitch -- bytes), checked against the destination buffer."""
    out = []
    for piece in pieces:
        src, peer, name, offset = piece[:4]
        if src.numel() == 0:
            continue
        es = src.element_size()
        nrows, ncols, spitch = grp._rows_of(src)
        dpitch = piece[4] if len(piece) > 4 and piece[4] is not None else ncols
        if len(piece) > 4 and piece[4] is not None and nrows == 1 and src.dim() >= 2 and src.shape[0] > 1:
            # a contiguous source scattered to pitched destination rows: its leading dimension is the row index
            nrows, ncols = src.shape[0], src[0].numel()
            spitch = ncols
        dst_t = grp.peers(name)[peer]
        last = offset + (nrows - 1) * dpitch + ncols
        if dst_t.dtype != src.dtype or offset < 0 or last > dst_t.numel() or dpitch < ncols:
            raise ValueError(f"P2P piece does not fit buffer {name!r} on rank {peer}")
        dst = dst_t.data_ptr() + offset * es
        if (src.data_ptr() | dst | (ncols * es) | (spitch * es) | (dpitch * es)) & 1:
            raise ValueError("P2P pieces must be 2-byte aligned in address and size")
        out.append((src.data_ptr(), peer, name, offset * es, ncols * es, nrows, spitch * es, dpitch * es))
    return out


class PhaseMismatch(RuntimeError):
    """The ranks of a group were not at the same point of a collective set-up (see ``gather_tagged``)."""


def gather_tagged(group, world, tag, value):
    """``all_gather_object`` of ``value`` with a tag that names the point of the set-up the caller is at.  Object
    collectives pair up by ORDER, not by meaning: a rank that raised locally between two of them (and went on to the
    caller's next collective) would silently pair that one with its peers' previous one -- from then on everybody reads
    somebody else's answers.  With the tag every rank sees the slip in the SAME collective and raises ``PhaseMismatch``;
    ``parallel.shard_sequence`` (the only caller that survives a failed set-up) then repeats its own gather once, which
    pairs with the gather its peers reach after THEIR raise: the ranks are in step again."""
    got = [None] * world
    dist.all_gather_object(got, (tag, value), group=group)
    tags = [g[0] for g in got]
    if any(t != tag for t in tags):
        raise PhaseMismatch(f"ranks at different points of the set-up: {tags}")
    return [g[1] for g in got]


class _FineUnavailable(RuntimeError):
    """This platform (or one rank of the group) did not hand out fine-grained / uncached device memory."""


class _Block:
    """Device memory from ``bya_p2p_alloc`` (or a peer's, mapped by ``bya_p2p_ipc_import``) as an object torch can wrap."""

    def __init__(self, ptr, nbytes, mine):
        self.ptr, self.nbytes, self.mine = ptr, nbytes, mine
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    def release(self):
        lib = _hip.load()
        if self.ptr:
            (lib.bya_p2p_free if self.mine else lib.bya_p2p_ipc_release)(self.ptr)
            self.ptr = 0


class _Peer:
    """What the copy tables need of a peer's buffer: where it is mapped here, how big it is, what it holds."""

    def __init__(self, ptr, shape, dtype, keep=None):
        self._ptr, self.shape, self.dtype, self._keep = ptr, tuple(shape), dtype, keep
        n = 1
        for s in self.shape:
            n *= s
        self._n = n

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n


class Channel:
    """One exchange of the step: a control block (flags + device-resident sequence counters) and, per set of source
    pointers it has been used with, a device-resident copy table.  The engine re-allocates its workspace when the geometry
    changes and gives every captured hipGraph a workspace of its own: the SAME logical exchange then comes with other
    source addresses -- it keeps its channel (and its sequence numbers, which all ranks advance in step) and gets one more
    table.  A table keeps its source tensors alive; tables bound during a stream capture stay for good (the graph holds their
    address), of the others only the ``TABLES_PER_CHANNEL`` most recently used ones are kept, so a server that moves between
    geometries does not pin every workspace it ever had."""

    def __init__(self, grp, index):
        self.grp, self.index = grp, index
        self.ctrl_ptr = grp.ctrl[index].data_ptr()
        self.peer_ctrl = torch.tensor([grp.ctrl_peers[j].data_ptr() + index * CTRL_WORDS * 4 for j in range(grp.kworld)],
                                      dtype=torch.int64, device=grp.dev)
        self.tables = collections.OrderedDict()      # source-pointer signature -> [table, n_copies, total_chunks, sources, pinned, verify tables]
        self.cur = None
        self._join = None
        if grp.verify:                               # where this channel's records go on every peer (include/bya.h)
            self.peer_rec = torch.tensor([grp.peers("__verify_rec__")[j].data_ptr() + index * 32 * REC_WORDS * 8 for j in range(grp.kworld)],
                                         dtype=torch.int64, device=grp.dev)

    def bind(self, pieces):
        sig = tuple((p[0].data_ptr(), p[1], p[2], p[3], tuple(p[0].shape), p[0].stride(), p[4] if len(p) > 4 else None) for p in pieces)
        ent = self.tables.get(sig)
        if ent is None:
            # (verify mode: the descriptors first -- a pair with too many pieces raises before anything is kept)
            vt = self.grp._build_verify_table(pieces) if self.grp.verify else None
            ent = self.tables[sig] = list(self.grp._build_table(pieces)) + [False, vt]
        else:
            self.tables.move_to_end(sig)
        if torch.cuda.is_current_stream_capturing():
            ent[4] = True
        loose = [k for k, e in self.tables.items() if not e[4]]
        for k in loose[:max(0, len(loose) - TABLES_PER_CHANNEL)]:
            if k != sig:
                del self.tables[k]
        self.cur = ent
        return self

    def _launch(self, fn, stream, wait=False):
        g = self.grp
        table, n, total_chunks = self.cur[:3]
        tail = (g.ctrl.data_ptr(), g.wait_limit_ms) if wait else ()     # the group's first control block, this launch's wait limit
        if g.verify:                                                    # the instance that also sums and writes the records
            tail += tuple(t.data_ptr() for t in self.cur[5]) + (self.peer_rec.data_ptr(),)
        _hip.check(fn(table.data_ptr(), n, total_chunks, self.peer_ctrl.data_ptr(), g.kworld, g.krank, self.ctrl_ptr, *tail,
                      stream.cuda_stream), fn.__name__)
        g.pushes += 1

    def push(self, side=False):
        g = self.grp
        cur = torch.cuda.current_stream(g.dev)
        stream = cur
        if side and (g.world > 1 or g.solo is not None):
            stream = g.side_stream
            ev = torch.cuda.Event()
            ev.record(cur)
            stream.wait_event(ev)
        lib = _hip.load()
        self._launch(lib.bya_p2p_push_verified if g.verify else lib.bya_p2p_push, stream)
        self._join = None
        if stream is not cur:
            self._join = torch.cuda.Event()
            self._join.record(stream)
        return self

    def wait(self):
        g = self.grp
        cur = torch.cuda.current_stream(g.dev)
        if self._join is not None:
            cur.wait_event(self._join)              # (also rejoins the side stream into a graph capture)
            self._join = None
        _hip.check(_hip.load().bya_p2p_wait(self.ctrl_ptr, g.kworld, g.ctrl.data_ptr(), g.wait_limit_ms, cur.cuda_stream), "bya_p2p_wait")
        return self.verify() if g.verify else self

    def exchange(self):
        """push + wait in one launch (``P2PGroup.MERGED = False``: as two, the round-4 form); verify mode: + the verify launch."""
        if not self.grp.MERGED:
            return self.push().wait()
        lib = _hip.load()
        self._launch(lib.bya_p2p_exchange_verified if self.grp.verify else lib.bya_p2p_exchange, torch.cuda.current_stream(self.grp.dev),
                     wait=True)
        return self.verify() if self.grp.verify else self

    def verify(self):
        """Verify mode: enqueue ``bya_p2p_verify`` on the current stream -- every piece the last exchange this channel has
        WAITED for brought into this rank's buffers is summed again, as a consumer would read it, and compared with its
        sender's record (``P2PGroup.exchange_mismatches``).  ``exchange()`` and ``wait()`` end with it; calling it again
        repeats the check on what the buffers hold now.  No host synchronisation: it is captured with the step."""
        g = self.grp
        if not g.verify:
            raise RuntimeError("P2P exchange verification is off for this group (BYA_SP_VERIFY=all, or P2PGroup(verify=True))")
        import sys
        ops = sys.modules.get(__package__ + ".ops")          # (the timers live there; a bucket of its own)
        tok = ops._begin("bya_p2p_verify") if ops is not None else None
        _hip.check(_hip.load().bya_p2p_verify(self.ctrl_ptr, g.vrec[self.index].data_ptr(), g.buf_bases.data_ptr(), g.kworld, g.krank,
                                              g.ctrl.data_ptr(), g.vlog.data_ptr(), torch.cuda.current_stream(g.dev).cuda_stream),
                   "bya_p2p_verify")
        if tok is not None:
            ops._end(tok)
        g.verifies += 1
        return self

    def records(self):
        """Verify mode, diagnostics (synchronises): per sender rank the record of the last exchange this channel has waited
        for, {"sequence", "pieces": [{"buf_id", "buffer", "dst_byte_offset", "row_bytes", "rows", "dst_pitch", "A", "B"}]}."""
        g = self.grp
        torch.cuda.synchronize(g.dev)
        seq = int(g.ctrl[self.index, 33].item()) & 0xFFFFFFFF
        rec = g.vrec[self.index, :g.kworld].cpu().view(g.kworld, 2, REC_WORDS // 2)[:, seq & 1]
        names = {i: n for n, i in g._buf_ids.items()}
        out = []
        for s in range(g.kworld):
            r = rec[s].tolist()
            ps = [dict(zip(("buf_id", "dst_byte_offset", "row_bytes", "rows", "dst_pitch", "A", "B"), r[2 + k * REC_PIECE:2 + (k + 1) * REC_PIECE]))
                  for k in range(max(0, min(r[1], VERIFY_PIECES)))]
            for p_ in ps:
                p_["buffer"] = names.get(p_["buf_id"])
                p_["A"], p_["B"] = p_["A"] & (2 ** 64 - 1), p_["B"] & (2 ** 64 - 1)
            out.append({"sequence": r[0], "pieces": ps})
        return out


class P2PGroup:
    MERGED = True

    def __init__(self, group=None, device=None, mem="coarse", solo=None, verify=None):
        """``verify`` (None: BYA_SP_VERIFY=all): VERIFY MODE, a diagnostic -- every exchange of this group, whoever issues it,
        carries per-piece checksums from the sender to the receiver, which sums what it reads from its own receive buffers
        behind the wait and compares (``Channel.verify``, ``exchange_mismatches``, ``check``; include/bya.h defines the
        checksum and the record).  Collective like everything else here: every rank of the group the same.
        ``solo=(rank, world)``: PROBE MODE (tools/solo_rank_step.py) -- this one process plays rank ``rank`` of a
        ``world``-rank group whose other ranks do not exist: every "peer" buffer is a second local allocation, pushes store
        into those, and a wait only expects this rank's own flag.  The received data is therefore wrong (the peers' parts
        never arrive) but every kernel and every exchange launch of ONE rank's step runs with its real shapes: what one GPU
        can measure of an N-GPU step.  Never used by the product path."""
        self.solo = solo
        self.verify = verify_mode_from_env() if verify is None else bool(verify)
        if self.verify and solo is not None:
            raise ValueError("P2P exchange verification (BYA_SP_VERIFY=all) on a solo probe group: the peers' parts never arrive, "
                             "what it receives is wrong by construction")
        if solo is not None:
            self.group, (self.rank, self.world) = None, solo
        else:
            self.group = group if group is not None else dist.group.WORLD
            self.world, self.rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        if self.world > 32:
            raise ValueError("P2P exchange engine: at most 32 ranks (one node)")
        if mem not in KINDS:
            raise ValueError(f"P2P memory kind {mem!r}: expected one of {sorted(KINDS)}")
        self.mem = mem
        # what the kernels are told: the group's size and this rank -- in solo mode a 1-rank group whose only flag is word 0
        self.kworld, self.krank = (1, 0) if solo is not None else (self.world, self.rank)
        self.dev = torch.device(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
        self._named = {}
        self._buf_ids = {}               # name -> place in the order of the ``symmetric`` calls (collective: the same on every rank)
        self._keep = []
        self._channels = {}
        self._p2p_enabled = set()
        self.pushes = 0
        self.verifies = 0                # verify launches (verify mode: one per exchange, one per push / wait pair)
        if self.verify:
            # buf_id -> (local base address, bytes): what a record's (buf_id, offset) means on THIS rank; the mismatch log
            self.buf_bases = torch.zeros(VERIFY_BUFS, 2, dtype=torch.int64, device=self.dev)
            self.vlog = torch.zeros(LOG_WORDS, dtype=torch.int64, device=self.dev)
        self.closed = False
        self.side_stream = torch.cuda.Stream(self.dev)
        # seconds a wait of THIS group may take before it gives up (wall clock); handed to every wait / exchange launch -- a
        # launch captured into a hipGraph keeps the limit it was captured with
        self.wait_limit_ms = int(float(os.environ.get("BYA_P2P_TIMEOUT", "30")) * 1000)
        # the control block: peers store flags into it while this GPU's wait kernels poll them -> fine-grained memory
        # where the platform hands it out (RCCL allocates its flags that way for the same reason); coarse otherwise
        try:
            self.ctrl = self.symmetric("__ctrl__", (MAX_CHANNELS, CTRL_WORDS), torch.int32, zero=True, kind="fine")
            self.ctrl_kind = "fine"
        except _FineUnavailable:
            self.ctrl = self.symmetric("__ctrl__", (MAX_CHANNELS, CTRL_WORDS), torch.int32, zero=True, kind="coarse")
            self.ctrl_kind = "coarse"
        if solo is not None:
            self.ctrl_kind = f"local (solo probe, {getattr(self, 'solo_ctrl', 'coarse')})"
        self.ctrl_peers = self._named["__ctrl__"][1]
        if self.verify:
            # the records: written by the peers' push kernels, read by this rank's verify kernels -- like the flags, fine-grained
            # memory where the platform hands it out
            shape = (MAX_CHANNELS, 32, REC_WORDS)
            try:
                self.vrec = self.symmetric("__verify_rec__", shape, torch.int64, zero=True, kind="fine")
            except _FineUnavailable:
                self.vrec = self.symmetric("__verify_rec__", shape, torch.int64, zero=True, kind="coarse")
        LIVE_GROUPS.add(self)

    def _agree(self, err, what):
        """COLLECTIVE: every rank reports how its local part of ``what`` went; if any rank failed, ALL raise.  Ranks must never
        part ways inside the set-up (one in a barrier, another already in the caller's next collective: a hang on RCCL), so
        every step that can fail on one rank alone ends here."""
        errs = [err]
        if self.world > 1 and self.solo is None:
            errs = gather_tagged(self.group, self.world, ("agree", what), None if err is None else str(err))
        bad = [(j, e) for j, e in enumerate(errs) if e is not None]
        if bad:
            raise RuntimeError(f"P2P exchange engine, {what}: failed on rank(s) {bad}")

    def close(self):
        """Retire the group (a rung of the transport ladder that did not pass, or a model that is re-sharded): its sticky
        time-out counters no longer count for ``ops.check_gemm_workspace``, its copy tables go.  The buffers are kept for the
        life of the process ON PURPOSE -- a peer that fell behind may still store into them, and memory handed back to the
        allocator would be somebody else's by then.  What that pins: everything the rung had allocated -- for a sharded
        42-layer model ~0.5 GB of receive buffers per rank, the self-test's W x 256 KB, ``exchange_probe``'s 2 x W x 6 MB --
        once per rung LEFT (at most two per process: the ladder has three rungs), of 288 GB."""
        LIVE_GROUPS.discard(self)
        for ch in self._channels.values():
            ch.tables.clear()
            ch.cur = None
        _RETIRED.append((self._named, self._keep))
        self.closed = True

    # ---- symmetric buffers -------------------------------------------------------------------------------------------
    def symmetric(self, name, shape, dtype=torch.bfloat16, zero=False, kind=None):
        """COLLECTIVE on first use of ``name`` (every rank, same order).  -> local tensor; ``peers(name)[j]`` = rank j's
        buffer mapped here, in rank j's OWN shape (shapes may differ between ranks: uneven shards)."""
        ent = self._named.get(name)
        if ent is not None:
            loc = ent[0]
            if tuple(loc.shape) != tuple(shape) or loc.dtype != dtype:
                raise ValueError(f"symmetric buffer {name!r} exists with shape {tuple(loc.shape)} {loc.dtype}")
            return loc
        kind = kind or self.mem
        with torch.cuda.device(self.dev):
            if self.solo is not None:
                # (bf16 receive buffers start as gaussian noise, not zeros: the peers' parts never arrive, and kernels that
                # multiply zeros draw less power and clock higher than they would on a node)
                local = (torch.randn(*shape, device=self.dev) * 0.5).to(dtype) if dtype == torch.bfloat16 else \
                    torch.zeros(*shape, dtype=dtype, device=self.dev)
                if name == "__ctrl__" and kind == "fine":
                    # the control block in the memory kind a node would use (polls and counters cost more there): the probe
                    # should pay for it too.  Falls back to the torch allocation above where the platform refuses.
                    n = local.numel() * local.element_size()
                    ptr = ctypes.c_void_p(0)
                    if _hip.load().bya_p2p_alloc(n, KINDS["fine"], ctypes.byref(ptr)) == 0 and ptr.value:
                        blk = _Block(ptr.value, n, True)
                        self._keep.append(blk)
                        local = torch.as_tensor(blk, device=self.dev).view(dtype).view(*shape)
                        self.solo_ctrl = "fine"
                if name == "__ctrl__":
                    peers = [_Peer(local.data_ptr(), shape, dtype, local)] * self.world     # every flag lands in the own block
                else:
                    sinks = [torch.zeros(*shape, dtype=dtype, device=self.dev) for _ in range(self.world - 1)]
                    peers = [_Peer(t.data_ptr(), shape, dtype, t) for t in sinks]
                    peers.insert(self.rank, _Peer(local.data_ptr(), shape, dtype, local))
                self._named[name] = (local, peers)
                self._register(name, local)
                return local
            # (both end in _agree: nobody pushes before everybody has mapped, and a rank that could not map takes all down with it)
            local, peers = (self._symmetric_torch if kind == "coarse" else self._symmetric_ext)(shape, dtype, zero, kind)
        self._named[name] = (local, peers)
        self._register(name, local)
        return local

    def _register(self, name, local):
        """The buffer's ``buf_id`` (its place in the order of the ``symmetric`` calls) and, in verify mode, its entry in the
        device table the verify kernel resolves a record's (buf_id, offset) with."""
        i = self._buf_ids[name] = len(self._buf_ids)
        if self.verify:
            if i >= VERIFY_BUFS:
                raise RuntimeError(f"P2P exchange verification: more than {VERIFY_BUFS} symmetric buffers in one group")
            self.buf_bases[i] = torch.tensor([local.data_ptr(), local.numel() * local.element_size()], dtype=torch.int64)

    def _symmetric_torch(self, shape, dtype, zero, kind):
        # the WHOLE allocation is what a peer maps, and it must stay alive for as long as any peer may store into it
        # (= the life of this object)
        local = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self.dev)
        torch.cuda.synchronize(self.dev)
        peers = [None] * self.world
        peers[self.rank] = _Peer(local.data_ptr(), shape, dtype, local)
        if self.world > 1:
            info, err = None, None
            try:
                info = local.untyped_storage()._share_cuda_()
            except Exception as e:                      # noqa: BLE001  (no hipIpc export on this platform)
                err = f"_share_cuda_: {e!r}"
            infos = gather_tagged(self.group, self.world, "handles (torch)", (info, local.storage_offset(), tuple(shape)))
            try:
                for j, (inf, off, shp) in enumerate(infos):
                    if j == self.rank or err is not None or inf is None:
                        continue
                    st = torch.UntypedStorage._new_shared_cuda(*inf)
                    # (the mapped storage carries the OWNER's device index; only its address is used, by kernels of this GPU)
                    t = torch.empty(0, dtype=dtype, device=st.device).set_(st, off, shp)
                    if st.device != self.dev and (self.dev.index, st.device.index) not in self._p2p_enabled:
                        # one process sees several GPUs (torchrun without per-rank visibility): a kernel of THIS GPU may only
                        # dereference the peer's memory once peer access is enabled; torch does that on the first P2P copy
                        probe = torch.empty(1, dtype=dtype, device=self.dev)
                        probe.copy_(t.reshape(-1)[:1])
                        self._p2p_enabled.add((self.dev.index, st.device.index))
                    peers[j] = _Peer(t.data_ptr(), shp, dtype, (st, t))
            except Exception as e:                      # noqa: BLE001  (a peer's handle does not open here)
                err = f"mapping a peer's buffer: {e!r}"
            self._keep.append(local)
            self._agree(err, "mapping the peers' receive buffers (hipIpc through torch)")
        return local, peers

    def _symmetric_ext(self, shape, dtype, zero, kind):
        """Fine-grained / uncached memory: ``bya_p2p_alloc`` (zero-filled), handles by ``bya_p2p_ipc_export / import``.  Every
        rank reports whether it got its memory BEFORE anybody maps anything, so a refusal raises on all ranks together."""
        lib = _hip.load()
        n = 1
        for s in shape:
            n *= s
        nbytes = max(n * torch.empty(0, dtype=dtype).element_size(), 16)
        ptr, handle, err = ctypes.c_void_p(0), (ctypes.c_ubyte * 64)(), None
        rc = lib.bya_p2p_alloc(nbytes, KINDS[kind], ctypes.byref(ptr))
        if rc != 0 or not ptr.value:
            err = f"bya_p2p_alloc({kind}) -> {_hip.ERRORS.get(rc, rc)}"
        elif self.world > 1:
            rc = lib.bya_p2p_ipc_export(ptr, handle)
            if rc != 0:
                err = f"bya_p2p_ipc_export -> {_hip.ERRORS.get(rc, rc)}"
        local = None
        if err is None:
            try:
                blk = _Block(ptr.value, nbytes, True)
                local = torch.as_tensor(blk, device=self.dev)[:n * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(*shape)
                self._keep.append(blk)
            except Exception as e:                      # noqa: BLE001  (torch without the array interface on this platform)
                err = f"torch.as_tensor over device memory: {e!r}"
        infos = [(err, bytes(handle), tuple(shape))]
        if self.world > 1:
            infos = gather_tagged(self.group, self.world, f"handles ({kind})", (err, bytes(handle), tuple(shape)))
        bad = [(j, i[0]) for j, i in enumerate(infos) if i[0] is not None]
        if bad:
            if ptr.value and local is None:
                lib.bya_p2p_free(ptr)
            raise _FineUnavailable(f"{kind} device memory unavailable on rank(s) {bad}")
        peers = [None] * self.world
        peers[self.rank] = _Peer(local.data_ptr(), shape, dtype, local)
        err = None
        for j, (_, h, shp) in enumerate(infos):
            if j == self.rank or err is not None:
                continue
            p = ctypes.c_void_p(0)
            rc = lib.bya_p2p_ipc_import((ctypes.c_ubyte * 64).from_buffer_copy(h), ctypes.byref(p))
            if rc != 0 or not p.value:
                err = f"bya_p2p_ipc_import of rank {j}'s buffer -> {_hip.ERRORS.get(rc, rc)}"
                continue
            blk = _Block(p.value, 0, False)
            self._keep.append(blk)
            peers[j] = _Peer(p.value, shp, dtype, blk)
        self._agree(err, f"mapping the peers' {kind} buffers (bya_p2p_ipc_import)")
        return local, peers

    def peers(self, name):
        return self._named[name][1]

    def has(self, name):
        return name in self._named

    # ---- channels ------------------------------------------------------------------------------------------------------
    def channel(self, key, pieces):
        """The channel of the logical exchange ``key`` (created on first use: every rank, same order), bound to ``pieces`` =
        [(contiguous local tensor, peer rank, receive-buffer name, element offset there)]."""
        ch = self._channels.get(key)
        if ch is None:
            if len(self._channels) >= MAX_CHANNELS:
                raise RuntimeError("P2P exchange engine: out of channels")
            ch = self._channels[key] = Channel(self, len(self._channels))
        return ch.bind(pieces)

    @staticmethod
    def _rows_of(src):
        """A piece's source as (rows, row elements, row pitch in elements): any contiguous tensor is one row; otherwise a view
        whose trailing dimensions are dense behind ONE strided leading dimension (e.g. ``x[:, a:b]`` of a [P, L, F] tensor)."""
        if src.is_contiguous():
            return 1, src.numel(), src.numel()
        inner = src[0]
        if not inner.is_contiguous():
            raise ValueError("P2P piece sources must be contiguous, or dense rows behind one strided leading dimension")
        return src.shape[0], inner.numel(), src.stride(0)

    def _build_table(self, pieces):
        """pieces: (src, peer, name, offset) or (src, peer, name, offset, dst_pitch): ``src`` lands at element ``offset`` of
        rank ``peer``'s buffer ``name``; a strided source (see ``_rows_of``) and / or ``dst_pitch`` (elements between the
        starts of consecutive rows at the destination; default: dense) make it a 2-D piece."""
        rows, chunk0 = [], 0
        for src_ptr, peer, name, dst_off, row_bytes, nrows, spitch, dpitch in _piece_rows(self, pieces):
            rows.append((src_ptr, self.peers(name)[peer].data_ptr() + dst_off, row_bytes, nrows, spitch, dpitch, chunk0))
            if row_bytes > CHUNK:
                chunk0 += nrows * ((row_bytes + CHUNK - 1) // CHUNK)
            else:
                rpc = CHUNK // row_bytes
                chunk0 += (nrows + rpc - 1) // rpc
        if not rows:                                     # nothing to send: still takes part in the flag protocol
            rows, chunk0 = [(self.ctrl.data_ptr(), self.ctrl.data_ptr(), 0, 0, 0, 0, 0)], 1
        table = torch.tensor(rows, dtype=torch.int64, device=self.dev)
        return table, len(rows), chunk0, [p[0] for p in pieces]      # (the sources stay alive with the table)

    def _build_verify_table(self, pieces):
        """Verify mode: what the push kernel needs besides the copy table of ``pieces`` (same entries, same order) to write the
        records of include/bya.h -- per entry (destination rank, index of the piece in that rank's record, buf_id of the
        destination buffer = its place in the group's ``symmetric`` order, byte offset from that buffer's base ON THE RECEIVER),
        the pieces per destination rank, and the accumulator of the sums.  A pair with more than ``VERIFY_PIECES`` pieces is an
        error: nothing is ever left out of a record silently."""
        counts, rows = [0] * self.world, []
        for _, peer, name, dst_off, _, _, _, _ in _piece_rows(self, pieces):
            if counts[peer] == VERIFY_PIECES:
                raise ValueError(f"P2P exchange verification: more than {VERIFY_PIECES} pieces for rank {peer} in one exchange "
                                 f"(a record holds {VERIFY_PIECES})")
            rows.append((peer, counts[peer], self._buf_ids[name], dst_off))
            counts[peer] += 1
        if not rows:
            rows = [(-1, 0, 0, 0)]                       # (the copy table's place-holder entry)
        return (torch.tensor(rows, dtype=torch.int64, device=self.dev), torch.tensor(counts, dtype=torch.int64, device=self.dev),
                torch.zeros(len(rows), 2, dtype=torch.int64, device=self.dev))

    def drop_tables(self):
        """Forget every copy table no captured graph owns (the engine calls this when it lets go of a workspace)."""
        for ch in self._channels.values():
            for k in [k for k, e in ch.tables.items() if not e[4]]:
                del ch.tables[k]
            ch.cur = None

    # ---- health ----------------------------------------------------------------------------------------------------------
    def self_test(self, rounds=12, elems=64 * 1024):
        """``rounds`` all-to-alls of ``elems`` int32 per peer INTO THE SAME receive buffer, payload changing every round, every
        word checked, with the consumer's reads (which leave the buffer's lines in this GPU's caches) and an acknowledging
        exchange between two pushes -- the re-use pattern of the step, where a stale line shows if remote stores are not seen.
        Alternates the one-launch and the two-launch form.  Raises if anything differs or a wait gave up.  Run once at set-up,
        so that a platform where peer stores do not arrive (or arrive late) is noticed before the first step."""
        W, n = self.world, elems
        recv = self.symmetric("__selftest__", (W, n), torch.int32, zero=True)
        send = torch.zeros(W, n, dtype=torch.int32, device=self.dev)
        ramp = torch.arange(n, dtype=torch.int32, device=self.dev)
        data = self.channel("__selftest__", [(send[j], j, "__selftest__", self.rank * n) for j in range(W)])
        empty = torch.zeros(0, dtype=torch.int32, device=self.dev)
        ack = self.channel("__selftest_ack__", [(empty, j, "__selftest__", 0) for j in range(W)])
        src = torch.arange(W, dtype=torch.int32, device=self.dev)[:, None]
        bad = torch.zeros((), dtype=torch.int64, device=self.dev)
        keep_limit, self.wait_limit_ms = self.wait_limit_ms, 2000                      # a dead link shows in seconds, not minutes
        try:
            for it in range(rounds):
                for j in range(W):
                    send[j] = ramp * (it + 1) + (self.rank * 64 + j) * 1000003 + it * 7919
                if it % 2:
                    data.push().wait()
                else:
                    data.exchange()
                want = ramp[None, :] * (it + 1) + (src * 64 + self.rank) * 1000003 + it * 7919
                bad += (recv != want).sum()                  # the consumer: reads every word through the ordinary cache path
                ack.exchange()                               # "consumed": peers may overwrite the buffer from here on
                if it % 4 == 3 and self.timeouts():          # (synchronises) nothing arrives: do not sit through every round
                    break
        finally:
            self.wait_limit_ms = keep_limit
        torch.cuda.synchronize(self.dev)
        err = None
        if self.timeouts() or int(bad.item()):
            err = (f"self-test: {int(bad.item())} stale or missing words, {self.timeouts()} timed-out waits "
                   f"({self.mem} receive buffers, {self.ctrl_kind} flags)")
        self._agree(err, "self-test")                    # (all ranks pass or all ranks raise; also the closing barrier)

    def exchange_probe(self, mbytes_per_peer=6, reps=5):
        """COLLECTIVE diagnostic (bench.py --gpus N puts it into its line): time an all-to-all of ``mbytes_per_peer`` MB to
        every rank (the size of the packed q|k|v exchange of an 8-rank step is 5 MB per peer) as ONE exchange launch.
        -> {"bytes_sent": to the W - 1 peers, "us": per exchange on this rank, "GBps_out": bytes_sent / us}.  On a node this is
        the first number anyone gets for what the push kernel does to the xGMI links; with the ranks on one GPU it measures
        local copies."""
        W, n = self.world, int(mbytes_per_peer * (1 << 20)) // 2
        self.symmetric("__probe__", (W, n), torch.bfloat16)
        send = torch.zeros(W, n, dtype=torch.bfloat16, device=self.dev)
        ch = self.channel("__probe__", [(send[j], j, "__probe__", self.rank * n) for j in range(W)])
        for _ in range(2):
            ch.exchange()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            ch.exchange()
        e.record()
        torch.cuda.synchronize(self.dev)
        us = s.elapsed_time(e) / reps * 1e3
        sent = (W - 1) * n * 2
        return {"bytes_sent": sent, "us": round(us, 1), "GBps_out": round(sent / us * 1e-3, 1)}

    def timeouts(self):
        """Waits that gave up (0 on a healthy run); synchronises."""
        torch.cuda.synchronize(self.dev)
        return int(self.ctrl[:, 35].sum().item())

    def mismatches(self):
        """Steps whose gathered prediction differed between the ranks (``SeqShard.verify_gathered``; 0 on a healthy run); synchronises."""
        torch.cuda.synchronize(self.dev)
        return int(self.ctrl[0, 38].item())

    def exchange_mismatches(self):
        """Verify mode: the pieces that did not arrive as they were sent (at most the first ``LOG_ENTRIES``; [] on a healthy
        run, and with the mode off); synchronises.  One dict per piece: ``key`` = the key its channel was created with (e.g.
        ("seq", "h2r", S, Tt)), ``channel`` its index, ``sender`` rank, ``piece`` = index among the pieces that sender sends this
        rank in that exchange (-1: no record of that sequence number arrived), ``buffer`` name, ``sequence`` number, ``want`` =
        (A, B) of the sender's record, ``got`` = what this rank summed through its caches, ``reread_matches`` = 1 if a second
        pass with system-scope loads summed to ``want`` (memory holds what was sent; the first pass read something else), 0 if
        not (memory itself differs), -1 where nothing was read, and ``kind`` (``LOG_KINDS``)."""
        if not self.verify:
            return []
        torch.cuda.synchronize(self.dev)
        log = self.vlog[:LOG_ENTRY0 + LOG_ENTRY * LOG_ENTRIES].cpu().tolist()
        keys = {ch.index: k for k, ch in self._channels.items()}
        names = {i: n for n, i in self._buf_ids.items()}
        u64 = 2 ** 64 - 1
        out = []
        for e in range(min(log[0], LOG_ENTRIES)):
            ch, sender, seq, piece, wa, wb, ga, gb, reread, buf_id, _, kind = log[LOG_ENTRY0 + e * LOG_ENTRY:][:12]
            out.append({"key": keys.get(ch), "channel": ch, "sender": sender, "piece": piece, "buffer": names.get(buf_id),
                        "sequence": seq, "want": (wa & u64, wb & u64), "got": (ga & u64, gb & u64), "reread_matches": reread,
                        "kind": LOG_KINDS.get(kind, kind)})
        return out

    def exchange_mismatch_count(self):
        """Verify mode: pieces that did not arrive as sent, ALL of them (the log keeps the first ``LOG_ENTRIES``); synchronises."""
        torch.cuda.synchronize(self.dev)
        return int(self.ctrl[0, 40].item())

    def check(self):
        """Raise if any wait of this group ever gave up (its consumers ran on a stale receive buffer), a step's exchange
        checksum differed between the ranks, or (verify mode) a piece of an exchange did not arrive as it was sent."""
        x = self.exchange_mismatch_count() if self.verify else 0
        if x:
            e = self.exchange_mismatches()[0]
            raise _hip.ByaError(f"{x} piece(s) of P2P exchanges did not arrive as sent (BYA_SP_VERIFY=all); the first: exchange {e['key']!r} "
                                f"(channel {e['channel']}), sequence number {e['sequence']}, piece {e['piece']} from rank {e['sender']} in "
                                f"buffer {e['buffer']!r}: {e['kind']}, sent sums {e['want']}, read {e['got']}, reread_matches = "
                                f"{e['reread_matches']} -- results of this run are not to be trusted")
        m = self.mismatches()
        if m:
            raise _hip.ByaError(f"{m} step(s) ended with DIFFERENT gathered predictions on the ranks of this group (exchange checksum, "
                                f"BYA_SP_VERIFY): a receive buffer was read stale -- results of this run are not to be trusted")
        n = self.timeouts()
        if n:
            raise _hip.ByaError(f"{n} P2P wait(s) timed out (a peer's push did not arrive within the limit, BYA_P2P_TIMEOUT): "
                                f"results of this run are not to be trusted")

    def poison(self, out):
        """Enqueue ``bya_p2p_poison``: ``out`` (bf16) becomes NaN if any channel of this group carries a time-out, a step
        checksum that differed between the ranks, or (verify mode) a piece that did not arrive as sent."""
        assert out.dtype == torch.bfloat16 and out.is_contiguous()
        _hip.check(_hip.load().bya_p2p_poison(self.ctrl.data_ptr(), MAX_CHANNELS, out.data_ptr(), out.numel(),
                                              torch.cuda.current_stream(self.dev).cuda_stream), "bya_p2p_poison")
        return out

