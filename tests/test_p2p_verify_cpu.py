"""CPU: the exchange verification of the P2P engine (BYA_SP_VERIFY=all; include/bya.h defines checksum and record).  The
checksum restated in numpy -- and, chunk by chunk, the way the push kernel adds to it (csrc/comm.hip, p2p_copy_chunks<VERIFY>:
the word index of whatever a lane holds) -- and the host's descriptor builder (p2p.P2PGroup._build_verify_table) against a fake
group, in the style of tests/test_p2p_table_cpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bind_your_avatar_implementation_amd import p2p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = p2p.CHUNK
MOD = 65521


def checksum(words, first=0):
    """(A, B) of include/bya.h over the 16-bit words ``words``, the first of which has index ``first`` in its piece."""
    w = np.asarray(words, dtype=np.uint16).astype(np.uint64).reshape(-1)
    i = np.arange(first, first + w.size, dtype=np.uint64)
    return int(w.sum(dtype=np.uint64)), int((w * (i % np.uint64(MOD) + np.uint64(1))).sum(dtype=np.uint64))


def piece_words(t):
    """A tensor's elements in logical (row-major) order as 16-bit words."""
    return t.contiguous().view(torch.int16).reshape(-1).numpy().view(np.uint16)


class _FakeGroup:
    """Just enough of a P2PGroup for _build_table / _build_verify_table: named destination buffers in host memory, in the order
    they were 'allocated' (= their buf_id)."""
    _rows_of = staticmethod(p2p.P2PGroup._rows_of)
    _build_table = p2p.P2PGroup._build_table
    _build_verify_table = p2p.P2PGroup._build_verify_table

    def __init__(self, buffers, world):
        self.dev, self.world, self.verify = torch.device("cpu"), world, True
        self.ctrl = torch.zeros(4, dtype=torch.int32)
        self._bufs = buffers
        self._buf_ids = {name: i for i, name in enumerate(buffers)}

    def peers(self, name):
        return [p2p._Peer(t.data_ptr(), t.shape, t.dtype, t) for t in self._bufs[name]]


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "bya.h")).read()
    d = dict((m.group(1), m.group(2)) for m in re.finditer(r"#define BYA_P2P_VERIFY_(\w+) (.+)", src))
    assert (int(d["PIECES"]), int(d["REC_WORDS"]), int(d["BUFS"]), int(d["LOG_ENTRIES"])) == \
        (p2p.VERIFY_PIECES, p2p.REC_WORDS, p2p.VERIFY_BUFS, p2p.LOG_ENTRIES)
    assert p2p.LOG_WORDS == 16 + 16 * p2p.LOG_ENTRIES + p2p.VERIFY_PIECES * 32 * 4 and "16 + 16 * BYA_P2P_VERIFY_LOG_ENTRIES" in d["LOG_WORDS"]
    assert 2 + p2p.VERIFY_PIECES * p2p.REC_PIECE <= p2p.REC_WORDS // 2          # a record half holds the header and every piece


def test_checksum_is_order_independent_and_sees_a_shifted_row():
    rng = np.random.default_rng(0)
    w = rng.integers(0, 65536, size=200001, dtype=np.uint16)
    a, b = checksum(w)
    assert a == int(w.astype(object).sum()) % 2 ** 64
    assert b == sum(int(x) * (i % MOD + 1) for i, x in enumerate(w[:70000].tolist())) % 2 ** 64 + checksum(w[70000:], 70000)[1]
    # any cut into parts, added in any order, gives the same sums (what the chunk walk and the grid size do to them)
    cuts = sorted(rng.choice(np.arange(1, w.size), size=37, replace=False).tolist())
    parts = [(lo, hi) for lo, hi in zip([0] + cuts, cuts + [w.size])]
    rng.shuffle(parts)
    pa = sum(checksum(w[lo:hi], lo)[0] for lo, hi in parts) % 2 ** 64
    pb = sum(checksum(w[lo:hi], lo)[1] for lo, hi in parts) % 2 ** 64
    assert (pa, pb) == (a, b)
    # rows that landed at another pitch: the same words in another order -- A cannot tell, B does
    rows = w[:37 * 260].reshape(37, 260)
    shifted = np.roll(rows, 1, axis=0)
    assert checksum(shifted)[0] == checksum(rows)[0] and checksum(shifted)[1] != checksum(rows)[1]
    # the weights wrap at 65521 words: word 65521 weighs what word 0 does
    one = np.zeros(MOD + 2, dtype=np.uint16)
    one[MOD] = 7
    assert checksum(one) == (7, 7)
    one[MOD], one[MOD - 1] = 0, 7
    assert checksum(one) == (7, 7 * MOD)


def kernel_sums(table, n_rows, total_chunks, grid, read, world=1, rank=0):
    """What the VERIFY instances of the push kernel add to acc[entry]: per chunk of the walk, the words of the chunk with the
    word index the kernel computes for them (lg0 = row0 * row_bytes + col0; row r of a chunk of grouped rows starts r * row_bytes
    behind it).  ``read(addr, n)`` -> the n bytes at an address."""
    rows = table.tolist()
    share = -(-total_chunks // world)
    acc = [[0, 0] for _ in range(n_rows)]
    for b in range(grid):
        for it in range(b, share * world, grid):
            c = ((it + rank + 1) % world) * share + it // world
            if c >= total_chunks:
                continue
            i = 0
            while i + 1 < n_rows and rows[i + 1][6] <= c:
                i += 1
            src, _, row_bytes, nrow, sp, _, chunk0 = rows[i]
            if row_bytes <= 0 or nrow <= 0:
                continue
            ci = c - chunk0
            if row_bytes > CHUNK:
                cpr = -(-row_bytes // CHUNK)
                r0, col0 = divmod(ci, cpr)
                col0 *= CHUNK
                nr, n = 1, min(CHUNK, row_bytes - col0)
            else:
                rpc = CHUNK // row_bytes
                r0, col0 = ci * rpc, 0
                nr, n = min(rpc, nrow - r0), row_bytes
            lg0 = r0 * row_bytes + col0
            for r in range(nr):
                a, bb = checksum(np.frombuffer(read(src + (r0 + r) * sp + col0, n), dtype=np.uint16), (lg0 + r * n) // 2)
                acc[i][0] = (acc[i][0] + a) % 2 ** 64
                acc[i][1] = (acc[i][1] + bb) % 2 ** 64
    return acc


def _pieces_and_group():
    """The four pieces of the GPU test (tests/test_p2p_verify_gpu.py), one per branch of the copy loop, + a strided source."""
    torch.manual_seed(0)
    rnd = lambda *s: torch.randint(-32768, 32767, s, dtype=torch.int16)
    flat = rnd(4099).view(torch.bfloat16)                           # a 16-byte body and a 2-byte tail
    wide = rnd(37, 520).view(torch.bfloat16)                        # rows of 260 elements = 520 bytes, 1040 apart
    long_ = rnd(40000).view(torch.bfloat16)                         # one row of 80000 bytes: cut into two chunks
    odd = rnd(64)                                                   # 26 int16 from an odd word on
    bufs = {"r0": [torch.zeros(4104, dtype=torch.bfloat16)], "r1": [torch.zeros(37, 780, dtype=torch.bfloat16)],
            "r2": [torch.zeros(40000, dtype=torch.bfloat16)], "r3": [torch.zeros(64, dtype=torch.int16)]}
    pieces = [(flat, 0, "r0", 0), (wide[:, :260], 0, "r1", 12, 780), (torch.zeros(0, dtype=torch.bfloat16), 0, "r0", 0),
              (long_, 0, "r2", 0), (odd[1:27], 0, "r3", 3)]
    return pieces, _FakeGroup(bufs, 1), (flat, wide[:, :260], long_, odd[1:27])


@pytest.mark.parametrize("grid", [1, 5, 16])
def test_kernel_walk_adds_up_to_the_checksum_of_every_piece(grid):
    pieces, g, sent = _pieces_and_group()
    table, n, total_chunks, keep = g._build_table(pieces)
    assert n == 4 and total_chunks == 5
    mem = [(t.view(torch.int16).reshape(-1).numpy().view(np.uint8), t.data_ptr()) for t in (keep[0], keep[1]._base, keep[3], keep[4]._base)]

    def read(addr, nbytes):
        for arr, base in mem:
            if base <= addr and addr + nbytes <= base + arr.size:
                return arr[addr - base:addr - base + nbytes].tobytes()
        raise AssertionError("read outside every source")
    acc = kernel_sums(table, n, total_chunks, grid, read)
    for k, t in enumerate(sent):
        assert tuple(acc[k]) == checksum(piece_words(t)), k


def test_descriptors_carry_buf_id_and_receiver_relative_offsets():
    pieces, g, _ = _pieces_and_group()
    desc, counts, acc = g._build_verify_table(pieces)
    table = g._build_table(pieces)[0]
    assert desc.shape == (4, 4) and counts.tolist() == [4] and acc.shape == (4, 2) and acc.dtype == torch.int64 and not acc.any()
    # (destination rank, index in its record, buf_id = place in the allocation order, byte offset from the buffer's base)
    assert desc.tolist() == [[0, 0, 0, 0], [0, 1, 1, 24], [0, 2, 2, 0], [0, 3, 3, 6]]        # the empty piece is skipped
    for row, d in zip(table.tolist(), desc.tolist()):                                         # same entries, same order as the copy table
        name = list(g._bufs)[d[2]]
        assert row[1] == g._bufs[name][0].data_ptr() + d[3]
    assert table[1].tolist()[2:6] == [520, 37, 1040, 1560]                                    # strided source, pitched destination


def test_descriptors_count_pieces_per_peer_and_use_each_peers_own_base():
    world = 3
    a = [torch.zeros(8, 64, dtype=torch.bfloat16) for _ in range(world)]
    b = [torch.zeros(5 + j, 32, dtype=torch.bfloat16) for j in range(world)]                  # per peer: its own shape
    g = _FakeGroup({"__ctrl__": [torch.zeros(4, dtype=torch.int32)] * world, "a": a, "b": b}, world)
    src = torch.randn(4, 64).to(torch.bfloat16)
    pieces = [(src[0], 0, "a", 64), (src[:, :16], 2, "b", 32 + 8, 32), (src[1], 0, "a", 128), (torch.zeros(0, dtype=torch.bfloat16), 1, "a", 0),
              (src[2, :32], 2, "b", 0)]
    desc, counts, acc = g._build_verify_table(pieces)
    assert counts.tolist() == [2, 0, 2]
    assert desc.tolist() == [[0, 0, 1, 128], [2, 0, 2, 80], [0, 1, 1, 256], [2, 1, 2, 0]]
    # nothing to send at all: the place-holder entry of the copy table, a record without pieces for every peer
    desc, counts, acc = g._build_verify_table([(torch.zeros(0, dtype=torch.bfloat16), 1, "a", 0)])
    assert desc.tolist() == [[-1, 0, 0, 0]] and counts.tolist() == [0, 0, 0] and acc.shape == (1, 2)
    assert g._build_table([(torch.zeros(0, dtype=torch.bfloat16), 1, "a", 0)])[1] == 1


def test_more_pieces_than_a_record_holds_raise():
    g = _FakeGroup({"a": [torch.zeros(64, 8, dtype=torch.bfloat16)] * 2}, 2)
    src = torch.zeros(9, 8, dtype=torch.bfloat16)
    eight = [(src[k], 1, "a", 8 * k) for k in range(8)]
    assert g._build_verify_table(eight + [(src[8], 0, "a", 0)])[1].tolist() == [1, 8]         # 8 to one peer: the limit itself
    with pytest.raises(ValueError, match="more than 8 pieces for rank 1"):
        g._build_verify_table(eight + [(src[8], 1, "a", 64)])
    # an empty piece does not count
    assert g._build_verify_table(eight + [(torch.zeros(0, dtype=torch.bfloat16), 1, "a", 0)])[1].tolist() == [0, 8]


def test_solo_probe_groups_refuse_the_mode(monkeypatch):
    with pytest.raises(ValueError, match="solo probe"):
        p2p.P2PGroup(solo=(0, 2), verify=True)
    monkeypatch.setenv("BYA_SP_VERIFY", "all")
    assert p2p.verify_mode_from_env()
    with pytest.raises(ValueError, match="solo probe"):
        p2p.P2PGroup(solo=(1, 4))
    monkeypatch.setenv("BYA_SP_VERIFY", "1")                                                   # "1" keeps its meaning: the canary alone
    assert not p2p.verify_mode_from_env()


def test_entry_points_validate_before_they_launch():
    from bind_your_avatar_implementation_amd import _hip
    lib = _hip.load()
    base = 1 << 40
    assert lib.bya_p2p_verify(None, base, base, 2, 0, base, base, None) == -1
    assert lib.bya_p2p_verify(base, base, base, 2, 2, base, base, None) == -1                  # rank outside the group
    assert lib.bya_p2p_verify(base, base, base, 33, 0, base, base, None) == -1
    assert lib.bya_p2p_verify(base, base + 4, base, 2, 0, base, base, None) == -2              # records are 64-bit words
    assert lib.bya_p2p_verify(base + 128, base, base, 2, 0, base, base, None) == -1            # not a control block of this group
    assert lib.bya_p2p_verify(base, base, base, 2, 0, base + 256, base, None) == -1
    assert lib.bya_p2p_push_verified(base, 1, 1, base, 2, 0, base, None, base, base, base, None) == -1
    assert lib.bya_p2p_push_verified(base, 1, 1, base, 2, 0, base, base, base, base + 4, base, None) == -2
    assert lib.bya_p2p_exchange_verified(base, 1, 1, base, 2, 0, base, base, 0, base, base, base, None, None) == -1
    assert lib.bya_p2p_exchange_verified(base, 0, 1, base, 2, 0, base, base, 0, base, base, base, base, None) == -1
    assert ctypes.sizeof(ctypes.c_int64) * p2p.REC_WORDS * 32 * p2p.MAX_CHANNELS == 8 << 20    # the record buffer: 8 MiB per rank
