#!/usr/bin/env python3
"""Emit the hand-placed instruction stream of csrc/gemm_v5.hip (persistent 128x256 GEMM, one wave per SIMD, 64x128 per wave,
THREE-stage LDS ring): the K-tile variants of one output tile.  A K-tile is 64 MFMAs (v_mfma_f32_16x16x32_bf16, 16 cycles
each): MF(S, I, J) = acc[I][J] += W-fragment I x A-fragment J of 32-wide k-step S (MFZ: the same with C = 0).  Between them
go, at most one per MFMA gap, the "side" instructions:

  RA(1, j) / RW(1, i)   ds_read_b128 of the k-step-1 fragments of THIS K-tile (ring stage t % 3)
  SYNC()                every wave holds all fragments of K-tile t and K-tile t+1 has landed for everybody: ONE barrier
  DP(q)                 LDS-DMA piece q (0-3: A rows, 4-11: W rows) of K-tile t+3 into the stage this K-tile just left
  RA(0, j) / RW(0, i)   ds_read_b128 of the k-step-0 fragments of K-tile t+1 (stage (t + 1) % 3)
  NEXT()                s_waitcnt lgkmcnt(0), ring addresses advance one stage

Variants: A = first K-tile of an output tile (C = 0; its K-tile 1 was waited for in front of the previous epilogue, so SYNC
has no vmcnt wait), B = every other one (SYNC waits until only the 12 pieces of K-tile t+2 are in flight).  Edit the tables,
run the script: it rewrites the block between the GENERATED markers of csrc/gemm_v5.hip.
"""
import os
import re

import generated_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "bind_your_avatar_implementation_amd", "csrc", "gemm_v5.hip")

SYNC_AT = 27


def schedule(variant):
    side = {m: [] for m in range(64)}
    for j in range(4):
        side[j].append(f"RA_LOOP(1, {j});")
    for i in range(8):
        side[4 + 2 * i].append(f"RW_LOOP(1, {i});")
    side[SYNC_AT].append("SYNC_A();" if variant == "A" else "SYNC_B();")
    for q in range(12):
        side[SYNC_AT + 1 + 2 * q].append(f"DP({q});")
    reads = [f"RW_LOOP(0, {i});" for i in range(5)] + [f"RA_LOOP(0, {j});" for j in range(4)] + [f"RW_LOOP(0, {i});" for i in range(5, 8)]
    for n, r in enumerate(reads):
        side[SYNC_AT + 2 + 2 * n].append(r)
    side[63].append("NEXT();")
    # a fragment register may be re-loaded only behind the last MFMA that reads it (slot of MF(s, i, j) = 32 s + 4 i + j)
    for m in range(64):
        for ins in side[m]:
            mt = re.match(r"R([AW])_LOOP\((\d), (\d)\);", ins)
            if mt and mt.group(2) == "0":
                idx = int(mt.group(3))
                last = 28 + idx if mt.group(1) == "A" else 4 * idx + 3
                assert m > last, (ins, m, last)
    return side


def emit():
    out = []
    for v in "AB":
        side = schedule(v)
        out.append(f"        {'if' if v == 'A' else '} else if'} constexpr (V == '{v}') {{")
        for m in range(64):
            s, rest = divmod(m, 32)
            i, j = divmod(rest, 4)
            mf = "MFZ" if (v == "A" and s == 0) else "MF"
            out.append(f"            {mf}({s}, {i}, {j});" + ("  " + " ".join(side[m]) if side[m] else ""))
    out.append("        }")
    return "\n".join(out)


if __name__ == "__main__":
    generated_block.main(PATH, emit())
