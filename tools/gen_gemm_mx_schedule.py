"""Emits the K-tile body of csrc/gemm_mx_v4.hip between its GENERATED markers: the 64 block-scaled MFMAs in the order of
csrc/gemm_fp8_v4.hip (phase 0 = W blocks 0..3 x A blocks 0..7, phase 1 = W blocks 4..7 x A blocks 0..7, A-major), its barriers
and fragment re-reads, and per K-tile 18 LDS-DMA pieces instead of 16: the 8 + 8 one-KiB code pieces and the two 256-byte
scale pieces (SPIECE) of a wave, each issued right behind the MFMA the table names.  Every fragment read carries the read of
its scale byte (the RAF / RWF / REREAD macros of the source), so the scale of a block retires with the block.
The e2m1-weight form of the kernel (FMT_W = MX_E2M1: 64-byte W rows) has a body of its own between the GENERATED-W4 markers:
the same MFMAs, barriers and re-reads with 14 pieces per K-tile -- 8 A, 4 W, 2 scale.  B2's count comes from each table.
The e2m3-activation forms (FMT_A = MX_E2M3: 96-byte rows, six one-KiB pieces per operand and wave) have two more, between the
GENERATED-A6 (e2m3 weights: 6 A, 6 W, 2 scale = 14 pieces) and GENERATED-A6W4 (e2m1 weights: 6 + 4 + 2 = 12) markers, and the
lengths of their tables are written between the GENERATED-PIECES markers as MX_PIECES_A6 / MX_PIECES_A6W4: the source's
prologue and tile-end waits (vmcnt) take them from there.
usage: python tools/gen_gemm_mx_schedule.py [--check]"""
import os

import generated_block

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bind_your_avatar_implementation_amd", "csrc",
                   "gemm_mx_v4.hip")
B1_AFTER = 9            # barrier B1 sits behind this MFMA (the shipped placement of gen_gemm_fp8_schedule.py)
B2_AFTER = 30
# MFMA behind which piece k is issued: code pieces A 0..7, W 0..7 where the fp8 kernel has them, then the A and the W scale piece
PIECES = list(range(10, 31, 3)) + list(range(32, 57, 3)) + [59, 62]
# ... of the e2m1-weight form: the A pieces where they are, the four W pieces spread over the slots the eight had
PIECES_W4 = list(range(10, 31, 3)) + [32] + list(range(35, 57, 6)) + [59, 62]
# ... of the e2m3-activation forms: six A pieces between B1 and B2, the six (e2m3) or four (e2m1) W pieces over phase 1
PIECES_A6 = list(range(10, 31, 4)) + list(range(32, 53, 4)) + [59, 62]
PIECES_A6W4 = list(range(10, 31, 4)) + list(range(32, 51, 6)) + [59, 62]
# A code pieces of a wave and K-tile by table; the W pieces follow, then the A and the W scale piece
N_A_OF = {id(PIECES): 8, id(PIECES_W4): 8, id(PIECES_A6): 6, id(PIECES_A6W4): 6}
N_W_OF = {id(PIECES): 8, id(PIECES_W4): 4, id(PIECES_A6): 6, id(PIECES_A6W4): 4}


def body(pieces=PIECES):
    N_A = N_A_OF[id(pieces)]
    n_w = len(pieces) - N_A - 2
    assert n_w == N_W_OF[id(pieces)] and len(pieces) == {id(PIECES): 18, id(PIECES_W4): 14, id(PIECES_A6): 14, id(PIECES_A6W4): 12}[id(pieces)]
    assert all(B1_AFTER < n < 64 for n in pieces) and pieces == sorted(pieces)
    out = ["            RWF(4, cWl, cWh, cSw);"]
    for n in range(64):
        phase, j, i = n >> 5, (n >> 2) & 7, (n & 3) + 4 * (n >> 5)
        line = f"            MFX({i}, {j});"
        if n < 3:
            line += f" RWF({5 + n}, cWl, cWh, cSw);"
        if n == B1_AFTER:
            line += " B1();"
        for k, at in enumerate(pieces):
            if at == n:
                if k < N_A + n_w:
                    line += f" PIECE({k - N_A if k >= N_A else k}, {'true' if k >= N_A else 'false'});"
                else:
                    line += f" SPIECE({'true' if k == N_A + n_w + 1 else 'false'});"
        if n == B2_AFTER:
            line += f" B2({sum(1 for at in pieces if at <= B2_AFTER)});"
        if n == 31:
            line += " REREAD_W();"
        if phase == 1 and (n & 3) == 3:
            line += f" REREAD_A({j});"
        out.append(line)
    return "\n".join(out)


if __name__ == "__main__":
    counts = f"constexpr int MX_PIECES_A6 = {len(PIECES_A6)}, MX_PIECES_A6W4 = {len(PIECES_A6W4)};"
    generated_block.main(HIP, body(), tagged={"-W4": body(PIECES_W4), "-A6": body(PIECES_A6), "-A6W4": body(PIECES_A6W4),
                                              "-PIECES": counts})
