"""Emits the K-tile body of csrc/gemm_mx_v4.hip between its GENERATED markers: the 64 block-scaled MFMAs in the order of
csrc/gemm_fp8_v4.hip (phase 0 = W blocks 0..3 x A blocks 0..7, phase 1 = W blocks 4..7 x A blocks 0..7, A-major), its barriers
and fragment re-reads, and per K-tile 18 LDS-DMA pieces instead of 16: the 8 + 8 one-KiB code pieces and the two 256-byte
scale pieces (SPIECE) of a wave, each issued right behind the MFMA the table names.  Every fragment read carries the read of
its scale byte (the RAF / RWF / REREAD macros of the source), so the scale of a block retires with the block.
The e2m1-weight form of the kernel (FMT_W = MX_E2M1: 64-byte W rows) has a body of its own between the GENERATED-W4 markers:
the same MFMAs, barriers and re-reads with 14 pieces per K-tile -- 8 A, 4 W, 2 scale.  B2's count comes from each table.
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
N_A = 8                 # A code pieces of a wave and K-tile (both forms); the W pieces follow, then the A and the W scale piece


def body(pieces=PIECES):
    n_w = len(pieces) - N_A - 2
    assert (pieces is PIECES and n_w == 8) or (pieces is PIECES_W4 and n_w == 4 and len(pieces) == 14)
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
    generated_block.main(HIP, body(), tagged={"-W4": body(PIECES_W4)})
