"""CPU restatement of the q/k score-bound statistics (include/bya.h: bya_qknorm_rope's ``stats``, the *_stats entry points), shared
by tests/test_qkn_stats_cpu.py (which pins it on fp64) and tests/test_qkn_stats_gpu.py (which holds the kernels to it bit for
bit).  Not a test module."""
import numpy as np
import torch


def row_norm2(rows):
    """rows: bf16 tensor [..., heads * 64] of STORED q or k rows -> float32 numpy [..., heads], the squared norm of every head
    row in the kernels' order: float32 throughout; per group of 8 consecutive columns the 8 squares added in sequence (a
    square of a bf16 value is exact in float32); then the eight group sums as ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))."""
    assert rows.dtype == torch.bfloat16 and rows.shape[-1] % 64 == 0
    x = rows.detach().float().cpu().numpy().astype(np.float32)
    x = x.reshape(*x.shape[:-1], x.shape[-1] // 64, 8, 8)
    sq = x * x
    s = sq[..., 0]
    for e in range(1, 8):
        s = (s + sq[..., e]).astype(np.float32)
    pair = [(s[..., 2 * g] + s[..., 2 * g + 1]).astype(np.float32) for g in range(4)]
    return (((pair[0] + pair[1]).astype(np.float32)) + ((pair[2] + pair[3]).astype(np.float32))).astype(np.float32)


def table(q, k):
    """q, k: bf16 [batch, rows, heads * 64] as stored -> float32 tensor [2, batch * heads]: per (batch, head) the maximum over
    the rows of ``row_norm2``, q's line first -- what ``stats.amax(0)`` must hold, bit for bit."""
    return torch.from_numpy(np.stack([row_norm2(t).max(axis=-2).reshape(-1) for t in (q, k)]))


def bits32(t):
    """fp32 tensor -> its bit patterns (the comparisons on the table are on bits: no tolerance, and -0 / NaN are told apart)."""
    return t.detach().cpu().contiguous().view(torch.int32)
