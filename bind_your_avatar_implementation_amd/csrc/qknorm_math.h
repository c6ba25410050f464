// Arithmetic of the per-head q/k LayerNorm(64) + interleaved-pair RoPE (diffusers CogVideoXAttnProcessor2_0 +
// apply_rotary_emb; reference models/transformer.py:204-208), shared by its two homes so that they agree BIT FOR BIT:
//   * qknorm_rope_kernel (norm.hip): in place on the stored q / k, 8 lanes x 8 values per head row;
//   * the QKV projection's epilogue (gemm_v4.hip, QKN instance): on the accumulators, before q / k are stored at all.
// A head row is 64 values as eight groups g of 8 consecutive ones.  Every operation whose rounding depends on its order is
// spelled out here: sums go 8 values in sequence, then the tree (g ^ 1), (g ^ 2), (g ^ 4); products that feed an addition
// are explicit fmaf; nothing is left to -ffp-contract.
#pragma once
#include "bya_common.h"

__device__ __forceinline__ float qkn_sum8(const float (&v)[8]) {
    float s = v[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) s += v[e];
    return s;
}
// v[e] -= mean; returns sum of squares of the centred values (sequential, fused multiply-adds)
__device__ __forceinline__ float qkn_centre_sq8(float (&v)[8], float mean) {
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] -= mean;
        sq = __builtin_fmaf(v[e], v[e], sq);
    }
    return sq;
}
// centred values -> (x_hat * w + b), rotated by (cos, sin) where `rope` (a per-lane flag: branch-free, the rotation is
// computed for every lane and selected), times k_scale when it is not 1
__device__ __forceinline__ void qkn_finish8(float (&v)[8], float rstd, const float (&w)[8], const float (&b)[8], bool rope,
                                            const float (&cc)[8], const float (&ss)[8], float k_scale) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = __builtin_fmaf(v[e] * rstd, w[e], b[e]);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; e += 2) {   // pair (2i, 2i+1): rot = (-x[2i+1], x[2i])
        o[e] = __builtin_fmaf(v[e], cc[e], -(v[e + 1] * ss[e]));
        o[e + 1] = __builtin_fmaf(v[e + 1], cc[e + 1], v[e] * ss[e + 1]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = rope ? o[e] : v[e];
    if (k_scale != 1.0f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= k_scale;
    }
}

// ---- the score-bound statistics (include/bya.h: bya_qknorm_rope's `stats`, the *_stats entry points): the squared norm of a
// finished head row, taken from the bf16-ROUNDED values as they are stored.  One group's share: its 8 squares added in
// sequence (the square of a bf16 value is exact in fp32, so a fused multiply-add and a multiply + add give the same bits);
// the callers then add the groups by the tree (g ^ 1), (g ^ 2), (g ^ 4), like every other sum here.
__device__ __forceinline__ float qkn_norm2_8(const float (&r)[8]) {
    float n2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) n2 += r[e] * r[e];
    return n2;
}
// Maximum of a 32-bit pattern over the 16 lanes of a DPP row (lane & 15 = the MFMA layout's fr), in every lane of the row:
// quads, then quad pairs, then the row's two halves.  On bit patterns because that is what the table's atomic maximum compares
// (a non-negative float orders like its pattern, and a NaN row wins there as it does in the stand-alone kernel).
__device__ __forceinline__ uint32_t qkn_row16_umax(uint32_t x) {
    auto step = [](uint32_t v, uint32_t o) { return v > o ? v : o; };
    x = step(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true));     // quad_perm [1,0,3,2]
    x = step(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true));     // quad_perm [2,3,0,1]
    x = step(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true));    // row_half_mirror
    return step(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, true)); // row_mirror
}
// One no-return atomic maximum at agent scope (the stand-alone kernel's) on entry `tab[i]`; a zero raises nothing
__device__ __forceinline__ void qkn_stats_raise(unsigned* tab, long long i, uint32_t bits) {
    if (bits) (void)__hip_atomic_fetch_max(tab + i, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the rotary tables of the GEMM epilogues (epilogue_qkn, epilogue_mx_wide8_qkn, epilogue_mx_qkn): fp32 [M - text_rows, 64]
// cos and sin behind buffer descriptors, so that a row that is not rotated reads zeros from an out-of-range offset instead of
// taking a branch (hipcc can then keep the next row block's loads in flight under this one's arithmetic).
struct QknRotary {
    __amdgpu_buffer_rsrc_t cos, sin;
};
// ARGS: GemmArgs (M, qkn_text_rows, qkn_cos, qkn_sin).  CLAMP: tables of 2 GiB or more are cut at the descriptor's reach (the
// bf16 GEMM); the MX launcher refuses such a launch (mx_qkn_args), so its kernels do not carry the comparison.
template <bool CLAMP, class ARGS>
__device__ __forceinline__ QknRotary qkn_rotary(const ARGS& p) {
    const long long trows = (long long)p.M - p.qkn_text_rows;
    int tbytes;
    if constexpr (CLAMP) tbytes = trows > 0 && p.qkn_cos ? (int)(trows * 256 > 0x7fffffffLL ? 0x7fffffffLL : trows * 256) : 0;
    else tbytes = trows > 0 && p.qkn_cos ? (int)(trows * 256) : 0;
    return QknRotary{__builtin_amdgcn_make_buffer_rsrc((void*)p.qkn_cos, 0, tbytes, 0x00020000),
                     __builtin_amdgcn_make_buffer_rsrc((void*)p.qkn_sin, 0, tbytes, 0x00020000)};
}
// one token's eight cos and eight sin of a lane's eight columns: 16 bytes at byte offsets o0 and o1 of each table
// (0xffffffff: out of range, zeros)
struct QknRotary8 {
    float c[8], s[8];
};
__device__ __forceinline__ QknRotary8 qkn_rotary_load8(const QknRotary& r, uint32_t o0, uint32_t o1) {
    const f32x4 c0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r.cos, o0, 0, 0));
    const f32x4 c1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r.cos, o1, 0, 0));
    const f32x4 s0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r.sin, o0, 0, 0));
    const f32x4 s1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r.sin, o1, 0, 0));
    QknRotary8 t;
#pragma unroll
    for (int i = 0; i < 4; ++i) { t.c[i] = c0[i]; t.c[4 + i] = c1[i]; t.s[i] = s0[i]; t.s[4 + i] = s1[i]; }
    return t;
}
