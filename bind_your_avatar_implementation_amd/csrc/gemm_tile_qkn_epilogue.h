// The q/k-norm + RoPE epilogue on the lane layout of the 128 x 128 loop of gemm_fp8_kernel.h, which the tiled MX kernels
// (gemm_mx.hip) and the tiled fp8 kernel (gemm_fp8_kernel.h) both run: one copy for the two families.  The fp8 kernel has
// applied its row x channel scales to the accumulators before it calls this (gemm_fp8_body), the MX kernels' block scales
// are inside the instruction.
#pragma once
#include "gemm_common.h"
#include "qknorm_math.h"

namespace {

// ---- the q/k-norm epilogue (bya_gemm_mx_qkv_norm_rope): the packed q|k|v projection with the per-head q/k LayerNorm(64) +
// RoPE of bya_qknorm_rope on its accumulators (reference models/transformer.py:204-208), bit for bit bya_gemm_mx_mixed(...,
// n_split) followed by bya_qknorm_rope.  Arithmetic: qknorm_math.h, whose eight groups g of a head row are 8 consecutive
// columns each.  Here a lane (fr, fq) holds columns 16 i + 4 fq .. + 3 of its wave in acc[i][j]: a head is the fragments
// i = 4 h .. 4 h + 3, group g sits in fragment g >> 1 in the lane pair fq = 2 (g & 1), 2 (g & 1) + 1.  qkn_sum8 and
// qkn_centre_sq8 run sequentially over a group's eight values, so a lane's own partial sum would round differently: the pair
// trades its four values instead.  v_permlane16_swap of a register with itself leaves the EVEN lane's value in the first
// result and the ODD lane's in the second, in both lanes -- the values in column order.  What is traded is
// bf16(acc + bias), the value the two-launch path stored and read back, two to a register: two swaps per fragment.  Both
// lanes then evaluate the group's sum; the tree is (g ^ 1) = lane ^ 32 (v_permlane32_swap), (g ^ 2) = the lane's fragments
// i ^ 1, (g ^ 4) = i ^ 2 -- same operands per addition as the stand-alone kernel (an addition does not depend on the order of
// its two operands).  qkn_finish8 is element-wise and the RoPE pairs (2 i, 2 i + 1) lie inside four columns.  q, k or v is
// decided per head (width % 64 == 0), wave-uniformly: a wave or a tile may straddle q | k or k | v; v heads and heads past N
// take the plain bias epilogue (epilogue_block's arithmetic and 8-byte stores).
// Stores, STORE16: after the trade the pair holds the eight columns twice, so the even lane finishes and stores fragments
// 4 h, 4 h + 2 and the odd lane 4 h + 1, 4 h + 3, 16 bytes each; else every lane finishes its own four columns of every
// fragment and stores 8 bytes.  The same number of finished values, table loads and bytes either way.
// Rotary rows come through buffer descriptors: rows that are not rotated read zeros from an out-of-range offset, no branch.
#ifndef BYA_MX_QKN_STORE16
#define BYA_MX_QKN_STORE16 1
#endif
template <int NI, int MI, bool STORE16>
__device__ __forceinline__ void epilogue_mx_qkn(const GemmArgs& p, int z, int m_base, int n_wave, int fq,
                                                const f32x4 (&acc)[NI][MI]) {
    static_assert(NI % 4 == 0, "whole heads per wave");
    constexpr int NH = NI / 4;
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p.C + (long long)z * p.c_bs), 0, 0x7fffffff, 0x00020000);
    const QknRotary rot = qkn_rotary<false>(p);                    // (the launcher keeps the tables below 2 GiB)
    const bool has_bias = p.bias != nullptr;
    const bool odd = fq & 1;
    auto colbytes = [&](int n) {
        return ((uint32_t)(n / p.n_split) * (uint32_t)p.c_split_stride + (uint32_t)(n % p.n_split)) * 2u;
    };
    // the lane's two finished pieces k = 0, 1 of a head: columns hc[k] .. + 7 (STORE16), or hc[k] .. + 3 and hc[k] + 16 .. + 19
    int hc[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) hc[k] = STORE16 ? 16 * (2 * k + (fq & 1)) + 8 * (fq >> 1) : 32 * k + 4 * fq;
    auto load8 = [&](const bf16_t* src, int k) {
        if constexpr (STORE16) return *reinterpret_cast<const u32x4*>(src + hc[k]);
        else {
            const u32x2 a = *reinterpret_cast<const u32x2*>(src + hc[k]), b = *reinterpret_cast<const u32x2*>(src + hc[k] + 16);
            return u32x4{a[0], a[1], b[0], b[1]};
        }
    };
    // Head by head, rows inside: one head's parameters and bias are live at a time, and a finished head's accumulators are
    // dead (the 256 x 256 tile has 128 of them per lane and two heads per wave: rows outside spilled).  The price is that its
    // second head reads the rotary rows again, from L2.
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int n_head = n_wave + 64 * h;
        const int tsel = n_head / p.qkn_width;                      // 0 = q, 1 = k, else v or past N: wave-uniform
        u32x2 bv[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int n4 = n_head + 16 * f + 4 * fq;
            bv[f] = has_bias ? *reinterpret_cast<const u32x2*>(p.bias + (n4 < p.N ? n4 : 0)) : u32x2{0u, 0u};
        }
        if (tsel < 2) {
            const float ks = tsel == 1 ? p.qkn_kscale : 1.0f;
            u32x4 wq[2], bq[2];
            uint32_t colb[2][2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                wq[k] = load8(p.qkn_w[tsel], k);
                bq[k] = load8(p.qkn_b[tsel], k);
                colb[k][0] = colbytes(n_head + hc[k]);
                colb[k][1] = colbytes(n_head + hc[k] + 16);
            }
#pragma unroll
            for (int j = 0; j < MI; ++j) {
                const int m = m_base + 16 * j;
                const bool mok = m < p.M;
                const uint32_t coff = (mok ? (uint32_t)m : 0u) * (uint32_t)(p.ldc * 2);
                const bool rope = mok && m >= p.qkn_text_rows;
                QknRotary8 cs[2];
                const uint32_t t0 = (uint32_t)(m - p.qkn_text_rows) * 256u;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint32_t o0 = rope ? t0 + (uint32_t)hc[k] * 4u : 0xffffffffu;
                    const uint32_t o1 = rope ? o0 + (STORE16 ? 16u : 64u) : 0xffffffffu;
                    cs[k] = qkn_rotary_load8(rot, o0, o1);
                }
                float v[4][8];                                      // group g = 2 f + (fq >> 1) of the head row, in column order
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    // bf16(acc + bias): the projection as the two-launch path stored it, one rounding
                    const f32x4 a = acc[4 * h + f][j];
                    const uint32_t r0 = pack2bf(a[0] + bflo(bv[f][0]), a[1] + bfhi(bv[f][0]));
                    const uint32_t r1 = pack2bf(a[2] + bflo(bv[f][1]), a[3] + bfhi(bv[f][1]));
                    const auto s0 = lane_pair16(r0), s1 = lane_pair16(r1);
                    unpack8(u32x4{s0[0], s1[0], s0[1], s1[1]}, v[f]);
                }
                float s[4];
#pragma unroll
                for (int f = 0; f < 4; ++f) s[f] = lane_add32(qkn_sum8(v[f]));
                const float mean = ((s[0] + s[1]) + (s[2] + s[3])) * (1.0f / 64);
#pragma unroll
                for (int f = 0; f < 4; ++f) s[f] = lane_add32(qkn_centre_sq8(v[f], mean));
                const float rstd = rsqrtf(((s[0] + s[1]) + (s[2] + s[3])) * (1.0f / 64) + p.qkn_eps);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    float u[8], w8[8], b8[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if constexpr (STORE16) u[e] = odd ? v[2 * k + 1][e] : v[2 * k][e];
                        else u[e] = odd ? v[2 * k + (e >> 2)][4 + (e & 3)] : v[2 * k + (e >> 2)][e & 3];
                    }
                    unpack8(wq[k], w8);
                    unpack8(bq[k], b8);
                    qkn_finish8(u, rstd, w8, b8, rope, cs[k].c, cs[k].s, ks);
                    const u32x4 o = pack8(u);
                    if constexpr (STORE16) {
                        __builtin_amdgcn_raw_buffer_store_b128(o, rsC, mok ? coff + colb[k][0] : 0xffffffffu, 0, 0);
                    } else {
                        __builtin_amdgcn_raw_buffer_store_b64(u32x2{o[0], o[1]}, rsC, mok ? coff + colb[k][0] : 0xffffffffu, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b64(u32x2{o[2], o[3]}, rsC, mok ? coff + colb[k][1] : 0xffffffffu, 0, 0);
                    }
                }
            }
        } else {
            // v, or columns past N: epilogue_block's arithmetic (alpha = 1, no activation) and stores
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const int n4 = n_head + 16 * f + 4 * fq;
                const uint32_t colb = n4 < p.N ? colbytes(n4) : 0xffffffffu;
#pragma unroll
                for (int j = 0; j < MI; ++j) {
                    const int m = m_base + 16 * j;
                    const f32x4 a = acc[4 * h + f][j];
                    u32x2 o;
                    o[0] = pack2bf(a[0] + bflo(bv[f][0]), a[1] + bfhi(bv[f][0]));
                    o[1] = pack2bf(a[2] + bflo(bv[f][1]), a[3] + bfhi(bv[f][1]));
                    __builtin_amdgcn_raw_buffer_store_b64(o, rsC, (m < p.M && n4 < p.N) ? (uint32_t)m * (uint32_t)(p.ldc * 2) + colb : 0xffffffffu, 0, 0);
                }
            }
        }
    }
}

}  // namespace
