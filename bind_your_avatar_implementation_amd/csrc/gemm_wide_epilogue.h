// The 16-byte ("wide") epilogues of the persistent one-wave-per-SIMD bf16 GEMM kernels: gemm_v4.hip (256 x 256 tiles, a wave
// owns 128 x 128: NJ = 8 row blocks) and gemm_v5.hip / gemm_v6.hip (128 x 256 tiles, a wave owns 64 x 128: NJ = 4).  They stage
// the W rows of a wave's 128-column span in the permuted order that makes a lane's eight accumulator tiles i = 0..7 hold
// EIGHT CONSECUTIVE output columns (the LDS image: top of gemm_persistent.h).
#pragma once
#include "gemm_persistent.h"
#include "qknorm_math.h"
#include <type_traits>

namespace {

// Wide epilogue of one wave.  The lane (fr = lane & 15, fq = lane >> 4) holds, for row block j and accumulator register e,
// the EIGHT consecutive columns  n8 = n_wave + (4 e + fq) * 8 + i,  i = 0..7  in acc[i][j][e]  (W rows are staged in the
// permuted order of gemm_persistent.h), of row  m = m_wave + 16 j + fr.  Per element the expression of epilogue_block
// (gemm_common.h), which the tiled kernels evaluate.  The one copy for every persistent kernel; two compile-time switches:
//   * SCALED (gemm_fp8_v4.hip): the accumulator is first multiplied by its activation-row x weight-channel scale,
//     sa[batch * M] x sw[N]; not so for bf16 and for MX, whose block scales are inside the instruction;
//   * PIN (gemm_mx_v4.hip, whose instance takes a non-const acc): the accumulators stay in their AGPRs until the row blocks of
//     a burst are due -- an asm that takes them as "+a" at the head of the burst makes every earlier copy of them pointless.
//     Without it hipcc's allocator opened that kernel's epilogue with over a hundred v_accvgpr_read at once (as many
//     accumulators as VGPRs were free at that point) and then sent two lane constants to scratch.
// Split tiles (see the top).  A slab holds a tile's partial sums in the order this epilogue walks the accumulators:
// unit (wave, j, e, half) = the lane's values i = 4 half .. 4 half + 3 of row block j, register e: 16 bytes per lane at
// ((wave * 64 + (j * 4 + e) * 2 + half) * 64 + lane) * 16, so that one store instruction writes eight whole 128-byte lines.
// raw_out != null: this workgroup is a WRITER -- its accumulators go to that slab with write-through (sc1) stores and
// nothing else happens.  Same call site as the ordinary epilogue and through one VALU multiply: a second kind of consumer
// of the asm-owned accumulators (a plain store of them) made hipcc put the store's data tuples into AGPRs too and evict
// accumulators to scratch right behind their last MFMA, inside the K-loop -- 250 registers of scratch traffic per tile.
template <int ACT, int JB, bool SPLIT, bool CONV = false, int NJ = 8, bool PIN = false, bool SCALED = false>
__device__ __forceinline__ void epilogue_wide(const GemmArgs& p, int z, int m_wave, int n_wave, int fr, int fq,
                                              std::conditional_t<PIN, f32x4, const f32x4> (&acc)[8][NJ], int wave, int lane,
                                              float* raw_out = nullptr, const float* __restrict__ sa = nullptr,
                                              const float* __restrict__ sw = nullptr) {
    const bool has_res = p.res != nullptr, has_gate = p.gate0 != nullptr, has_bias = p.bias != nullptr;
    const bool has_rs = p.bias_rowscale != nullptr;
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((has_res ? p.res : p.C) + (long long)z * p.res_bs), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.C + (long long)z * p.c_bs), 0, 0x7fffffff, 0x00020000);
    const char* g0base = reinterpret_cast<const char*>(p.gate0 + (long long)z * p.gate_bs);
    const char* g1base = reinterpret_cast<const char*>(p.gate1 + (long long)z * p.gate_bs);
    u32x4 bv[4], g0[4], g1[4];
    f32x4 wv[4][2];                                              // SCALED: the eight channel scales of each column group
    uint32_t ncb[4], colb[4];
    bool nok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n8 = n_wave + (4 * e + fq) * 8;
        nok[e] = n8 < p.N;                                       // N % 8 == 0 on this kernel's shapes (checked by the launcher)
        ncb[e] = nok[e] ? (uint32_t)n8 * 2u : 0u;
        colb[e] = (uint32_t)n8 * 2u;
        if (p.n_split > 0) colb[e] = ((uint32_t)(n8 / p.n_split) * (uint32_t)p.c_split_stride + (uint32_t)(n8 % p.n_split)) * 2u;
        bv[e] = has_bias ? *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(p.bias) + ncb[e]) : u32x4{0u, 0u, 0u, 0u};
        if constexpr (SCALED) {
            wv[e][0] = *reinterpret_cast<const f32x4*>(sw + (nok[e] ? n8 : 0));
            wv[e][1] = *reinterpret_cast<const f32x4*>(sw + (nok[e] ? n8 : 0) + 4);
        }
        if (has_gate) {
            g0[e] = *reinterpret_cast<const u32x4*>(g0base + ncb[e]);
            g1[e] = *reinterpret_cast<const u32x4*>(g1base + ncb[e]);
        }
    }
#pragma unroll
    for (int jb = 0; jb < NJ; jb += JB) {
        u32x4 rv[JB][4];
        float rs[JB], ra[JB];
        bool mok[JB];
        uint32_t roff[JB], coff[JB];
        if constexpr (PIN) {
#pragma unroll
            for (int jj = 0; jj < JB; ++jj)
#pragma unroll
                for (int i = 0; i < 8; ++i) asm volatile("" : "+a"(acc[i][jb + jj]));
        }
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            const int m = m_wave + 16 * (jb + jj) + fr;
            mok[jj] = m < p.M;
            uint32_t mc = mok[jj] ? (uint32_t)m : 0u;
            if constexpr (CONV) {
                // row m = padded pixel (t, h, w) of the output grid [To, Hp, Wp]: kept if it is a real pixel, and then stored
                // (and its residual read) at row (t H + h) W + w of the unpadded output
                const uint32_t plane = (uint32_t)(p.conv_Hp * p.conv_Wp);
                const uint32_t t = mc / plane, rem = mc - t * plane;
                const uint32_t h = rem / (uint32_t)p.conv_Wp, w = rem - h * (uint32_t)p.conv_Wp;
                mok[jj] = mok[jj] && h < (uint32_t)p.conv_H && w < (uint32_t)p.conv_W && t < (uint32_t)p.conv_To;
                mc = mok[jj] ? (t * (uint32_t)p.conv_H + h) * (uint32_t)p.conv_W + w : 0u;
            }
            rs[jj] = has_rs ? p.bias_rowscale[(long long)z * p.M + mc] : 1.0f;
            if constexpr (SCALED) ra[jj] = sa[(long long)z * p.M + mc];
            // 32-bit byte offsets behind descriptors of 0x7fffffff records, as in every bf16 epilogue here: the host cuts a launch
            // whose C or residual rows span 2 GiB into row chunks (gemm_row_chunks, gemm_common.h) before it gets here
            roff[jj] = mc * (uint32_t)(p.ldres * 2);
            coff[jj] = mc * (uint32_t)(p.ldc * 2);
            if (has_res) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    rv[jj][e] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                        rsR, (mok[jj] && nok[e]) ? roff[jj] + ncb[e] : 0xffffffffu, 0, 0));
            }
        }
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            const int j = jb + jj;
            const int m = m_wave + 16 * j + fr;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float b8[8], v[8], a0[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if constexpr (SCALED) a0[i] = acc[i][j][e] * (ra[jj] * wv[e][i >> 2][i & 3]);     // row x channel scale
                    else a0[i] = acc[i][j][e];
                }
                if (SPLIT && raw_out) {
                    const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc((void*)raw_out, 0, (int)GEMM_WS_SLAB_BYTES, 0x00020000);
                    const uint32_t so = (uint32_t)(((wave * 64 + (j * 4 + e) * 2) * 64 + lane) * 16);
                    // the values pass through one VALU multiply by an opaque 1.0: stored as they are, hipcc put the store's
                    // data tuples into AGPRs too and evicted accumulators to scratch inside the K-loop to make room
                    float one = 1.0f;
                    asm volatile("" : "+s"(one));
                    const f32x4 lof = {a0[0] * one, a0[1] * one, a0[2] * one, a0[3] * one};
                    const f32x4 hif = {a0[4] * one, a0[5] * one, a0[6] * one, a0[7] * one};
                    const u32x4 lo = __builtin_bit_cast(u32x4, lof), hi = __builtin_bit_cast(u32x4, hif);
                    __builtin_amdgcn_raw_buffer_store_b128(lo, rsS, so, 0, 16 /* sc1 */);
                    __builtin_amdgcn_raw_buffer_store_b128(hi, rsS, so + 1024, 0, 16 /* sc1 */);
                    continue;
                }
                unpack8(bv[e], b8);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = p.alpha * apply_act<ACT>(fmaf(rs[jj], b8[i], a0[i]), p.leaky);
                if (has_gate) {
                    float g8[8];
                    unpack8(m < p.gate_split ? g0[e] : g1[e], g8);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] *= g8[i];
                }
                if (has_res) {
                    float r8[8];
                    unpack8(rv[jj][e], r8);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] += r8[i];
                }
                __builtin_amdgcn_raw_buffer_store_b128(pack8(v), rsC, (mok[jj] && nok[e]) ? coff[jj] + colb[e] : 0xffffffffu, 0, 0);
            }
        }
    }
}

// The packed q|k|v projection's epilogue with the per-head q/k LayerNorm(64) + RoPE inside (QKN instance; reference
// models/transformer.py:204-208 = diffusers CogVideoXAttnProcessor2_0: norm_q / norm_k, apply_rotary_emb on the video rows).
// Round 4 wrote q, k and launched bya_qknorm_rope on them: 473 MB of traffic per layer against 218 MB if q and k are written
// once.  In the wide epilogue's layout a lane (fr, fq) holds, for row block j, the eight consecutive columns
// n_wave + (4 e + fq) * 8 + i: the wave's 128 columns are two heads, head hh = registers e = 2 hh, 2 hh + 1, and a head row is
// spread over the FOUR lanes fq = 0 .. 3 of one fr -- group g = 4 (e & 1) + fq of qknorm_math.h's eight.  The tree (g ^ 1),
// (g ^ 2), (g ^ 4) is therefore lane ^ 16, lane ^ 32, then the lane's own two registers: same operands, same order, same bits
// as the stand-alone kernel.  The projection is rounded to bf16 first (the value the two-launch path stored and read back).
// v tiles (n_wave >= 2 width) take the plain bias epilogue.
// STATS (the *_stats entry points; an instance of its own, the plain one keeps its instruction stream): the launch also records
// the score-bound statistics of bya_qknorm_rope -- per finished q / k head row the squared norm of the values AS STORED
// (pack8, unpack8), group by group (qkn_norm2_8) and by the same tree, so the same bits as the stand-alone kernel's.  Rows
// past M count as 0.  Nothing touches memory per row: a lane keeps the maximum over its NJ row blocks in one register per
// head, qkn_row16_umax takes it over the 16 rows of a block, and lane 0 issues ONE atomic maximum per (wave, head, tile) --
// the stand-alone kernel issues one per (row, head).  Slot = workgroup % slots, as there.
template <int NJ = 8, bool STATS = false>
__device__ __forceinline__ void epilogue_qkn(const GemmArgs& p, int z, int m_wave, int n_wave, int fr, int fq, const f32x4 (&acc)[8][NJ]) {
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p.C + (long long)z * p.c_bs), 0, 0x7fffffff, 0x00020000);
    const int tsel = n_wave / p.qkn_width;                       // 0 = q, 1 = k, 2 = v (a tile never straddles: width % 128 == 0)
    const bool has_bias = p.bias != nullptr;
    u32x4 bv[4];
    uint32_t colb[4];
    bool nok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n8 = n_wave + (4 * e + fq) * 8;
        nok[e] = n8 < p.N;
        const uint32_t ncb = nok[e] ? (uint32_t)n8 * 2u : 0u;
        colb[e] = ((uint32_t)(n8 / p.n_split) * (uint32_t)p.c_split_stride + (uint32_t)(n8 % p.n_split)) * 2u;
        bv[e] = has_bias ? *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(p.bias) + ncb) : u32x4{0u, 0u, 0u, 0u};
    }
    // LayerNorm parameters of this lane's columns: e and e + 2 sit at the same place of their heads
    float wv[2][8], bb[2][8];
    const int tn = tsel < 2 ? tsel : 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int hc = (4 * e + fq) * 8;
        unpack8(*reinterpret_cast<const u32x4*>(p.qkn_w[tn] + hc), wv[e]);
        unpack8(*reinterpret_cast<const u32x4*>(p.qkn_b[tn] + hc), bb[e]);
    }
    const float ks = tsel == 1 ? p.qkn_kscale : 1.0f;
    const QknRotary rot = qkn_rotary<true>(p);
    uint32_t n2max[2] = {0u, 0u};                                // STATS: per head, the largest squared row norm so far (bits)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int m = m_wave + 16 * j + fr;
        const bool mok = m < p.M;
        const uint32_t coff = (mok ? (uint32_t)m : 0u) * (uint32_t)(p.ldc * 2);
        const bool rope = tsel < 2 && m >= p.qkn_text_rows && mok;
        // rotary-table row of this token (qkn_rotary_load8: no branch, a row that is not rotated reads zeros)
        QknRotary8 cs[2];
        {
            const uint32_t t0 = rope ? (uint32_t)(m - p.qkn_text_rows) * 256u : 0xffffffffu;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const uint32_t off = rope ? t0 + (uint32_t)((4 * e + fq) * 32) : 0xffffffffu;
                cs[e] = qkn_rotary_load8(rot, off, rope ? off + 16u : off);
            }
        }
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            float v[2][8];
#pragma unroll
            for (int el = 0; el < 2; ++el) {
                const int e = 2 * hh + el;
                float b8[8];
                unpack8(bv[e], b8);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[el][i] = acc[i][j][e] + b8[i];
            }
            if (tsel < 2) {
                // the projection as the two-launch path stored it: one rounding to bf16
#pragma unroll
                for (int el = 0; el < 2; ++el) {
                    const u32x4 r = pack8(v[el]);
                    unpack8(r, v[el]);
                }
                float s0 = lane_add32(lane_add16(qkn_sum8(v[0]))), s1 = lane_add32(lane_add16(qkn_sum8(v[1])));
                const float mean = (s0 + s1) * (1.0f / 64);
                float q0 = lane_add32(lane_add16(qkn_centre_sq8(v[0], mean))), q1 = lane_add32(lane_add16(qkn_centre_sq8(v[1], mean)));
                const float rstd = rsqrtf((q0 + q1) * (1.0f / 64) + p.qkn_eps);
                qkn_finish8(v[0], rstd, wv[0], bb[0], rope, cs[0].c, cs[0].s, ks);
                qkn_finish8(v[1], rstd, wv[1], bb[1], rope, cs[1].c, cs[1].s, ks);
                if constexpr (STATS) {
                    // the row as stored (the same pack8 as the store below), its two groups of this lane, then the tree
                    float r[2][8];
                    unpack8(pack8(v[0]), r[0]);
                    unpack8(pack8(v[1]), r[1]);
                    const float n2 = lane_add32(lane_add16(qkn_norm2_8(r[0]))) + lane_add32(lane_add16(qkn_norm2_8(r[1])));
                    const uint32_t nb = (mok && nok[2 * hh]) ? __float_as_uint(n2) : 0u;
                    n2max[hh] = nb > n2max[hh] ? nb : n2max[hh];
                }
            }
#pragma unroll
            for (int el = 0; el < 2; ++el) {
                const int e = 2 * hh + el;
                __builtin_amdgcn_raw_buffer_store_b128(pack8(v[el]), rsC, (mok && nok[e]) ? coff + colb[e] : 0xffffffffu, 0, 0);
            }
        }
    }
    if constexpr (STATS) {
        if (tsel < 2) {
            // the wave's two heads are neighbours of one tensor (width % 128 == 0): entries i0 and i0 + 1 of
            // [slot][tsel][qkn_stats_nbh], i0 = z * heads + head < qkn_stats_nbh (qkn_stats_args, gemm_common.h)
            unsigned* const tab = reinterpret_cast<unsigned*>(p.qkn_stats) +
                                  ((long long)(blockIdx.x % (unsigned)p.qkn_stats_slots) * 2 + tsel) * p.qkn_stats_nbh;
            const long long i0 = (long long)z * (p.qkn_width / 64) + (n_wave - tsel * p.qkn_width) / 64;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const uint32_t top = qkn_row16_umax(n2max[hh]);          // (the four fq lanes of a row hold the same value)
                if ((fr | fq) == 0) qkn_stats_raise(tab, i0 + hh, top);
            }
        }
    }
}

// The q/k-norm epilogue of one wave (bya_gemm_mx_qkv_norm_rope_on): the packed q|k|v projection with the per-head q/k
// LayerNorm(64) + RoPE of bya_qknorm_rope on its accumulators -- epilogue_qkn (gemm_wide_epilogue.h) on this kernel's
// accumulators, with q, k or v decided per 64-column HEAD (as epilogue_mx_qkn of gemm_mx.hip does), wave-uniformly:
// head hh of the wave is registers e = 2 hh, 2 hh + 1, columns n_wave + 64 hh .. + 63, tsel = (n_wave + 64 hh) / width, so
// width % 64 == 0 is enough and a wave may straddle q | k or k | v.  Bit for bit bya_gemm_mx_mixed(..., n_split) followed by
// bya_qknorm_rope; arithmetic: qknorm_math.h, whose eight groups g of a head row are 8 consecutive columns each.  The lane
// (fr, fq) holds columns n_wave + 64 hh + (4 el + fq) * 8 + i of row 16 j + fr in acc[i][j][2 hh + el]: group g = 4 el + fq.
// What is normalised is bf16(acc + bias), the value the two-launch path stored and read back (one rounding: pack, unpack);
// qkn_sum8 / qkn_centre_sq8 run over the lane's eight values in column order = one whole group; the tree (g ^ 1), (g ^ 2),
// (g ^ 4) is lane ^ 16 (v_permlane16_swap), lane ^ 32 (v_permlane32_swap), then the lane's own two registers (s_e0 + s_e1):
// the same operands per addition as the stand-alone kernel (an addition does not depend on the order of its two operands),
// in the same order.  qkn_finish8 is element-wise and the RoPE pairs (2 i, 2 i + 1) lie inside the lane's eight columns.
// v heads and heads past N take the plain bias epilogue: acc + bias rounded to bf16, epilogue_block's value for alpha = 1
// and no activation.  Rotary rows come through buffer descriptors: rows that are not rotated read zeros from an
// out-of-range offset, no per-row branch.  16-byte stores through the C descriptor with the n_split / c_split_stride column
// map; rows past M and columns past N write nothing.
// Rows outside, heads inside: the rotary row of a token is the same for both heads of the wave, so it is fetched once per
// row block; the two heads' bias and LayerNorm parameters (q's and k's may differ between a wave's two heads) stay PACKED,
// 52 registers, and are unpacked where they are used.  The accumulators of a burst of JB row blocks are pinned in their
// AGPRs until the burst is due (epilogue_wide's PIN) and a scheduling barrier keeps a burst's table loads inside it: 201
// VGPRs + 256 AGPRs, no scratch.  (Heads outside with the pin inside the q/k | v branch made every accumulator a phi of two
// AGPR copies: 205 registers of scratch.)
// SCALED (gemm_fp8_v4.hip's QKN instance, bya_gemm_fp8_qkv_norm_rope): the accumulator is first multiplied by its
// activation-row x weight-channel scale, sa[batch * M] x sw[N], the product of the two scales formed first -- epilogue_wide's
// SCALED expression -- and that product is rounded to fp32 before the bias is added, as the two-launch path's fmaf(1, bias,
// scaled) does: an empty asm that owns the register keeps hipcc's default -ffp-contract from merging the multiply and the
// addition into one fma(acc, scale, bias), which rounds once less.  The eight channel scales of each of the lane's four column
// groups stay in 32 registers for the whole tile.
// STATS: epilogue_qkn's, with the tensor decided per head -- one register per head holds the largest squared norm of the rows
// as stored, one atomic maximum per (wave, q or k head, tile) raises entry z * heads + head of the head's tensor.
template <int JB, bool SCALED = false, bool STATS = false>
__device__ __forceinline__ void epilogue_mx_wide8_qkn(const GemmArgs& p, int z, int m_wave, int n_wave, int fr, int fq,
                                                      f32x4 (&acc)[8][8], const float* __restrict__ sa = nullptr,
                                                      const float* __restrict__ sw = nullptr) {
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.C + (long long)z * p.c_bs), 0, 0x7fffffff, 0x00020000);
    const QknRotary rot = qkn_rotary<false>(p);                    // (the launcher keeps the tables below 2 GiB)
    const bool has_bias = p.bias != nullptr;
    // per head: q / k / v, bias, column map and (q, k) the LayerNorm parameters of this lane's columns, all packed
    int tsel[2];
    u32x4 bv[2][2], wq[2][2], bq[2][2];
    uint32_t colb[2][2];
    bool nok[2][2];
    f32x4 wsc[2][2][2];                                             // SCALED: the eight channel scales of each column group
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        const int n_head = n_wave + 64 * hh;
        tsel[hh] = n_head / p.qkn_width;                            // 0 = q, 1 = k, else v or past N: wave-uniform
#pragma unroll
        for (int el = 0; el < 2; ++el) {
            const int n8 = n_head + (4 * el + fq) * 8;
            nok[hh][el] = n8 < p.N;
            colb[hh][el] = ((uint32_t)(n8 / p.n_split) * (uint32_t)p.c_split_stride + (uint32_t)(n8 % p.n_split)) * 2u;
            bv[hh][el] = has_bias ? *reinterpret_cast<const u32x4*>(p.bias + (nok[hh][el] ? n8 : 0)) : u32x4{0u, 0u, 0u, 0u};
            const bf16_t* const lw = tsel[hh] == 1 ? p.qkn_w[1] : p.qkn_w[0];       // (v heads load q's and do not use them)
            const bf16_t* const lb = tsel[hh] == 1 ? p.qkn_b[1] : p.qkn_b[0];
            wq[hh][el] = *reinterpret_cast<const u32x4*>(lw + (4 * el + fq) * 8);
            bq[hh][el] = *reinterpret_cast<const u32x4*>(lb + (4 * el + fq) * 8);
            if constexpr (SCALED) {
                wsc[hh][el][0] = *reinterpret_cast<const f32x4*>(sw + (nok[hh][el] ? n8 : 0));
                wsc[hh][el][1] = *reinterpret_cast<const f32x4*>(sw + (nok[hh][el] ? n8 : 0) + 4);
            }
        }
    }
    const bool any_qk = tsel[0] < 2;                                // (tsel ascends: a q or k head, if any, is head 0)
    uint32_t n2max[2] = {0u, 0u};                                   // STATS: per head, the largest squared row norm so far (bits)
#pragma unroll
    for (int jb = 0; jb < 8; jb += JB) {
        __builtin_amdgcn_sched_barrier(0);                          // a burst's table loads stay inside the burst
#pragma unroll
        for (int jj = 0; jj < JB; ++jj)
#pragma unroll
            for (int i = 0; i < 8; ++i) asm volatile("" : "+a"(acc[i][jb + jj]));
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            const int j = jb + jj;
            const int m = m_wave + 16 * j + fr;
            const bool mok = m < p.M;
            const uint32_t coff = (mok ? (uint32_t)m : 0u) * (uint32_t)(p.ldc * 2);
            const bool rope = any_qk && mok && m >= p.qkn_text_rows;
            const uint32_t t0 = (uint32_t)(m - p.qkn_text_rows) * 256u;
            float ra = 1.0f;
            if constexpr (SCALED) ra = sa[(long long)z * p.M + (mok ? m : 0)];
            QknRotary8 cs[2];                                       // the rotary row: the same columns of both heads
#pragma unroll
            for (int el = 0; el < 2; ++el) {
                const uint32_t o0 = rope ? t0 + (uint32_t)((4 * el + fq) * 32) : 0xffffffffu;
                const uint32_t o1 = rope ? o0 + 16u : 0xffffffffu;
                cs[el] = qkn_rotary_load8(rot, o0, o1);
            }
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                float v[2][8];
#pragma unroll
                for (int el = 0; el < 2; ++el) {
                    float b8[8];
                    unpack8(bv[hh][el], b8);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if constexpr (SCALED) {
                            float s = acc[i][j][2 * hh + el] * (ra * wsc[hh][el][i >> 2][i & 3]);      // row x channel scale
                            asm("" : "+v"(s));                      // (rounded here: no fma with the bias)
                            v[el][i] = s + b8[i];
                        } else {
                            v[el][i] = acc[i][j][2 * hh + el] + b8[i];
                        }
                    }
                }
                if (tsel[hh] < 2) {
                    const float ks = tsel[hh] == 1 ? p.qkn_kscale : 1.0f;
                    // the projection as the two-launch path stored it: one rounding to bf16
#pragma unroll
                    for (int el = 0; el < 2; ++el) {
                        const u32x4 r = pack8(v[el]);
                        unpack8(r, v[el]);
                    }
                    const float s0 = lane_add32(lane_add16(qkn_sum8(v[0]))), s1 = lane_add32(lane_add16(qkn_sum8(v[1])));
                    const float mean = (s0 + s1) * (1.0f / 64);
                    const float q0 = lane_add32(lane_add16(qkn_centre_sq8(v[0], mean))), q1 = lane_add32(lane_add16(qkn_centre_sq8(v[1], mean)));
                    const float rstd = rsqrtf((q0 + q1) * (1.0f / 64) + p.qkn_eps);
#pragma unroll
                    for (int el = 0; el < 2; ++el) {
                        float w8[8], b8[8];
                        unpack8(wq[hh][el], w8);
                        unpack8(bq[hh][el], b8);
                        qkn_finish8(v[el], rstd, w8, b8, rope, cs[el].c, cs[el].s, ks);
                    }
                    if constexpr (STATS) {
                        float r[2][8];
                        unpack8(pack8(v[0]), r[0]);
                        unpack8(pack8(v[1]), r[1]);
                        const float n2 = lane_add32(lane_add16(qkn_norm2_8(r[0]))) + lane_add32(lane_add16(qkn_norm2_8(r[1])));
                        const uint32_t nb = (mok && nok[hh][0]) ? __float_as_uint(n2) : 0u;
                        n2max[hh] = nb > n2max[hh] ? nb : n2max[hh];
                    }
                }
#pragma unroll
                for (int el = 0; el < 2; ++el)
                    __builtin_amdgcn_raw_buffer_store_b128(pack8(v[el]), rsC, (mok && nok[hh][el]) ? coff + colb[hh][el] : 0xffffffffu, 0, 0);
            }
        }
    }
    if constexpr (STATS) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            if (tsel[hh] < 2) {                                         // (wave-uniform; entry < qkn_stats_nbh: qkn_stats_args)
                unsigned* const tab = reinterpret_cast<unsigned*>(p.qkn_stats) +
                                      ((long long)(blockIdx.x % (unsigned)p.qkn_stats_slots) * 2 + tsel[hh]) * p.qkn_stats_nbh;
                const long long i = (long long)z * (p.qkn_width / 64) + (n_wave + 64 * hh - tsel[hh] * p.qkn_width) / 64;
                const uint32_t top = qkn_row16_umax(n2max[hh]);
                if ((fr | fq) == 0) qkn_stats_raise(tab, i, top);
            }
        }
    }
}

}  // namespace
