// Persistent 256 x 256 x 128 MX GEMM for e4m3 activations x e4m3 weights: gemm256p_fp8_kernel (gemm_fp8_v4.hip) on the
// block-scaled instruction, with real e8m0 block scales -- ONE wave per SIMD, 128 x 128 per wave, 256 accumulator AGPRs, the
// hand-placed two-phase K-tile of that file, its barriers B1 / B2, its four K-tile variants A / B / C / D, the next output
// tile's first two K-tiles requested while this one drains.  Operands, epilogues and RESULT BITS are those of the 128 x 128
// kernel of gemm_mx.hip (gemm_mx_body<MX_E4M3, MX_E4M3>): per 16 x 16 block one v_mfma_scale_f32_16x16x128_f8f6f4 per
// K-tile, K-tiles ascending, W fragment first, the first K-tile on C = 0, on the same operand bytes (a lane's 32 bytes are
// chunks fq and 4 + fq of the K-tile row: the lane order the block-scaled e4m3 instruction wants, gemm_mx.hip) under the
// same scales -- the same instruction sequence per output element, so the two kernels agree bit for bit.
//
// What this file adds to gemm_fp8_v4.hip is the scale side:
//   * LDS: the two 64 KiB code stages stay where they are (the stage flip is address bit 16); behind them, at 128 KiB, two
//     2 KiB scale areas flipped by bit 11: one dword per row and K-tile (the row's 4 block scales), A rows 0..255 at 4 row,
//     W SLOT rows at 1024 + 4 slot.  132 KiB of the CU's 160.
//   * staging: a wave moves the scale dwords of its 64 A rows and of its 64 W slot rows as two 4-byte-per-lane LDS-DMA pieces
//     per K-tile (18 pieces instead of 16), the W ones through the SAME slot -> source-row map as the W codes (w_slot_col),
//     so the fragment of slot row r finds its scales in slot row r.  Buffer descriptors with the tile's extent, as for the
//     codes: a row past M or N lands as zero bytes -- scale 2^-127 on zero codes.
//   * reads: lane (fr, fq) needs byte fq of the dword of row 16 j + fr, for 8 A blocks and 8 W blocks: 16 ds_read_u8 per
//     K-tile (the byte arrives in position 0: no VALU between LDS and the MFMA, so no VALU-write -> MFMA-read hazard to pad
//     inside asm), each issued right behind the fragment read of its block, so it retires with it: W(0..3) at the phase
//     boundary, A(j) behind A(j)'s last MFMA, W(4..7) at the head of the next K-tile.
// Counted waits: B2 counts the pieces of K-tile t + 2 requested so far (tools/gen_gemm_mx_schedule.py), the prologue and
// the tile end wait for all but the 18 youngest, a K-tile ends on lgkmcnt(3) = A(7)'s two fragment reads and its scale.
//
// The quantising epilogue (bya_gemm_mx_quant, out e4m3) needs no staging here: in the wide layout a lane holds EIGHT
// consecutive columns, an MX block of a row is exactly the four lanes fq = 0..3, and the lane's 8 code bytes are contiguous.
// (The ring is not free either: the next tile's first two K-tiles are in it.)
// The q/k-norm epilogue (bya_gemm_mx_qkv_norm_rope_on) needs none either: a head row is the four lanes fq = 0..3 too
// (epilogue_mx_wide8_qkn, gemm_wide_epilogue.h: shared with the persistent fp8 kernel).
//
// FMT_W = MX_E2M1 (e2m1 weights under the same e4m3 activations; bya_gemm_mx_call): the W side alone changes.  A W row of a
// K-tile is 64 bytes -- the 64-byte-row image of gemm_persistent.h at TILE_A of the stage, 16 KiB of its 32 -- so a wave moves
// its 64 W slot rows as FOUR pieces (14 pieces per K-tile: the second generated body below, and vmcnt(14) where the e4m3 form
// waits on 18), a W fragment is ONE ds_read_b128 (wh[] is gone: 32 VGPRs), and the MFMA takes it as a four-register operand
// under cbsz:4 -- the instruction sequence of gemm_mx_body<MX_E4M3, MX_E2M1>, so the bits are that kernel's.  Slot map
// (w_slot_col), scales, A side, tile walk, accumulator layout and the three epilogues are shared with the e4m3 form.
//
// FMT_A = MX_E2M3 (e2m3 activations with e2m3 or e2m1 weights; bya_gemm_mx_call with BYA_MX_KERNEL_FP6): the A side changes,
// and the W side with it for e2m3 weights.  A K-tile row is 96 bytes -- the 96-byte-row image of gemm_persistent.h, 24 KiB of
// the 32 an operand has in a stage -- so a wave moves its 64 slot rows as SIX pieces (14 pieces per K-tile with e2m3 weights,
// 12 with e2m1: the third and fourth generated body; the counted waits come from MX_PIECES_*, which the generator writes from
// its piece tables), a fragment is three ds_read_b64 into SIX registers, and the MFMA takes it under blgp:2 (A) / cbsz:2 (W)
// -- the instruction sequence of gemm_mx_body<MX_E2M3, W>, so the bits are that kernel's.  A K-tile ends on lgkmcnt(4) = A(7)'s
// three fragment reads and its scale.  The e2m3 rate of the instruction is twice e4m3's: LDS fragment reads (96 KiB per CU
// and K-tile at 256 bytes per clock) and the 64 MFMAs of a wave are of the same order, nothing about its time is promised.
// QOUT = MX_E2M3 (any operand pair): the quantising epilogue for e2m3 output (epilogue_mx_wide8_quant6).
// K >= 512.
// Compiled WITHOUT -amdgpu-mfma-vgpr-form, like gemm_fp8_v4.hip.
#include "gemm_wide_epilogue.h"
#include "mx_common.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK8 = 128;                                   // e4m3 elements (= bytes) per K-tile
constexpr int SC_BASE = 2 * 65536, SC_STAGE = 2048, SC_W = 1024;   // the scale areas behind the two code stages
// LDS-DMA pieces of a wave per K-tile of the e2m3-activation bodies (e2m3 / e2m1 weights)
// GENERATED-PIECES-BEGIN (tools/gen_gemm_mx_schedule.py: the lengths of its piece tables)
constexpr int MX_PIECES_A6 = 14, MX_PIECES_A6W4 = 12;
// GENERATED-PIECES-END
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x6 __attribute__((ext_vector_type(6)));
typedef uint32_t u32x3a4 __attribute__((ext_vector_type(3), aligned(4)));       // three dwords at a 4-byte boundary

// one 256-byte LDS-DMA piece of scales: lane l's dword from its global offset to LDS m0 + 4 l
template <int LDS_OFF>
__device__ __forceinline__ void dma_scale_piece(uint32_t lds_base, uint32_t voff, const i32x4& rsrc, uint32_t soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
                 :
                 : "s"(lds_base + LDS_OFF), "v"(voff), "s"(rsrc), "s"(soff)
                 : "memory");
}
template <int OFF>
__device__ __forceinline__ void ds_read64(i32x2& dst, uint32_t addr) {
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
// the six-register e2m3 operand from its three 8-byte reads (no move: the three are allocated side by side)
__device__ __forceinline__ i32x6 cat6(const i32x2& a, const i32x2& b, const i32x2& c) {
    const i32x4 ab = __builtin_shufflevector(a, b, 0, 1, 2, 3), cc = __builtin_shufflevector(c, c, 0, 1, -1, -1);
    return __builtin_shufflevector(ab, cc, 0, 1, 2, 3, 4, 5);
}
template <int OFF>
__device__ __forceinline__ void ds_read_byte(int& dst, uint32_t addr) {
    asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}
// the scale rows of tile c behind its origin: what is left of [batch * M, ks] (A) or [N, ks] (W), nothing for an invalid tile
__device__ __forceinline__ i32x4 tile_rsrc_sa(const GemmArgs& p, const uint8_t* sa, int ks, const PersistentTile& c) {
    const long long left = (long long)(p.M - c.m0) * ks;
    return raw_rsrc(sa + ((long long)c.z * p.M + c.m0) * ks, c.valid && left > 0 ? (uint32_t)left : 0u);
}
__device__ __forceinline__ i32x4 tile_rsrc_sw(const GemmArgs& p, const uint8_t* sw, int ks, const PersistentTile& c) {
    const long long left = (long long)(p.N - c.n0) * ks;
    return raw_rsrc(sw + (long long)c.n0 * ks, c.valid && left > 0 ? (uint32_t)left : 0u);
}

// Quantising epilogue of one wave (bya_gemm_mx_quant, out e4m3): per element  v = bf16( alpha * act(acc + rowscale * bias) ),
// then the block rule of mx_common.h.  MX block e of row 16 j + fr (32 columns from n_wave + 32 e) is the four lanes
// fq = 0..3: |max| over the lane's eight values and its lane ^ 16 / lane ^ 32 partners, mx_quant8_bits on the eight values =
// the lane's 8 code bytes at byte 8 fq of the block, one 8-byte store; the four scale bytes of a row's 128 columns leave as one
// dword from the lane fq = 0.  Rows past M and columns past N (N % 128 == 0: whole 128-column groups) write nothing.  The
// arithmetic per element is epilogue_mx_quant's (gemm_mx.hip), so the bytes are the 128 x 128 kernel's.
template <int ACT>
__device__ __forceinline__ void epilogue_mx_wide8_quant(const GemmArgs& p, uint8_t* __restrict__ qs, int z, int m_wave, int n_wave,
                                                        int fr, int fq, const f32x4 (&acc)[8][8]) {
    const bool has_bias = p.bias != nullptr, has_rs = p.bias_rowscale != nullptr;
    const bool nok = n_wave < p.N;
    uint8_t* const cbase = reinterpret_cast<uint8_t*>(p.C) + (long long)z * p.c_bs;
    u32x4 bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n8 = n_wave + (4 * e + fq) * 8;
        bv[e] = has_bias ? *reinterpret_cast<const u32x4*>(p.bias + (nok ? n8 : 0)) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int m = m_wave + 16 * j + fr;
        const bool ok = m < p.M && nok;
        const float rs = has_rs ? p.bias_rowscale[(long long)z * p.M + (m < p.M ? m : 0)] : 1.0f;
        uint32_t sdword = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float b8[8], t[8], v[8];
            unpack8(bv[e], b8);
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = p.alpha * apply_act<ACT>(fmaf(rs, b8[i], acc[i][j][e]), p.leaky);
            unpack8(pack8(t), v);                                 // the one rounding to bf16
            float amax = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
            amax = lane_max32(lane_max16(amax));
            uint32_t sbyte;
            const uint64_t bits = mx_quant8_bits<MX_E4M3>(v, amax, sbyte);
            sdword |= sbyte << (8 * e);
            if (ok)
                *reinterpret_cast<u32x2*>(cbase + (long long)m * p.ldc + n_wave + 32 * e + 8 * fq) =
                    u32x2{(uint32_t)bits, (uint32_t)(bits >> 32)};
        }
        if (ok && fq == 0)
            *reinterpret_cast<uint32_t*>(qs + ((long long)z * p.M + m) * (p.N / 32) + n_wave / 32) = sdword;
    }
}

// ... for e2m3 output (QOUT = MX_E2M3 of the kernel, any operand pair): the same values, amax and block rule; the lane's eight
// codes are 48 bits at byte 6 fq of the 24-byte block.  The lane ^ 16 pair (fq ^ 1) trades them (v_permlane16_swap of a register
// with itself: both lanes then hold the even lane's and the odd lane's value), and the lanes fq = 0 and fq = 2 store the pair's
// 12 contiguous, 4-byte-aligned bytes, at byte 0 / 12 of the block, as one three-dword vector store: the bytes of
// epilogue_mx_quant<.., MX_E2M3> (gemm_mx.hip).  Scale bytes as above.  The eight row blocks are WRITTEN OUT: their e2m3
// conversions are more than `#pragma unroll` unrolls in one loop, and a loop that stays a loop indexes acc at run time -- the
// whole array then lives in scratch (1040 bytes per lane); each row block's accumulators stay pinned in their AGPRs until it is
// due (as epilogue_wide's PIN): 161-163 VGPRs + 256 AGPRs, no scratch.
template <int ACT>
__device__ __forceinline__ void epilogue_mx_wide8_quant6(const GemmArgs& p, uint8_t* __restrict__ qs, int z, int m_wave, int n_wave,
                                                         int fr, int fq, f32x4 (&acc)[8][8]) {
    const bool has_bias = p.bias != nullptr, has_rs = p.bias_rowscale != nullptr;
    const bool nok = n_wave < p.N;
    uint8_t* const cbase = reinterpret_cast<uint8_t*>(p.C) + (long long)z * p.c_bs;
    u32x4 bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n8 = n_wave + (4 * e + fq) * 8;
        bv[e] = has_bias ? *reinterpret_cast<const u32x4*>(p.bias + (nok ? n8 : 0)) : u32x4{0u, 0u, 0u, 0u};
    }
    auto row_block = [&](const int j) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+a"(acc[i][j]));
        const int m = m_wave + 16 * j + fr;
        const bool ok = m < p.M && nok;
        const float rs = has_rs ? p.bias_rowscale[(long long)z * p.M + (m < p.M ? m : 0)] : 1.0f;
        uint32_t sdword = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float b8[8], t[8], v[8];
            unpack8(bv[e], b8);
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] = p.alpha * apply_act<ACT>(fmaf(rs, b8[i], acc[i][j][e]), p.leaky);
            unpack8(pack8(t), v);                                 // the one rounding to bf16
            float amax = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
            amax = lane_max32(lane_max16(amax));
            uint32_t sbyte;
            const uint64_t bits = mx_quant8_bits<MX_E2M3>(v, amax, sbyte);
            sdword |= sbyte << (8 * e);
            const auto lo = lane_pair16((uint32_t)bits), hi = lane_pair16((uint32_t)(bits >> 32));
            if (ok && !(fq & 1))
                *reinterpret_cast<u32x3a4*>(cbase + (long long)m * p.ldc + (n_wave / 32 + e) * 24 + 6 * fq) =
                    u32x3a4{lo[0], hi[0] | (lo[1] << 16), (lo[1] >> 16) | (hi[1] << 16)};
        }
        if (ok && fq == 0)
            *reinterpret_cast<uint32_t*>(qs + ((long long)z * p.M + m) * (p.N / 32) + n_wave / 32) = sdword;
    };
    row_block(0); row_block(1); row_block(2); row_block(3); row_block(4); row_block(5); row_block(6); row_block(7);
}

// QOUT = MX_EPI_BF16: the bf16 epilogue; MX_EPI_QKN: the q/k-norm one (p.qkn_*), MX_EPI_QKN_STATS: the same with the score-bound
// statistics (p.qkn_stats; the launcher takes it where the arguments carry a table); MX_E4M3 / MX_E2M3: the quantising one for that
// output format (C = codes with ldc / c_bs in bytes, qs = its scale bytes).  FMT_W: the weights' element format, FMT_A or
// MX_E2M1; FMT_A: the activations', MX_E4M3 or MX_E2M3 (the top of the file)
template <int QOUT, int FMT_W, int FMT_A>
__global__ __launch_bounds__(256, 1) void gemm256p_mx_kernel(GemmArgs p, const uint8_t* __restrict__ sa,
                                                            const uint8_t* __restrict__ sw, int tiles_m, int tiles_n, int batch,
                                                            int GM, uint8_t* __restrict__ qs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = 256, BN = 256, STAGE = (BM + BN) * BK8, TILE_A = BM * BK8;
    static_assert(STAGE == 65536 && SC_BASE == 2 * STAGE, "stage flip uses one address bit; the scales sit behind the codes");
    static_assert(FMT_A == MX_E4M3 || FMT_A == MX_E2M3, "activations: e4m3 or e2m3");
    static_assert(FMT_W == FMT_A || FMT_W == MX_E2M1, "weights: the activations' format or e2m1");
    constexpr bool W4 = FMT_W == MX_E2M1, A6 = FMT_A == MX_E2M3, W6 = FMT_W == MX_E2M3;
    constexpr int BKA = A6 ? 96 : BK8;                         // bytes of an A row per K-tile
    constexpr int BKW = W4 ? 64 : W6 ? 96 : BK8;               // ... of a W row
    constexpr int NPA = A6 ? 6 : 8;                            // A code pieces of a wave per K-tile
    constexpr int NPW = W4 ? 4 : W6 ? 6 : 8;                   // W code pieces
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = p.K / BK8, ks = p.K / 32;
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fq = lane >> 4;

    const TileWalk<BM, BN> walk(tiles_m, tiles_n, batch, GM);
    int seq = 0;
    PersistentTile cur = walk.coord(seq);
    if (!cur.valid) return;

    // fragment read addresses (the LDS image: gemm_persistent.h; c*: the stage of the current K-tile).  The lane's scale byte
    // is byte fq of the dword of row a_row (A) / slot row w_row (W), blocks 16 rows = 64 bytes apart (cSa / cSw, below)
    const int a_row = wm * 128 + fr, w_row = wn * 128 + fr;
    const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
    // (e2m3: the one address of the lane's 24 bytes in c?l; c?h unused, as cWh is for e2m1)
    uint32_t cAl = A6 ? frag_addr96(lds0, a_row, fq) : frag_addr(lds0, a_row, fq), cAh = frag_addr(lds0, a_row, 4 + fq);
    uint32_t cWl = W4 ? frag_addr64(lds0 + TILE_A, w_row, fq) : W6 ? frag_addr96(lds0 + TILE_A, w_row, fq) : frag_addr(lds0 + TILE_A, w_row, fq);
    uint32_t cWh = frag_addr(lds0 + TILE_A, w_row, 4 + fq);
    uint32_t fill = __builtin_amdgcn_readfirstlane(lds0 + wave * 64 * BKA);     // this wave's first A piece, current stage
    uint32_t sfill = __builtin_amdgcn_readfirstlane(lds0 + SC_BASE + wave * 256);   // ... its A scale piece
    // the lane's scale byte: byte fq of the dword of row a_row (A) / slot row w_row (W), blocks 16 rows = 64 bytes apart
    uint32_t cSa = lds0 + SC_BASE + 4 * a_row + fq, cSw = lds0 + SC_BASE + SC_W + 4 * w_row + fq;

    // staging (map and source-side swizzle: gemm_persistent.h): wave w moves LDS slot rows [64w, 64w + 64) of the A tile and
    // of the W tile, 8 one-KiB pieces each (e2m3: 6, the wave's 6 KiB cut linearly; e2m1 W: 4, sixteen 64-byte rows each; a
    // narrower W share starts less than an A share per wave apart: w_back),
    // and their scale dwords, lane l = slot row 64w + l
    uint32_t voA[8], voW[8];                                   // (e2m1: voW[0..3]; e2m3: [0..5])
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int rl = wave * 64 + q * 8 + (lane >> 3);
        if constexpr (!A6) voA[q] = stage_off(lane, rl, rl, (uint32_t)p.lda);
        if constexpr (!W4 && !W6) voW[q] = stage_off(lane, rl, w_slot_col(rl), (uint32_t)p.ldw);
    }
    if constexpr (A6) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int rl = wave * 64 + stage_row96(lane, q);
            voA[q] = stage_off96(lane, q, rl, rl, (uint32_t)p.lda);
            if constexpr (W6) voW[q] = stage_off96(lane, q, rl, w_slot_col(rl), (uint32_t)p.ldw);
        }
    }
    if constexpr (W4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rl = wave * 64 + q * 16 + (lane >> 2);
            voW[q] = stage_off64(lane, rl, w_slot_col(rl), (uint32_t)p.ldw);
        }
    }
    // `fill` steps 64 A rows per wave (8 KiB, e2m3: 6 KiB), a narrower W image less (e2m1: 4 KiB)
    const uint32_t w_back = (uint32_t)wave * (uint32_t)(64 * (BKA - BKW));
    const uint32_t voSa = (uint32_t)(wave * 64 + lane) * (uint32_t)ks;
    const uint32_t voSw = (uint32_t)w_slot_col(wave * 64 + lane) * (uint32_t)ks;
    const uint8_t* const A8 = reinterpret_cast<const uint8_t*>(p.A);
    const uint8_t* const W8 = reinterpret_cast<const uint8_t*>(p.W);
    const int kw_bytes = W4 ? p.K / 2 : W6 ? p.K / 4 * 3 : p.K;     // bytes of a W row that the GEMM reads
    const int ka_bytes = A6 ? p.K / 4 * 3 : 0;                      // ... of an A row (0: K)
    i32x4 rsA = tile_rsrc_a(p, A8, cur, ka_bytes), rsW = tile_rsrc_w(p, W8, cur, kw_bytes);
    i32x4 rsSa = tile_rsrc_sa(p, sa, ks, cur), rsSw = tile_rsrc_sw(p, sw, ks, cur);

#define DMA_A(Q, BASE, VO, RS, SOFF) DMA_PIECE(Q, BASE, VO, RS, SOFF)
#define DMA_W(Q, BASE, VO, RS, SOFF) DMA_PIECE(Q, (BASE) + TILE_A - w_back, VO, RS, SOFF)
#define ALLW(M, ...) do { if constexpr (W4) { ALL4(M, __VA_ARGS__); } else if constexpr (W6) { ALL6(M, __VA_ARGS__); } else { ALL8(M, __VA_ARGS__); } } while (0)
#define ALLA(M, ...) do { if constexpr (A6) { ALL6(M, __VA_ARGS__); } else { ALL8(M, __VA_ARGS__); } } while (0)
#define DMA_SA(BASE, RS, SOFF) dma_scale_piece<0>(BASE, voSa, RS, SOFF)
#define DMA_SW(BASE, RS, SOFF) dma_scale_piece<SC_W>(BASE, voSw, RS, SOFF)
    // ---- prologue of the FIRST tile only: K-tiles 0 and 1
    ALLA(DMA_A, fill, voA, rsA, 0u);
    ALLW(DMA_W, fill, voW, rsW, 0u);
    DMA_SA(sfill, rsSa, 0u);
    DMA_SW(sfill, rsSw, 0u);
    ALLA(DMA_A, fill ^ STAGE, voA, rsA, (uint32_t)BKA);
    ALLW(DMA_W, fill ^ STAGE, voW, rsW, (uint32_t)BKW);
    DMA_SA(sfill ^ SC_STAGE, rsSa, 4u);
    DMA_SW(sfill ^ SC_STAGE, rsSw, 4u);
    // K-tile 0 has landed once all but the pieces of K-tile 1 have: NPA + NPW + 2 of them
#define WAIT_KTILE(TAIL) do {                                                                                            \
        if constexpr (A6) asm volatile("s_waitcnt vmcnt(%0)" TAIL :: "n"(W4 ? MX_PIECES_A6W4 : MX_PIECES_A6) : "memory");       \
        else if constexpr (W4) asm volatile("s_waitcnt vmcnt(14)" TAIL ::: "memory");                                      \
        else asm volatile("s_waitcnt vmcnt(18)" TAIL ::: "memory");                                                        \
    } while (0)
    static_assert(NPA + NPW + 2 == (A6 ? (W4 ? MX_PIECES_A6W4 : MX_PIECES_A6) : W4 ? 14 : 18), "the counted waits follow the pieces of a K-tile");
    WAIT_KTILE("");

    f32x4 acc[8][8];
    // low / high 16 bytes of the A (row block j) and W (column block i) fragments; an e2m1 W fragment is wl alone
    i32x4 al[8], ah[8], wl[8], wh[8];
    i32x2 a6[3][8], w6[3][8];                    // e2m3: the three 8-byte reads of a fragment (al / ah, wl / wh unused)
    int xa[8], xw[8];                            // their scale bytes for this lane's K-block fq, in byte 0

    for (;;) {
        // ---- K-tile 0 of this output tile has landed for this wave (prologue wait / the wait in front of the previous
        // epilogue); make that true for everybody, then fetch its A fragments and W(0..3), each with its scale
        asm volatile("s_barrier" ::: "memory");
#define RAF(J, LO, HI, SC) do {                                                                                          \
            if constexpr (A6) { ds_read64<(J) * 1536>(a6[0][J], LO); ds_read64<(J) * 1536 + 8>(a6[1][J], LO); ds_read64<(J) * 1536 + 16>(a6[2][J], LO); } \
            else { ds_read128<(J) * 2048>(al[J], LO); ds_read128<(J) * 2048>(ah[J], HI); }                                 \
            ds_read_byte<(J) * 64>(xa[J], SC);                                                                             \
        } while (0)
#define RWF(I, LO, HI, SC) do {                                                                                          \
            if constexpr (W4) { ds_read128<(I) * 1024>(wl[I], LO); }                                                       \
            else if constexpr (W6) { ds_read64<(I) * 1536>(w6[0][I], LO); ds_read64<(I) * 1536 + 8>(w6[1][I], LO); ds_read64<(I) * 1536 + 16>(w6[2][I], LO); } \
            else { ds_read128<(I) * 2048>(wl[I], LO); ds_read128<(I) * 2048>(wh[I], HI); }                                 \
            ds_read_byte<(I) * 64>(xw[I], SC);                                                                             \
        } while (0)
        RAF(0, cAl, cAh, cSa); RAF(1, cAl, cAh, cSa); RAF(2, cAl, cAh, cSa); RAF(3, cAl, cAh, cSa);
        RAF(4, cAl, cAh, cSa); RAF(5, cAl, cAh, cSa); RAF(6, cAl, cAh, cSa); RAF(7, cAl, cAh, cSa);
        RWF(0, cWl, cWh, cSw); RWF(1, cWl, cWh, cSw); RWF(2, cWl, cWh, cSw); RWF(3, cWl, cWh, cSw);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

        const PersistentTile nxt = walk.coord(seq + 1);
        const i32x4 rsAn = tile_rsrc_a(p, A8, nxt, ka_bytes), rsWn = tile_rsrc_w(p, W8, nxt, kw_bytes);
        const i32x4 rsSan = tile_rsrc_sa(p, sa, ks, nxt), rsSwn = tile_rsrc_sw(p, sw, ks, nxt);

        // One K-tile, variant V (gemm_fp8_v4.hip); t = its index inside the output tile.
        auto ktile = [&](int t, auto v_c) {
            constexpr char V = decltype(v_c)::value;
            const uint32_t soff = (uint32_t)((t + 2) * BKA), ssoff = (uint32_t)((t + 2) * 4);
            const uint32_t wsoff = (uint32_t)((t + 2) * BKW);
            const uint32_t nAl = cAl ^ STAGE, nAh = cAh ^ STAGE, nWl = cWl ^ STAGE, nWh = cWh ^ STAGE;
            const uint32_t nSa = cSa ^ SC_STAGE, nSw = cSw ^ SC_STAGE;
#define OPW(I) __builtin_shufflevector(wl[I], wh[I], 0, 1, 2, 3, 4, 5, 6, 7)
#define OPA(J) __builtin_shufflevector(al[J], ah[J], 0, 1, 2, 3, 4, 5, 6, 7)
            // e2m1 W: the four registers of the lane's block under cbsz:4 (activations: blgp:0, the default)
#define OPW6(I) cat6(w6[0][I], w6[1][I], w6[2][I])
#define OPA6(J) cat6(a6[0][J], a6[1][J], a6[2][J])
            // e2m3 activations: the six registers of the lane's block under blgp:2; e2m3 W the same under cbsz:2
#define MFX6(I, J) do {                                                                                                  \
                if constexpr (W4 && V == 'A')                                                                              \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, 0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:2" \
                                 : "=a"(acc[I][J]) : "v"(wl[I]), "v"(OPA6(J)), "v"(xw[I]), "v"(xa[J]));                    \
                else if constexpr (W4)                                                                                     \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4 blgp:2" \
                                 : "+a"(acc[I][J]) : "v"(wl[I]), "v"(OPA6(J)), "v"(xw[I]), "v"(xa[J]));                    \
                else if constexpr (V == 'A')                                                                               \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, 0, %3, %4 op_sel_hi:[0,0,0] cbsz:2 blgp:2" \
                                 : "=a"(acc[I][J]) : "v"(OPW6(I)), "v"(OPA6(J)), "v"(xw[I]), "v"(xa[J]));                  \
                else                                                                                                       \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:2 blgp:2" \
                                 : "+a"(acc[I][J]) : "v"(OPW6(I)), "v"(OPA6(J)), "v"(xw[I]), "v"(xa[J]));                  \
            } while (0)
#define MFX(I, J) do {                                                                                                   \
                if constexpr (A6) MFX6(I, J);                                                                              \
                else if constexpr (W4 && V == 'A')                                                                              \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, 0, %3, %4 op_sel_hi:[0,0,0] cbsz:4"        \
                                 : "=a"(acc[I][J]) : "v"(wl[I]), "v"(OPA(J)), "v"(xw[I]), "v"(xa[J]));                     \
                else if constexpr (W4)                                                                                     \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4"       \
                                 : "+a"(acc[I][J]) : "v"(wl[I]), "v"(OPA(J)), "v"(xw[I]), "v"(xa[J]));                     \
                else if constexpr (V == 'A')                                                                                    \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, 0, %3, %4 op_sel_hi:[0,0,0]"               \
                                 : "=a"(acc[I][J]) : "v"(OPW(I)), "v"(OPA(J)), "v"(xw[I]), "v"(xa[J]));                    \
                else                                                                                                       \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"              \
                                 : "+a"(acc[I][J]) : "v"(OPW(I)), "v"(OPA(J)), "v"(xw[I]), "v"(xa[J]));                    \
            } while (0)
            // one LDS-DMA piece: K-tile t + 2 of this tile, or the next tile's first two
#define PIECE(Q, IS_W) do {                                                                                              \
                if constexpr (V == 'C') { if (IS_W) DMA_W(Q, fill, voW, rsWn, 0u); else DMA_A(Q, fill, voA, rsAn, 0u); }  \
                else if constexpr (V == 'D') { if (IS_W) DMA_W(Q, fill, voW, rsWn, (uint32_t)BKW); else DMA_A(Q, fill, voA, rsAn, (uint32_t)BKA); } \
                else { if (IS_W) DMA_W(Q, fill, voW, rsW, wsoff); else DMA_A(Q, fill, voA, rsA, soff); }                  \
            } while (0)
#define SPIECE(IS_W) do {                                                                                                \
                if constexpr (V == 'C') { if (IS_W) DMA_SW(sfill, rsSwn, 0u); else DMA_SA(sfill, rsSan, 0u); }            \
                else if constexpr (V == 'D') { if (IS_W) DMA_SW(sfill, rsSwn, 4u); else DMA_SA(sfill, rsSan, 4u); }       \
                else { if (IS_W) DMA_SW(sfill, rsSw, ssoff); else DMA_SA(sfill, rsSa, ssoff); }                           \
            } while (0)
            // B1: this K-tile's stage is free (W(4..7) and their scales, the last reads of it, have returned for every wave)
#define B1() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
            // B2: K-tile t + 1 has landed for everybody (N = the pieces of K-tile t + 2 requested so far in this K-tile)
#define B2(N) do { if constexpr (V != 'D') asm volatile("s_waitcnt vmcnt(" #N ")\n\ts_barrier" ::: "memory"); } while (0)
#define REREAD_W() do { if constexpr (V != 'D') { RWF(0, nWl, nWh, nSw); RWF(1, nWl, nWh, nSw); RWF(2, nWl, nWh, nSw); RWF(3, nWl, nWh, nSw); } } while (0)
#define REREAD_A(J) do { if constexpr (V != 'D') RAF(J, nAl, nAh, nSa); } while (0)
            if constexpr (A6 && !W4) {
            // GENERATED-A6-BEGIN (tools/gen_gemm_mx_schedule.py: 6 A, 6 W and 2 scale pieces)
            RWF(4, cWl, cWh, cSw);
            MFX(0, 0); RWF(5, cWl, cWh, cSw);
            MFX(1, 0); RWF(6, cWl, cWh, cSw);
            MFX(2, 0); RWF(7, cWl, cWh, cSw);
            MFX(3, 0);
            MFX(0, 1);
            MFX(1, 1);
            MFX(2, 1);
            MFX(3, 1);
            MFX(0, 2);
            MFX(1, 2); B1();
            MFX(2, 2); PIECE(0, false);
            MFX(3, 2);
            MFX(0, 3);
            MFX(1, 3);
            MFX(2, 3); PIECE(1, false);
            MFX(3, 3);
            MFX(0, 4);
            MFX(1, 4);
            MFX(2, 4); PIECE(2, false);
            MFX(3, 4);
            MFX(0, 5);
            MFX(1, 5);
            MFX(2, 5); PIECE(3, false);
            MFX(3, 5);
            MFX(0, 6);
            MFX(1, 6);
            MFX(2, 6); PIECE(4, false);
            MFX(3, 6);
            MFX(0, 7);
            MFX(1, 7);
            MFX(2, 7); PIECE(5, false); B2(6);
            MFX(3, 7); REREAD_W();
            MFX(4, 0); PIECE(0, true);
            MFX(5, 0);
            MFX(6, 0);
            MFX(7, 0); REREAD_A(0);
            MFX(4, 1); PIECE(1, true);
            MFX(5, 1);
            MFX(6, 1);
            MFX(7, 1); REREAD_A(1);
            MFX(4, 2); PIECE(2, true);
            MFX(5, 2);
            MFX(6, 2);
            MFX(7, 2); REREAD_A(2);
            MFX(4, 3); PIECE(3, true);
            MFX(5, 3);
            MFX(6, 3);
            MFX(7, 3); REREAD_A(3);
            MFX(4, 4); PIECE(4, true);
            MFX(5, 4);
            MFX(6, 4);
            MFX(7, 4); REREAD_A(4);
            MFX(4, 5); PIECE(5, true);
            MFX(5, 5);
            MFX(6, 5);
            MFX(7, 5); REREAD_A(5);
            MFX(4, 6);
            MFX(5, 6);
            MFX(6, 6);
            MFX(7, 6); SPIECE(false); REREAD_A(6);
            MFX(4, 7);
            MFX(5, 7);
            MFX(6, 7); SPIECE(true);
            MFX(7, 7); REREAD_A(7);
            // GENERATED-A6-END
            } else if constexpr (A6) {
            // GENERATED-A6W4-BEGIN (tools/gen_gemm_mx_schedule.py: 6 A, 4 W and 2 scale pieces)
            RWF(4, cWl, cWh, cSw);
            MFX(0, 0); RWF(5, cWl, cWh, cSw);
            MFX(1, 0); RWF(6, cWl, cWh, cSw);
            MFX(2, 0); RWF(7, cWl, cWh, cSw);
            MFX(3, 0);
            MFX(0, 1);
            MFX(1, 1);
            MFX(2, 1);
            MFX(3, 1);
            MFX(0, 2);
            MFX(1, 2); B1();
            MFX(2, 2); PIECE(0, false);
            MFX(3, 2);
            MFX(0, 3);
            MFX(1, 3);
            MFX(2, 3); PIECE(1, false);
            MFX(3, 3);
            MFX(0, 4);
            MFX(1, 4);
            MFX(2, 4); PIECE(2, false);
            MFX(3, 4);
            MFX(0, 5);
            MFX(1, 5);
            MFX(2, 5); PIECE(3, false);
            MFX(3, 5);
            MFX(0, 6);
            MFX(1, 6);
            MFX(2, 6); PIECE(4, false);
            MFX(3, 6);
            MFX(0, 7);
            MFX(1, 7);
            MFX(2, 7); PIECE(5, false); B2(6);
            MFX(3, 7); REREAD_W();
            MFX(4, 0); PIECE(0, true);
            MFX(5, 0);
            MFX(6, 0);
            MFX(7, 0); REREAD_A(0);
            MFX(4, 1);
            MFX(5, 1);
            MFX(6, 1); PIECE(1, true);
            MFX(7, 1); REREAD_A(1);
            MFX(4, 2);
            MFX(5, 2);
            MFX(6, 2);
            MFX(7, 2); REREAD_A(2);
            MFX(4, 3); PIECE(2, true);
            MFX(5, 3);
            MFX(6, 3);
            MFX(7, 3); REREAD_A(3);
            MFX(4, 4);
            MFX(5, 4);
            MFX(6, 4); PIECE(3, true);
            MFX(7, 4); REREAD_A(4);
            MFX(4, 5);
            MFX(5, 5);
            MFX(6, 5);
            MFX(7, 5); REREAD_A(5);
            MFX(4, 6);
            MFX(5, 6);
            MFX(6, 6);
            MFX(7, 6); SPIECE(false); REREAD_A(6);
            MFX(4, 7);
            MFX(5, 7);
            MFX(6, 7); SPIECE(true);
            MFX(7, 7); REREAD_A(7);
            // GENERATED-A6W4-END
            } else if constexpr (!W4) {
            // GENERATED-BEGIN (tools/gen_gemm_mx_schedule.py)
            RWF(4, cWl, cWh, cSw);
            MFX(0, 0); RWF(5, cWl, cWh, cSw);
            MFX(1, 0); RWF(6, cWl, cWh, cSw);
            MFX(2, 0); RWF(7, cWl, cWh, cSw);
            MFX(3, 0);
            MFX(0, 1);
            MFX(1, 1);
            MFX(2, 1);
            MFX(3, 1);
            MFX(0, 2);
            MFX(1, 2); B1();
            MFX(2, 2); PIECE(0, false);
            MFX(3, 2);
            MFX(0, 3);
            MFX(1, 3); PIECE(1, false);
            MFX(2, 3);
            MFX(3, 3);
            MFX(0, 4); PIECE(2, false);
            MFX(1, 4);
            MFX(2, 4);
            MFX(3, 4); PIECE(3, false);
            MFX(0, 5);
            MFX(1, 5);
            MFX(2, 5); PIECE(4, false);
            MFX(3, 5);
            MFX(0, 6);
            MFX(1, 6); PIECE(5, false);
            MFX(2, 6);
            MFX(3, 6);
            MFX(0, 7); PIECE(6, false);
            MFX(1, 7);
            MFX(2, 7); B2(7);
            MFX(3, 7); REREAD_W();
            MFX(4, 0); PIECE(7, false);
            MFX(5, 0);
            MFX(6, 0);
            MFX(7, 0); PIECE(0, true); REREAD_A(0);
            MFX(4, 1);
            MFX(5, 1);
            MFX(6, 1); PIECE(1, true);
            MFX(7, 1); REREAD_A(1);
            MFX(4, 2);
            MFX(5, 2); PIECE(2, true);
            MFX(6, 2);
            MFX(7, 2); REREAD_A(2);
            MFX(4, 3); PIECE(3, true);
            MFX(5, 3);
            MFX(6, 3);
            MFX(7, 3); PIECE(4, true); REREAD_A(3);
            MFX(4, 4);
            MFX(5, 4);
            MFX(6, 4); PIECE(5, true);
            MFX(7, 4); REREAD_A(4);
            MFX(4, 5);
            MFX(5, 5); PIECE(6, true);
            MFX(6, 5);
            MFX(7, 5); REREAD_A(5);
            MFX(4, 6); PIECE(7, true);
            MFX(5, 6);
            MFX(6, 6);
            MFX(7, 6); SPIECE(false); REREAD_A(6);
            MFX(4, 7);
            MFX(5, 7);
            MFX(6, 7); SPIECE(true);
            MFX(7, 7); REREAD_A(7);
            // GENERATED-END
            } else {
            // GENERATED-W4-BEGIN (tools/gen_gemm_mx_schedule.py: 8 A, 4 W and 2 scale pieces)
            RWF(4, cWl, cWh, cSw);
            MFX(0, 0); RWF(5, cWl, cWh, cSw);
            MFX(1, 0); RWF(6, cWl, cWh, cSw);
            MFX(2, 0); RWF(7, cWl, cWh, cSw);
            MFX(3, 0);
            MFX(0, 1);
            MFX(1, 1);
            MFX(2, 1);
            MFX(3, 1);
            MFX(0, 2);
            MFX(1, 2); B1();
            MFX(2, 2); PIECE(0, false);
            MFX(3, 2);
            MFX(0, 3);
            MFX(1, 3); PIECE(1, false);
            MFX(2, 3);
            MFX(3, 3);
            MFX(0, 4); PIECE(2, false);
            MFX(1, 4);
            MFX(2, 4);
            MFX(3, 4); PIECE(3, false);
            MFX(0, 5);
            MFX(1, 5);
            MFX(2, 5); PIECE(4, false);
            MFX(3, 5);
            MFX(0, 6);
            MFX(1, 6); PIECE(5, false);
            MFX(2, 6);
            MFX(3, 6);
            MFX(0, 7); PIECE(6, false);
            MFX(1, 7);
            MFX(2, 7); B2(7);
            MFX(3, 7); REREAD_W();
            MFX(4, 0); PIECE(7, false);
            MFX(5, 0);
            MFX(6, 0);
            MFX(7, 0); PIECE(0, true); REREAD_A(0);
            MFX(4, 1);
            MFX(5, 1);
            MFX(6, 1);
            MFX(7, 1); REREAD_A(1);
            MFX(4, 2);
            MFX(5, 2); PIECE(1, true);
            MFX(6, 2);
            MFX(7, 2); REREAD_A(2);
            MFX(4, 3);
            MFX(5, 3);
            MFX(6, 3);
            MFX(7, 3); PIECE(2, true); REREAD_A(3);
            MFX(4, 4);
            MFX(5, 4);
            MFX(6, 4);
            MFX(7, 4); REREAD_A(4);
            MFX(4, 5);
            MFX(5, 5); PIECE(3, true);
            MFX(6, 5);
            MFX(7, 5); REREAD_A(5);
            MFX(4, 6);
            MFX(5, 6);
            MFX(6, 6);
            MFX(7, 6); SPIECE(false); REREAD_A(6);
            MFX(4, 7);
            MFX(5, 7);
            MFX(6, 7); SPIECE(true);
            MFX(7, 7); REREAD_A(7);
            // GENERATED-W4-END
            }
#undef B1
#undef B2
#undef REREAD_W
#undef REREAD_A
            // the next K-tile starts with A(0) and W(0..3): everything but A(7)'s three reads (e2m3: four; LDS returns in order;
            // they are covered by that K-tile's wait in front of B1)
            if constexpr (V != 'D' && A6) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
            else if constexpr (V != 'D') asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory");
            cAl ^= STAGE; cAh ^= STAGE; cWl ^= STAGE; cWh ^= STAGE; fill ^= STAGE;
            cSa ^= SC_STAGE; cSw ^= SC_STAGE; sfill ^= SC_STAGE;
            if constexpr (A6) {
                KEEP8(a6[0]); KEEP8(a6[1]); KEEP8(a6[2]); KEEP8(xa); KEEP8(xw);
                if constexpr (W4) { KEEP8(wl); } else { KEEP8(w6[0]); KEEP8(w6[1]); KEEP8(w6[2]); }
            } else {
                KEEP8(al); KEEP8(ah); KEEP8(wl); KEEP8(xa); KEEP8(xw);
                if constexpr (!W4) KEEP8(wh);
            }
#undef SPIECE
#undef PIECE
#undef MFX
#undef MFX6
#undef OPA6
#undef OPW6
#undef OPA
#undef OPW
        };
        ktile(0, IntTag<'A'>{});
        for (int t = 1; t + 2 < nk; ++t) ktile(t, IntTag<'B'>{});
        ktile(nk - 2, IntTag<'C'>{});
        ktile(nk - 1, IntTag<'D'>{});
#undef RAF
#undef RWF
        // K-tile 0 of the next output tile (18 pieces, e2m1 W: 14, e2m3 A: 14 / 12, requested during variant C) has landed once all but the as
        // many younger pieces of its K-tile 1 have; the MFMAs are inline asm, so pad their last results before the epilogue
        // reads them
        WAIT_KTILE("\n\ts_nop 15\n\ts_nop 15");
#undef WAIT_KTILE

        if constexpr (QOUT == MX_EPI_QKN) {
            epilogue_mx_wide8_qkn<2>(p, cur.z, cur.m0 + wm * 128, cur.n0 + wn * 128, fr, fq, acc);
        } else if constexpr (QOUT == MX_EPI_QKN_STATS) {
            epilogue_mx_wide8_qkn<2, false, true>(p, cur.z, cur.m0 + wm * 128, cur.n0 + wn * 128, fr, fq, acc);
        } else {
            auto run = [&](auto act_tag) {
                if constexpr (QOUT == MX_EPI_BF16)       // (wave, lane: the split writer's, unused here; PIN: acc stays in AGPRs per burst)
                    epilogue_wide<decltype(act_tag)::value, 2, false, false, 8, true>(p, cur.z, cur.m0 + wm * 128, cur.n0 + wn * 128, fr, fq, acc, 0, 0);
                else if constexpr (QOUT == MX_E2M3)
                    epilogue_mx_wide8_quant6<decltype(act_tag)::value>(p, qs, cur.z, cur.m0 + wm * 128, cur.n0 + wn * 128, fr, fq, acc);
                else
                    epilogue_mx_wide8_quant<decltype(act_tag)::value>(p, qs, cur.z, cur.m0 + wm * 128, cur.n0 + wn * 128, fr, fq, acc);
            };
            dispatch_act_big(p.act, run);
        }

        if (!nxt.valid) break;
        ++seq;
        cur = nxt;
        rsA = rsAn;
        rsW = rsWn;
        rsSa = rsSan;
        rsSw = rsSwn;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the (empty-descriptor) prefetch pieces of the tile after the last
}

}  // namespace

// Is the persistent MX kernel applicable?  The rules of bya_gemm256p_fp8_eligible (16-byte epilogue accesses aligned, at least
// four K-tiles, 16-byte operand rows); quant: C = the codes, ldc / c_bs in bytes (bya_gemm_mx_quant has checked their
// 16-byte alignment and N % 128 == 0).  lda / ldw are BYTES of a code row, so the rules hold for e2m1 weights (ldw >= K / 2) as
// they stand
bool bya_gemm256p_mx_eligible(const void* args, bool quant) {
    const GemmArgs& a = *static_cast<const GemmArgs*>(args);
    if (!(a.K % BK8 == 0 && a.K >= 4 * BK8 && a.N % 8 == 0 && a.lda % 16 == 0 && a.ldw % 16 == 0 &&
          (long long)a.M * a.lda < (1LL << 32) && (long long)a.N * a.ldw < (1LL << 32)))
        return false;
    if (quant) return a.N % 128 == 0 && a.ldc % 16 == 0 && a.c_bs % 16 == 0 && !(((uintptr_t)a.C | (uintptr_t)a.bias) & 15);
    return a.n_split % 8 == 0 && a.ldc % 8 == 0 && (!a.res || a.ldres % 8 == 0) &&
        !(((uintptr_t)a.C | (uintptr_t)a.res | (uintptr_t)a.bias | (uintptr_t)a.gate0 | (uintptr_t)a.gate1) & 15) &&
        a.c_bs % 8 == 0 && a.res_bs % 8 == 0 && a.gate_bs % 8 == 0 && a.c_split_stride % 8 == 0;
}

// sa / sw: the e8m0 scale bytes [batch * M, K / 32] / [N, K / 32].  epi: MX_EPI_BF16, MX_EPI_QKN = the q/k-norm epilogue
// (GemmArgs::qkn_*; the caller has checked mx_qkn_args' conditions), MX_E4M3 = the quantising one (qs: its scale bytes);
// or MX_E2M3 = quantising to e2m3; a_fmt: MX_E4M3 or MX_E2M3, the activations' format; w_fmt: a_fmt or MX_E2M1, the weights'
int bya_launch_gemm256p_mx(const void* args, const uint8_t* sa, const uint8_t* sw, uint8_t* qs, int epi, int a_fmt, int w_fmt,
                           int batch, int gm, hipStream_t s) {
    const GemmArgs& a = *static_cast<const GemmArgs*>(args);
    const int tiles_m = (a.M + 255) / 256, tiles_n = (a.N + 255) / 256;
    const size_t lds = SC_BASE + 2 * SC_STAGE;
    const int grid = persistent_grid((long long)tiles_m * tiles_n * batch);
    if ((a_fmt != MX_E4M3 && a_fmt != MX_E2M3) || (w_fmt != a_fmt && w_fmt != MX_E2M1)) return BYA_ERR_UNSUPPORTED;
    if (epi != MX_EPI_BF16 && epi != MX_EPI_QKN && epi != MX_E4M3 && epi != MX_E2M3) return BYA_ERR_UNSUPPORTED;
    auto go = [&](auto epi_tag) {
        constexpr int EPI = decltype(epi_tag)::value;
        auto on = [&](auto w_tag, auto a_tag) {
            return launch_persistent<gemm256p_mx_kernel<EPI, decltype(w_tag)::value, decltype(a_tag)::value>>(
                grid, 256, lds, s, a, sa, sw, tiles_m, tiles_n, batch, gm < 1 ? 1 : gm, qs);
        };
        if (a_fmt == MX_E2M3) return w_fmt == MX_E2M1 ? on(IntTag<MX_E2M1>{}, IntTag<MX_E2M3>{}) : on(IntTag<MX_E2M3>{}, IntTag<MX_E2M3>{});
        return w_fmt == MX_E2M1 ? on(IntTag<MX_E2M1>{}, IntTag<MX_E4M3>{}) : on(IntTag<MX_E4M3>{}, IntTag<MX_E4M3>{});
    };
    if (epi == MX_EPI_QKN && a.qkn_stats) return go(IntTag<MX_EPI_QKN_STATS>{});
    return epi == MX_EPI_QKN ? go(IntTag<MX_EPI_QKN>{}) : epi == MX_E4M3 ? go(IntTag<MX_E4M3>{}) :
           epi == MX_E2M3 ? go(IntTag<MX_E2M3>{}) : go(IntTag<MX_EPI_BF16>{});
}
