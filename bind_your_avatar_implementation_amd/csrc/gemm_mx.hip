// MX (OCP Microscaling) "NT" GEMM on the block-scaled CDNA4 matrix instruction, and the block quantiser that feeds it:
//     C[m,n] = epi( sum_k A[m,k] * W[n,k] ),   A, W = e8m0 scale per 32 consecutive k  x  e4m3 / e2m3 elements,
//     or W alone in e2m1 under e4m3 / e2m3 activations (bya_gemm_mx_mixed: the instruction takes a format per operand)
// Format and storage: include/bya.h, "MX weights".  The four big Linears of a DiT block (attn1.to_q|k|v, attn1.to_out,
// ff.net.0.proj, ff.net.2 -- models/transformer.py:241-260) when the engine is built with MX weights
// (enable_mx_weights).  No reference counterpart; parity is against the CPU restatement on the same bytes
// (tests/test_mx_gpu.py).
//
// v_mfma_scale_f32_16x16x128_f8f6f4: 128 k per instruction; the scale VGPR of lane l carries the scale of row l & 15 for
// K-block l >> 4 of the step (byte selected by op_sel; the kernel shifts the lane's byte into position 0).  Which k a lane's
// operand VGPRs hold depends on the element width -- measured with one-hot W and a distinct scale per block
// (tests/test_mx_gpu.py, operand-map test on exact data):
//   - e2m3: six VGPRs = the 24 bytes of block l >> 4, element i at bits 6i.. (runs at the fp4 rate, twice the e4m3 rate);
//   - e4m3: VGPRs 0-3 hold k = 16 (l >> 4) .. +15, VGPRs 4-7 hold k = 64 + 16 (l >> 4) .. +15 -- the instruction's 32-k
//     block b is then bytes 16 b .. 16 b + 15 of the first and of the second 64-k half of lanes 32 (b / 2) ..., so a lane
//     filled with one contiguous 32-byte block (the layout of gemm_fp8_kernel.h, correct there only because its scales are
//     all 2^0) gets the wrong scale on half its bytes.  The kernel reads 16-byte chunks g and 4 + g of the K-tile for lane
//     group g: the instruction's block b is then exactly k = 32 b .. 32 b + 31 of the tile, as stored;
//   - e2m1 (the W operand only): four VGPRs = the 16 bytes of block l >> 4, element i at bits 4i.. (low nibble first),
//     whichever format the other operand has (tests/test_mxfp4_gpu.py, operand-map test on exact data).
//
// The kernel is the 128 x 128 tile of gemm_fp8_kernel.h (4 waves of 64 x 64, two-stage LDS ring fed by global_load_lds,
// group-M tile order) with real block scales, and for big e2m3 launches the same loop on 256 x 256 tiles (8 waves of
// 64 x 128):
//   - a K-tile is 128 elements = 128 bytes (e4m3: the XOR-swizzled image of the fp8 kernel) or 96 bytes (e2m3: rows stored
//     back to back with chunk pairs swapped on every other group of 8 rows, 16 bytes per lane and DMA instruction, the
//     lane's block read as three 8-byte pieces) or 64 bytes (e2m1 W: rows back to back, one 16-byte read per fragment);
//   - the 4 scale bytes of a row for one K-tile are one dword; the block's 256 rows' dwords ride in the same LDS stage
//     (one 4-byte global_load_lds per wave), so their wait is the ring's own vmcnt(0).
#include "gemm_common.h"
#include "mx_common.h"
#include "options.h"
#include "gemm_tile_qkn_epilogue.h"      // epilogue_mx_qkn: shared with the tiled fp8 kernel

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

constexpr int MX_BK = 128;                 // elements per K-tile (one MFMA step)
constexpr int MX_GROUP_M = 8;              // row-tiles per group of the tile order (as the fp8 kernel)
__host__ __device__ constexpr int mx_tile_row_bytes(int fmt) { return fmt == MX_E4M3 ? 128 : fmt == MX_E2M3 ? 96 : 64; }
// 16-byte global_load_lds instructions of one wave for ROWS rows of a K-tile
__host__ __device__ constexpr int mx_stage_dmas(int fmt, int rows, int nwaves) {
    return fmt == MX_E4M3 ? rows / nwaves / 8 : rows * mx_tile_row_bytes(fmt) / 1024 / nwaves;
}
// e2m3 launches of >= 200 256 x 256 tiles run on 256 x 256 tiles (8 waves, one workgroup per CU, half the L2 -> LDS bytes
// per FLOP of the 128 x 128 tile: 572 vs 699 us at q|k|v, 706 vs 978 us at ff.net.2), everything else on 128 x 128 tiles.
// The ring is two stages deep; three (a counted wait keeping the next K-tile's DMA in flight across the barrier) measured
// no faster, so DMA latency is not the bound.  Side builds flip both (tools/mx_gemm_ablate.py).
#ifndef BYA_MX_E2M3_STAGES
#define BYA_MX_E2M3_STAGES 2
#endif
static_assert(BYA_MX_E2M3_STAGES == 2 || BYA_MX_E2M3_STAGES == 3, "e2m3 ring: two or three stages");
#ifndef BYA_MX_E2M3_BIG_TILE
#define BYA_MX_E2M3_BIG_TILE 1
#endif
__host__ __device__ constexpr int mx_stages(int fmt) { return fmt == MX_E4M3 ? 2 : BYA_MX_E2M3_STAGES; }

// ROWS x RB bytes of one K-tile into LDS, 1 KiB per wave-instruction.
template <int FMT, int ROWS, int NWAVES>
__device__ __forceinline__ void stage_mx(const uint8_t* __restrict__ src, int ld, int row0, int row_max, int kb0,
                                         char* lds_tile, int wave, int lane) {
    if constexpr (FMT == MX_E4M3) {
        // 8 rows per instruction; 16-byte chunk c of row r lands at chunk c ^ ((r >> 1) & 7)
        constexpr int PER_WAVE = ROWS / NWAVES;
#pragma unroll
        for (int q = 0; q < PER_WAVE / 8; ++q) {
            const int rbase = wave * PER_WAVE + q * 8;
            const int rl = rbase + (lane >> 3);
            const int chunk = (lane & 7) ^ ((rl >> 1) & 7);
            int gr = row0 + rl;
            gr = gr < row_max ? gr : row_max;
            const uint8_t* g = src + (long long)gr * ld + kb0 + chunk * 16;
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(g), LDS_PTR(lds_tile + rbase * 128), 16, 0, 0);
        }
    } else if constexpr (FMT == MX_E2M1) {
        // 64-byte rows back to back, 16 rows per instruction: a row of the K-tile is one L2 sector.  16-byte chunk c of row r
        // lands at chunk c ^ (((r >> 2) & 1) << 1): unswizzled, rows r and r + 12 (and r + 4, r + 8 of the next lane group) of
        // one ds_read_b128 lane group {0-3, 12-15, 20-27} hit the same 16-byte slot of the 256-byte bank row -- a 2-way
        // conflict on every fragment read; with the XOR the 16 lanes of each group cover the 16 slots once
        constexpr int RB = 64, INSTR = ROWS * RB / 1024, PER_WAVE = INSTR / NWAVES;
        static_assert(INSTR % NWAVES == 0, "tile must split evenly over the waves");
#pragma unroll
        for (int q = 0; q < PER_WAVE; ++q) {
            const int qi = wave * PER_WAVE + q;
            const int rl = qi * 16 + (lane >> 2);
            const int chunk = (lane & 3) ^ (((rl >> 2) & 1) << 1);
            int gr = row0 + rl;
            gr = gr < row_max ? gr : row_max;
            const uint8_t* g = src + (long long)gr * ld + kb0 + chunk * 16;
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(g), LDS_PTR(lds_tile + qi * 1024), 16, 0, 0);
        }
    } else {
        // 96-byte rows back to back: byte t of the tile is row t / 96, offset t % 96 (a multiple of 16).  16-byte chunk c of
        // row r lands at chunk c ^ ((r >> 3) & 1) (pairs 0|1, 2|3, 4|5 stay in the row): rows r and r + 8, 768 bytes apart, hit
        // the same banks unswizzled -- a 2-way conflict on every fragment read
        constexpr int RB = 96, INSTR = ROWS * RB / 1024, PER_WAVE = INSTR / NWAVES;
        static_assert(INSTR % NWAVES == 0, "tile must split evenly over the waves");
#pragma unroll
        for (int q = 0; q < PER_WAVE; ++q) {
            const int qi = wave * PER_WAVE + q;
            const int t = qi * 1024 + lane * 16;
            const int rl = t / RB, off = t - rl * RB;
            int gr = row0 + rl;
            gr = gr < row_max ? gr : row_max;
            const uint8_t* g = src + (long long)gr * ld + kb0 + (off ^ (((rl >> 3) & 1) << 4));
            __builtin_amdgcn_global_load_lds(GLOBAL_PTR(g), LDS_PTR(lds_tile + qi * 1024), 16, 0, 0);
        }
    }
}

// lane group g's operand of one row (e4m3: k = 16 g .. +15 and 64 + 16 g .. +15; e2m3, e2m1: block g = k = 32 g .. 32 g + 31)
template <int FMT>
__device__ __forceinline__ i32x8 lds_frag_mx(const char* tile, int row, int g) {
    if constexpr (FMT == MX_E4M3) {
        const int sw = (row >> 1) & 7;
        const i32x4 lo = *reinterpret_cast<const i32x4*>(tile + row * 128 + ((g ^ sw) << 4));
        const i32x4 hi = *reinterpret_cast<const i32x4*>(tile + row * 128 + (((4 + g) ^ sw) << 4));
        return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    } else if constexpr (FMT == MX_E2M1) {
        const i32x4 b = *reinterpret_cast<const i32x4*>(tile + row * 64 + ((g ^ (((row >> 2) & 1) << 1)) << 4));
        return i32x8{b[0], b[1], b[2], b[3], 0, 0, 0, 0};
    } else {
        const char* r = tile + row * 96;
        const int x = ((row >> 3) & 1) << 4, o = g * 24;                    // (the staging's chunk swizzle)
        const i32x2 p0 = *reinterpret_cast<const i32x2*>(r + (o ^ x));
        const i32x2 p1 = *reinterpret_cast<const i32x2*>(r + ((o + 8) ^ x));
        const i32x2 p2 = *reinterpret_cast<const i32x2*>(r + ((o + 16) ^ x));
        return i32x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], 0, 0};
    }
}

// ---- the quantising epilogue (bya_gemm_mx_quant): the tile leaves as MX codes + scale bytes instead of bf16.
// Per element  v = bf16( alpha * act(acc + rowscale * bias) )  -- the value the bf16 epilogue stores and bya_quantize_mx reads
// back --, then the block rule of mx_common.h on it (mx_quant8_bits: the quantisers' own arithmetic).  A 32-column block of
// row m is the eight values of the four lanes fr + 16 fq, fq = 0..3, in the fragment pair i = 2 b, 2 b + 1: lane fq holds
// elements 4 fq .. 4 fq + 3 (i even) and 16 + 4 fq .. + 3 (i odd) of the block.  Its |max| is the lane's own eight, then the
// lane ^ 16 and lane ^ 32 partners (v_permlane16_swap / v_permlane32_swap; a maximum does not depend on the order).  Handed
// to mx_quant8_bits as "elements 0..3 | 4..7", the low half of the result is the lane's four codes of the even fragment and
// the high half those of the odd one: 4 bytes each at bytes 4 fq and 16 + 4 fq of an e4m3 block, 24 bits each at bytes 3 fq
// and 12 + 3 fq of an e2m3 block.
// Staging (the K-loop's ring is free after one barrier): both formats write ONE DWORD per four codes (e2m3: 24 bits, top byte
// zero) at byte n_local of row m_local, rows BN + 16 bytes apart -- 36 or 68 dwords, so the 16 rows of a ds_write_b32's 32-lane
// half fall on banks 4 r + fq (mod 32): 2-way, which costs a b32 write nothing.  Then the whole block reads the image back in
// 16-byte pieces of OUTPUT row segments, thread t -> piece t % CH of row t / CH, and stores 16 bytes per lane: e4m3 pieces are
// the staged bytes (one ds_read_b128), an e2m3 piece k of a 48-byte block pair is bits 128 k .. 128 k + 127 of the pair's
// sixteen 24-bit words = words 5 k .. 5 k + 5 shifted down by 8 k bits.  The scale bytes ride behind the codes, [BM][BN / 32].
template <int QOUT, int BN> struct MxQuantStage {
    static constexpr int PITCH = BN + 16;                                   // bytes of a staged row of codes
    static constexpr int CH = QOUT == MX_E4M3 ? BN / 16 : BN * 3 / 64;      // 16-byte pieces of an output row segment
    __host__ __device__ static constexpr int bytes(int BM) { return BM * PITCH + BM * (BN / 32); }
};

template <int ACT, int QOUT, int BM, int BN, int NI, int MI, int NTHREADS>
__device__ __forceinline__ void epilogue_mx_quant(const GemmArgs& p, uint8_t* __restrict__ qs, int z, int m0, int n0,
                                                  int ml, int nl, int fq, const f32x4 (&acc)[NI][MI], char* smem, int tid) {
    using St = MxQuantStage<QOUT, BN>;
    static_assert(QOUT == MX_E4M3 || QOUT == MX_E2M3, "activation formats only");
    static_assert(NI % 2 == 0 && (BM * St::CH) % NTHREADS == 0, "whole blocks per wave, whole pieces per thread");
    constexpr int PITCH = St::PITCH, CH = St::CH, SB = BN / 32;
    uint8_t* sc = reinterpret_cast<uint8_t*>(smem) + BM * PITCH;
    const bool has_bias = p.bias != nullptr, has_rs = p.bias_rowscale != nullptr;
    float rs[MI];
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const int m = m0 + ml + 16 * j;
        rs[j] = has_rs ? p.bias_rowscale[(long long)z * p.M + (m < p.M ? m : 0)] : 1.0f;
    }
    u32x2 bv[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int n4 = n0 + nl + 16 * i;
        bv[i] = has_bias ? *reinterpret_cast<const u32x2*>(p.bias + (n4 < p.N ? n4 : 0)) : u32x2{0u, 0u};
    }
    __syncthreads();                                     // every wave has read its last K-tile: the ring is free
#pragma unroll
    for (int b = 0; b < NI / 2; ++b) {
#pragma unroll
        for (int j = 0; j < MI; ++j) {
            float v[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const u32x2 bb = bv[2 * b + h];
                const float b4[4] = {bflo(bb[0]), bfhi(bb[0]), bflo(bb[1]), bfhi(bb[1])};
                float t[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    t[e] = p.alpha * apply_act<ACT>(fmaf(rs[j], b4[e], acc[2 * b + h][j][e]), p.leaky);
                const uint32_t r0 = pack2bf(t[0], t[1]), r1 = pack2bf(t[2], t[3]);      // the one rounding to bf16
                v[4 * h] = bflo(r0); v[4 * h + 1] = bfhi(r0); v[4 * h + 2] = bflo(r1); v[4 * h + 3] = bfhi(r1);
            }
            float amax = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
            amax = lane_max32(lane_max16(amax));
            uint32_t sbyte;
            const uint64_t bits = mx_quant8_bits<QOUT>(v, amax, sbyte);
            const uint32_t lo = QOUT == MX_E4M3 ? (uint32_t)bits : (uint32_t)bits & 0xffffffu;
            const uint32_t hi = QOUT == MX_E4M3 ? (uint32_t)(bits >> 32) : (uint32_t)(bits >> 24);
            char* row = smem + (ml + 16 * j) * PITCH + nl + 32 * b;
            *reinterpret_cast<uint32_t*>(row) = lo;
            *reinterpret_cast<uint32_t*>(row + 16) = hi;
            if (fq == 0) sc[(ml + 16 * j) * SB + (nl >> 5) + b] = (uint8_t)sbyte;
        }
    }
    __syncthreads();
    // columns of this tile inside N (N % 128 == 0: whole 128-column groups = whole pieces and whole scale dwords)
    const int ncols = p.N - n0 < BN ? p.N - n0 : BN;
    uint8_t* crow0 = reinterpret_cast<uint8_t*>(p.C) + (long long)z * p.c_bs + (long long)n0 * (QOUT == MX_E4M3 ? 8 : 6) / 8;
#pragma unroll
    for (int q = 0; q < BM * CH / NTHREADS; ++q) {
        const int t = q * NTHREADS + tid, r = t / CH, c = t - r * CH;
        const int m = m0 + r;
        u32x4 o;
        if constexpr (QOUT == MX_E4M3) {
            o = *reinterpret_cast<const u32x4*>(smem + r * PITCH + c * 16);
        } else {
            const int pr = c / 3, k = c - pr * 3;
            const uint32_t* d = reinterpret_cast<const uint32_t*>(smem + r * PITCH + pr * 64) + 5 * k;
            const uint64_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4], d5 = d[5];
            const uint64_t c0 = d0 | (d1 << 24) | (d2 << 48);
            const uint64_t c1 = (d2 >> 16) | (d3 << 8) | (d4 << 32) | (d5 << 56);
            const uint64_t c2 = d5 >> 8;
            const int s = 8 * k;
            const uint64_t o0 = k ? (c0 >> s) | (c1 << (64 - s)) : c0;
            const uint64_t o1 = k ? (c1 >> s) | (c2 << (64 - s)) : c1;
            o[0] = (uint32_t)o0; o[1] = (uint32_t)(o0 >> 32); o[2] = (uint32_t)o1; o[3] = (uint32_t)(o1 >> 32);
        }
        const bool ok = m < p.M && c * 16 < ncols * (QOUT == MX_E4M3 ? 8 : 6) / 8;
        if (ok) *reinterpret_cast<u32x4*>(crow0 + (long long)m * p.ldc + c * 16) = o;
    }
    // scale bytes: one dword per row and 128 columns
    for (int t = tid; t < BM * (SB / 4); t += NTHREADS) {
        const int r = t / (SB / 4), w = t - r * (SB / 4);
        const int m = m0 + r;
        if (m < p.M && w * 128 < ncols)
            *reinterpret_cast<uint32_t*>(qs + ((long long)z * p.M + m) * (p.N / 32) + n0 / 32 + 4 * w) =
                *reinterpret_cast<const uint32_t*>(sc + r * SB + 4 * w);
    }
}

// FMT_A: activations (the instruction's B operand, blgp); FMT_W: weights (its A operand, cbsz); QOUT = MX_EPI_BF16: the bf16
// epilogue, MX_EPI_QKN: the q/k-norm one (p.qkn_*); else the element format of the quantising one (qs = its scale bytes)
template <int FMT_A, int FMT_W, int BM, int BN, int WAVES_M, int WAVES_N, int QOUT>
__device__ __forceinline__ void gemm_mx_body(const GemmArgs& p, const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sw,
                                             int GM, uint8_t* __restrict__ qs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NWAVES = WAVES_M * WAVES_N, RB_A = mx_tile_row_bytes(FMT_A), RB_W = mx_tile_row_bytes(FMT_W);
    constexpr int TILE_A = BM * RB_A, TILE_W = BN * RB_W, SCALES = (BM + BN) * 4, STAGE = TILE_A + TILE_W + SCALES;
    static_assert(BM + BN == 64 * WAVES_M * WAVES_N, "one scale row per lane of the block");
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, MI = WM / 16, NI = WN / 16;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    const int id = xcd_remap(blockIdx.x, nwg);
    const int per_group = GM * tiles_n;
    const int group = id / per_group, first_m = group * GM;
    const int gsz = (tiles_m - first_m) < GM ? (tiles_m - first_m) : GM;
    const int in_g = id - group * per_group;
    const int tm = first_m + in_g % gsz, tn = in_g / gsz;
    const int m0 = tm * BM, n0 = tn * BN;
    const int z = blockIdx.z;

    const uint8_t* A = reinterpret_cast<const uint8_t*>(p.A) + (long long)z * p.a_bs;
    const uint8_t* W = reinterpret_cast<const uint8_t*>(p.W);
    const int nk = p.K / MX_BK, ks = p.K / 32;          // K-tiles; scale bytes per row

    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int fr = lane & 15, fq = lane >> 4;

    // The K-tile's 4 scale bytes of every A and W row travel through the LDS ring with the codes: one 4-byte DMA per lane
    // (lane t of the block: A row t, or W row t - BM), clamped like the staged rows.  (Eight scattered dword loads per wave and
    // K-tile straight into registers doubled the kernel's time: DESIGN.md section 11.)
    const uint8_t* srow;
    {
        const bool is_a = tid < BM;
        const int r = is_a ? m0 + tid : n0 + tid - BM, rmax = is_a ? p.M - 1 : p.N - 1;
        srow = is_a ? sa + ((long long)z * p.M + (r < rmax ? r : rmax)) * ks : sw + (long long)(r < rmax ? r : rmax) * ks;
    }
    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * STAGE;
        stage_mx<FMT_A, BM, NWAVES>(A, p.lda, m0, p.M - 1, kt * RB_A, base, wave, lane);
        stage_mx<FMT_W, BN, NWAVES>(W, p.ldw, n0, p.N - 1, kt * RB_W, base + TILE_A, wave, lane);
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(srow + 4 * kt), LDS_PTR(base + TILE_A + TILE_W + wave * 256), 4, 0, 0);
    };

    f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int sh = 8 * fq;                               // this lane's block within the K-tile -> its scale byte
    // Ring of NST stages (by the activation format).  Two deep (e4m3): every K-tile waits for all its loads, then one barrier.  Three deep (e2m3): the
    // wait is counted -- the loads of the next K-tile stay in flight across the barrier (a raw s_barrier: __syncthreads
    // would make hipcc drain them), so a K-tile's DMA has two K-tiles of compute to land in instead of none.
    constexpr int NST = mx_stages(FMT_A);
    constexpr int VM_STAGE = mx_stage_dmas(FMT_A, BM, NWAVES) + mx_stage_dmas(FMT_W, BN, NWAVES) + 1;           // DMAs per wave
    for (int s0 = 0; s0 < NST - 1 && s0 < nk; ++s0) stage(s0, s0);
    for (int kt = 0; kt < nk; ++kt) {
        if constexpr (NST == 2) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        } else {
            if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(VM_STAGE) : "memory");   // K-tile kt landed
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();               // ... for every wave, and every wave is done with stage (kt - 1) % NST
        }
        if (kt + NST - 1 < nk) stage(kt + NST - 1, (kt + NST - 1) % NST);
        const char* ta = smem + (kt % NST) * STAGE;
        const char* tw = ta + TILE_A;
        const uint32_t* ts = reinterpret_cast<const uint32_t*>(tw + TILE_W);
        int xa[MI], xw[NI];
#pragma unroll
        for (int j = 0; j < MI; ++j) xa[j] = (int)(ts[wm * WM + j * 16 + fr] >> sh);
#pragma unroll
        for (int i = 0; i < NI; ++i) xw[i] = (int)(ts[BM + wn * WN + i * 16 + fr] >> sh);
        i32x8 fa[MI], fw[NI];
#pragma unroll
        for (int j = 0; j < MI; ++j) fa[j] = lds_frag_mx<FMT_A>(ta, wm * WM + j * 16 + fr, fq);
#pragma unroll
        for (int i = 0; i < NI; ++i) fw[i] = lds_frag_mx<FMT_W>(tw, wn * WN + i * 16 + fr, fq);
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < MI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fa[j], acc[i][j], FMT_W, FMT_A,
                                                                             0, xw[i], 0, xa[j]);
    }

    // Lane holds C[m][n4 .. n4+3], m = m_base + 16 j, n4 = n_base + 16 i (W fragment = the instruction's A operand)
    const int m_base = m0 + wm * WM + fr, n_base = n0 + wn * WN + fq * 4;
    if constexpr (QOUT == MX_EPI_BF16) {
        auto run = [&](auto act_tag) {
            epilogue_block<decltype(act_tag)::value, NI, MI, (NI * MI > 16 ? 1 : NI)>(p, z, m_base, n_base, acc);
        };
        dispatch_act_big(p.act, run);
    } else if constexpr (QOUT == MX_EPI_QKN) {
        epilogue_mx_qkn<NI, MI, BYA_MX_QKN_STORE16 != 0>(p, z, m_base, n0 + wn * WN, fq, acc);
    } else {
        static_assert(MxQuantStage<QOUT, BN>::bytes(BM) <= NST * STAGE, "the staged tile must fit the K-loop's ring");
        auto run = [&](auto act_tag) {
            epilogue_mx_quant<decltype(act_tag)::value, QOUT, BM, BN, NI, MI, 64 * NWAVES>(
                p, qs, z, m0, n0, wm * WM + fr, wn * WN + fq * 4, fq, acc, smem, tid);
        };
        dispatch_act_big(p.act, run);
    }
}

template <int FMT_A, int FMT_W, int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_mx_kernel(GemmArgs p, const uint8_t* __restrict__ sa,
                                                                         const uint8_t* __restrict__ sw, int GM) {
    gemm_mx_body<FMT_A, FMT_W, BM, BN, WAVES_M, WAVES_N, MX_EPI_BF16>(p, sa, sw, GM, nullptr);
}

// ... with the quantising epilogue: C = codes (ldc, c_bs in bytes), qs = scale bytes [batch * M, N / 32]
template <int FMT_A, int FMT_W, int BM, int BN, int WAVES_M, int WAVES_N, int QOUT>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_mx_quant_kernel(GemmArgs p, const uint8_t* __restrict__ sa,
                                                                               const uint8_t* __restrict__ sw, int GM,
                                                                               uint8_t* __restrict__ qs) {
    gemm_mx_body<FMT_A, FMT_W, BM, BN, WAVES_M, WAVES_N, QOUT>(p, sa, sw, GM, qs);
}

// ... with the q/k-norm epilogue (GemmArgs::qkn_*)
template <int FMT_A, int FMT_W, int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_mx_qkn_kernel(GemmArgs p, const uint8_t* __restrict__ sa,
                                                                             const uint8_t* __restrict__ sw, int GM) {
    gemm_mx_body<FMT_A, FMT_W, BM, BN, WAVES_M, WAVES_N, MX_EPI_QKN>(p, sa, sw, GM, nullptr);
}

// The six operand instances of the tiled kernel: e4m3 / e2m3 activations x weights in the same format or in e2m1, the e2m3 ones
// on 128 x 128 or (big) 256 x 256 tiles.  f(MxInst<...>{}) is called for the one that (a_fmt, w_fmt, big) names.
template <int FMT_A_, int FMT_W_, int BM_, int BN_, int WAVES_M_, int WAVES_N_> struct MxInst {
    static constexpr int FMT_A = FMT_A_, FMT_W = FMT_W_, BM = BM_, BN = BN_, WAVES_M = WAVES_M_, WAVES_N = WAVES_N_;
};
template <typename F>
int mx_for_instance(int32_t a_fmt, int32_t w_fmt, bool big, F&& f) {
    const bool w4 = w_fmt == MX_E2M1;
    if (a_fmt == MX_E4M3) return w4 ? f(MxInst<MX_E4M3, MX_E2M1, 128, 128, 2, 2>{}) : f(MxInst<MX_E4M3, MX_E4M3, 128, 128, 2, 2>{});
    if (big) return w4 ? f(MxInst<MX_E2M3, MX_E2M1, 256, 256, 4, 2>{}) : f(MxInst<MX_E2M3, MX_E2M3, 256, 256, 4, 2>{});
    return w4 ? f(MxInst<MX_E2M3, MX_E2M1, 128, 128, 2, 2>{}) : f(MxInst<MX_E2M3, MX_E2M3, 128, 128, 2, 2>{});
}

// One launch of instance I of the tiled kernel with epilogue EPI (MX_EPI_BF16, MX_EPI_QKN, or the quantising epilogue's element
// format; qs: its scale bytes, else unused)
template <typename I, int EPI>
int launch_mx(const GemmArgs& a, const uint8_t* sa, const uint8_t* sw, uint8_t* qs, int batch, hipStream_t s) {
    constexpr int FMT_A = I::FMT_A, FMT_W = I::FMT_W, BM = I::BM, BN = I::BN, WAVES_M = I::WAVES_M, WAVES_N = I::WAVES_N;
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
    dim3 grid(tiles_m * tiles_n, 1, batch);
    // the ring: per stage the two code tiles and one scale dword per row
    const size_t lds = (size_t)mx_stages(FMT_A) * (BM * (mx_tile_row_bytes(FMT_A) + 4) + BN * (mx_tile_row_bytes(FMT_W) + 4));
    static std::atomic<unsigned long long> attr_done{0};
    auto go = [&](auto kern, auto... tail) {
        if (bya_allow_big_lds(reinterpret_cast<const void*>(kern), (int)lds, attr_done) != BYA_OK) return (int)BYA_ERR_LAUNCH;
        BYA_LAUNCH(kern, grid, dim3(64 * WAVES_M * WAVES_N), lds, s, a, sa, sw, MX_GROUP_M, tail...);
        return hipGetLastError() == hipSuccess ? (int)BYA_OK : (int)BYA_ERR_LAUNCH;
    };
    if constexpr (EPI == MX_EPI_BF16) return go(gemm_mx_kernel<FMT_A, FMT_W, BM, BN, WAVES_M, WAVES_N>);
    else if constexpr (EPI == MX_EPI_QKN) return go(gemm_mx_qkn_kernel<FMT_A, FMT_W, BM, BN, WAVES_M, WAVES_N>);
    else return go(gemm_mx_quant_kernel<FMT_A, FMT_W, BM, BN, WAVES_M, WAVES_N, EPI>, qs);
}

// ---- standalone quantiser: one lane per 8 consecutive elements (one 16-byte load), a lane quad per block.
template <int FMT>
__global__ __launch_bounds__(256) void quantize_mx_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ q,
                                                          uint8_t* __restrict__ scales, long long M, int K, long long ldx) {
    const long long per_row = K / 8, total = M * per_row;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = gid < total;                       // (total % 4 == 0: a quad is all in or all out)
    const long long row = ok ? gid / per_row : 0;
    const int c = ok ? (int)(gid - row * per_row) : 0;
    float v[8];
    if (ok) unpack8(*reinterpret_cast<const u32x4*>(x + row * ldx + c * 8), v);
    else
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
    amax = quad_amax(amax);
    if (!ok) return;
    const long long row_bytes = (long long)K / 32 * mx_block_bytes(FMT);
    const int part = c & 3, blk = c >> 2;
    uint8_t* dst = q + row * row_bytes + (long long)blk * mx_block_bytes(FMT) + part * (mx_block_bytes(FMT) / 4);
    const uint32_t sb = mx_quant8<FMT>(v, amax, dst);
    if (part == 0) scales[row * (K / 32) + blk] = (uint8_t)sb;
}

}  // namespace

extern "C" int bya_quantize_mx(const void* x, void* codes, void* scales, int32_t M, int32_t K, int64_t ldx, int32_t fmt,
                               hipStream_t stream) {
    if (!x || !codes || !scales || M <= 0 || K <= 0 || K % 128) return BYA_ERR_SHAPE;
    if (fmt != MX_E4M3 && fmt != MX_E2M3 && fmt != MX_E2M1) return BYA_ERR_SHAPE;
    if (ldx < K || ldx % 8 || ((uintptr_t)x & 15) || ((uintptr_t)codes & 7)) return BYA_ERR_ALIGN;
    const long long total = (long long)M * (K / 8);
    dim3 grid((unsigned)((total + 255) / 256));
    if (fmt == MX_E4M3)
        BYA_LAUNCH(quantize_mx_kernel<MX_E4M3>, grid, dim3(256), 0, stream, (const bf16_t*)x, (uint8_t*)codes,
                   (uint8_t*)scales, (long long)M, K, (long long)ldx);
    else if (fmt == MX_E2M3)
        BYA_LAUNCH(quantize_mx_kernel<MX_E2M3>, grid, dim3(256), 0, stream, (const bf16_t*)x, (uint8_t*)codes,
                   (uint8_t*)scales, (long long)M, K, (long long)ldx);
    else
        BYA_LAUNCH(quantize_mx_kernel<MX_E2M1>, grid, dim3(256), 0, stream, (const bf16_t*)x, (uint8_t*)codes,
                   (uint8_t*)scales, (long long)M, K, (long long)ldx);
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}

namespace {
// bya_gemm_mx_mixed's arguments -> GemmArgs; BYA_OK or the error that rejects them
int mx_args(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, const void* C,
            const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d, int32_t a_fmt, int32_t w_fmt,
            GemmArgs* out) {
    if (!A || !W || !a_scales || !w_scales || !C || !d) return BYA_ERR_SHAPE;
    // activations e4m3 / e2m3; weights in the same format or in e2m1
    if ((a_fmt != MX_E4M3 && a_fmt != MX_E2M3) || (w_fmt != a_fmt && w_fmt != MX_E2M1)) return BYA_ERR_UNSUPPORTED;
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->batch <= 0) return BYA_ERR_SHAPE;
    if (d->K % MX_BK != 0 || d->N % 4 != 0) return BYA_ERR_SHAPE;
    if ((long long)d->batch * d->M * (d->K / 32) >= (1LL << 31) || (long long)d->N * (d->K / 32) >= (1LL << 31))
        return BYA_ERR_SHAPE;
    if (d->lda < d->K / 32 * mx_block_bytes(a_fmt) || d->ldw < d->K / 32 * mx_block_bytes(w_fmt)) return BYA_ERR_SHAPE;
    if (d->lda % 16 || d->ldw % 16 || d->a_batch_stride % 16) return BYA_ERR_ALIGN;
    if (((uintptr_t)A | (uintptr_t)W) & 15) return BYA_ERR_ALIGN;
    if (((uintptr_t)a_scales | (uintptr_t)w_scales) & 3) return BYA_ERR_ALIGN;
    const int rc = gemm_epilogue_check(C, res, bias, gate0, gate1, d, act_on_big_tiles(d->act));      // none / GELU(tanh): the DiT Linears
    if (rc != BYA_OK) return rc;
    gemm_fill_args(A, W, bias, C, res, gate0, gate1, d, out);
    return BYA_OK;
}

// What may take the persistent kernel of gemm_mx_v4.hip.  kernel: 0 = nothing, 1 = launches that fill it (the rule of fp8_path,
// gemm_fp8.hip), 2 = without the tile count (tests); it is admitted for e4m3 x e4m3 always, and
//   w4:  for e2m1 weights under e4m3 activations as well (its FMT_W = MX_E2M1 instances),
//   fp6: for e2m3 activations (weights e2m3 or e2m1) and / or e2m3 output of the quantising epilogue as well (its FMT_A = MX_E2M3 /
//        QOUT = MX_E2M3 instances).
// bya_gemm_mx_call says all three in its `kernel` ARGUMENT (no option is read; w4 always, fp6 under BYA_MX_KERNEL_FP6).  The older
// entry points name the kernel only -- option mx_kernel, bya_gemm_mx_qkv_norm_rope_on its argument -- and admit nothing else: what
// they and their plan queries answer for e2m1 weights and for e2m3 is pinned to the tiled kernel.
struct MxKernel { int kernel; bool w4, fp6; };
inline MxKernel mx_kernel_option() { return MxKernel{bya_opt(BYA_OPT_MX_KERNEL), false, false}; }      // (read per launch)

// The kernel of one MX GEMM launch.  By the activation format: e4m3 on 128 x 128 tiles; e2m3 on 256 x 256 tiles when the launch
// has about a round of 256 CUs of them, or more; the persistent kernel where `k` admits the launch and it is eligible.  `a` = the
// whole launch (tile count), `piece` = one row chunk of it (eligibility); epi: MX_EPI_BF16, MX_EPI_QKN, or the quantising
// epilogue's element format.
inline int mx_path(const GemmArgs& a, int batch, const GemmArgs& piece, int32_t a_fmt, int32_t w_fmt, int epi, MxKernel k) {
    const long long tiles256 = (long long)((a.M + 255) / 256) * ((a.N + 255) / 256) * batch;
    const bool fp6 = a_fmt == MX_E2M3 || epi == MX_E2M3;
    const bool w_ok = a_fmt == MX_E4M3 ? w_fmt == MX_E4M3 || (k.w4 && w_fmt == MX_E2M1) : true;             // (mx_args: e2m3 or e2m1)
    if (k.kernel != 0 && w_ok && (!fp6 || k.fp6) && (k.kernel == 2 || tiles256 >= 200) &&
        bya_gemm256p_mx_eligible(&piece, epi >= 0))
        return BYA_GEMM_PATH_P256;
    return a_fmt == MX_E2M3 && BYA_MX_E2M3_BIG_TILE && tiles256 >= 200 ? BYA_GEMM_PATH_T256X256 : BYA_GEMM_PATH_T128X128;
}
constexpr int MX_P256_GROUP_M = 4;         // row-tiles per group of the persistent kernel's tile order (as bya_gemm_fp8)

// One launch on the kernel that `path` (mx_path) names, with epilogue epi: MX_EPI_BF16, MX_EPI_QKN, or the quantising epilogue's
// element format (qs: its scale bytes)
int mx_launch(int path, const GemmArgs& a, const uint8_t* sa, const uint8_t* sw, uint8_t* qs, int epi, int32_t a_fmt,
              int32_t w_fmt, int batch, hipStream_t s) {
    if (path == BYA_GEMM_PATH_P256) return bya_launch_gemm256p_mx(&a, sa, sw, qs, epi, a_fmt, w_fmt, batch, MX_P256_GROUP_M, s);
    return mx_for_instance(a_fmt, w_fmt, path == BYA_GEMM_PATH_T256X256, [&](auto inst) {
        using I = decltype(inst);
        if (epi == MX_EPI_BF16) return launch_mx<I, MX_EPI_BF16>(a, sa, sw, qs, batch, s);
        if (epi == MX_EPI_QKN) return launch_mx<I, MX_EPI_QKN>(a, sa, sw, qs, batch, s);
        return epi == MX_E4M3 ? launch_mx<I, MX_E4M3>(a, sa, sw, qs, batch, s) : launch_mx<I, MX_E2M3>(a, sa, sw, qs, batch, s);
    });
}

// bya_gemm_mx_quant's arguments -> GemmArgs (C = the codes; ldc, c_bs in bytes); BYA_OK or the error that rejects them
int mx_quant_args(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                  const void* q_codes, const void* q_scales, const bya_gemm_desc* d, int32_t a_fmt, int32_t w_fmt,
                  int32_t out_fmt, GemmArgs* out) {
    if (!A || !W || !a_scales || !w_scales || !q_codes || !q_scales || !d) return BYA_ERR_SHAPE;
    if (out_fmt != MX_E4M3 && out_fmt != MX_E2M3) return BYA_ERR_UNSUPPORTED;       // e2m1 is never an activation format
    if ((a_fmt != MX_E4M3 && a_fmt != MX_E2M3) || (w_fmt != a_fmt && w_fmt != MX_E2M1)) return BYA_ERR_UNSUPPORTED;
    if (d->n_split != 0) return BYA_ERR_UNSUPPORTED;                                 // a codes tensor has no column split
    if (d->N <= 0 || d->N % 128 != 0) return BYA_ERR_SHAPE;                          // the result is a legal K
    const long long row_bytes = (long long)d->N / 32 * mx_block_bytes(out_fmt);
    if (d->ldc < row_bytes) return BYA_ERR_SHAPE;
    if (d->M > 0 && d->batch > 0 && (long long)d->batch * d->M * (d->N / 32) >= (1LL << 31)) return BYA_ERR_SHAPE;
    if (d->ldc % 16 || d->c_batch_stride % 16 || ((uintptr_t)q_codes & 15) || ((uintptr_t)q_scales & 3)) return BYA_ERR_ALIGN;
    bya_gemm_desc e = *d;                                // the operand side: bya_gemm_mx_mixed's own checks
    e.ldres = 0; e.res_batch_stride = 0; e.gate_batch_stride = 0; e.gate_split = 0; e.c_split_stride = 0;
    return mx_args(A, a_scales, W, w_scales, bias, q_codes, nullptr, nullptr, nullptr, &e, a_fmt, w_fmt, out);
}

// bya_gemm_mx_qkv_norm_rope's arguments -> GemmArgs; BYA_ERR_UNSUPPORTED: not this epilogue's shape (the caller keeps
// bya_gemm_mx_mixed + bya_qknorm_rope); malformed arguments: the errors of qkn_norm_desc_check / qkn_head_args (gemm_common.h) and mx_args
int mx_qkn_args(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, const void* C,
                const bya_gemm_desc* d, const bya_qknorm_desc* n, const QknStats& st, int32_t a_fmt, int32_t w_fmt, GemmArgs* out) {
    const int rc0 = qkn_norm_desc_check(d, n);
    if (rc0 != BYA_OK) return rc0;
    const int rcs = qkn_stats_check(st);
    if (rcs != BYA_OK) return rcs;
    bya_gemm_desc e = *d;                                // the operand side: bya_gemm_mx_mixed's own checks
    e.ldres = 0; e.res_batch_stride = 0; e.gate_batch_stride = 0; e.gate_split = 0;
    const int rc = mx_args(A, a_scales, W, w_scales, bias, C, nullptr, nullptr, nullptr, &e, a_fmt, w_fmt, out);
    if (rc != BYA_OK) return rc;
    return qkn_head_args(C, d, n, st, out);              // (gemm_common.h: shared with bya_gemm_fp8_qkv_norm_rope)
}

// Every MX GEMM entry point of this file, launch (plan == nullptr) and plan query: one body, so the query answers what the
// launch does.  The epilogue is the one `c` names (norm: q/k-norm + RoPE; q_scales: quantising; else bf16); its own argument
// function refuses what it always refused, with its code; then mx_path with what `k` admits to the persistent kernel
// (c->kernel itself is not read here).  Only the bf16 epilogue is cut into row chunks: the q/k-norm launch is one piece by its
// argument check, and the quantising epilogue stores through 64-bit addresses.
// `st`: the score-bound statistics of the q/k-norm epilogue (bya_gemm_mx_qkv_norm_rope_stats alone passes a table).
int mx_call(const bya_mx_gemm_call* c, const bya_gemm_desc* d, MxKernel k, hipStream_t stream, bya_gemm_plan* plan,
            const QknStats& st = QknStats{}) {
    if (!c || !d) return BYA_ERR_SHAPE;
    if (c->norm && c->q_scales) return BYA_ERR_SHAPE;
    if ((c->norm || c->q_scales) && (c->res || c->gate0 || c->gate1)) return BYA_ERR_SHAPE;
    GemmArgs a;
    int rc, epi = MX_EPI_BF16;
    if (c->norm) {
        rc = mx_qkn_args(c->A, c->a_scales, c->W, c->w_scales, c->bias, c->C, d, c->norm, st, c->a_fmt, c->w_fmt, &a);
        epi = MX_EPI_QKN;
    } else if (c->q_scales) {
        rc = mx_quant_args(c->A, c->a_scales, c->W, c->w_scales, c->bias, c->C, c->q_scales, d, c->a_fmt, c->w_fmt, c->out_fmt, &a);
        epi = c->out_fmt;
    } else {
        rc = mx_args(c->A, c->a_scales, c->W, c->w_scales, c->bias, c->C, c->res, c->gate0, c->gate1, d, c->a_fmt, c->w_fmt, &a);
    }
    if (rc != BYA_OK) return rc;
    const long long ks = d->K / 32;
    auto run = [&](const GemmArgs& piece, int batch, long long row0) {
        const int path = mx_path(a, d->batch, piece, c->a_fmt, c->w_fmt, epi, k);
        // the score-bound statistics (bya_gemm_mx_qkv_norm_rope_stats) are the persistent kernel's: the tiled ones decline them
        if (epi == MX_EPI_QKN && a.qkn_stats && path != BYA_GEMM_PATH_P256) return BYA_ERR_UNSUPPORTED;
        if (plan) return gemm_plan_whole(plan, path, 1);
        return mx_launch(path, piece, (const uint8_t*)c->a_scales + row0 * ks, (const uint8_t*)c->w_scales, (uint8_t*)c->q_scales, epi,
                         c->a_fmt, c->w_fmt, batch, stream);
    };
    return epi == MX_EPI_BF16 ? gemm_row_chunks(a, d->batch, 1, plan, run) : run(a, d->batch, 0LL);
}

// bya_gemm_mx_call's kernel argument: 0, 1, 2, or BYA_MX_KERNEL_FP6 + one of them; e2m1 weights are admitted with either
bool mx_kernel_of_call(const bya_mx_gemm_call* c, MxKernel* k) {
    if (!c || c->kernel < 0 || (c->kernel & ~BYA_MX_KERNEL_FP6) > 2) return false;
    *k = MxKernel{c->kernel & ~BYA_MX_KERNEL_FP6, true, (c->kernel & BYA_MX_KERNEL_FP6) != 0};
    return true;
}

// The older entry points: their arguments as a call on the kernel `kernel` names, nothing else admitted to it.  Each keeps the
// checks mx_call has no reason for -- a null q_scales / norm would name another epilogue there.
int mx_mixed(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, const void* C, const void* res,
             const void* gate0, const void* gate1, const bya_gemm_desc* d, int32_t a_fmt, int32_t w_fmt, hipStream_t stream,
             bya_gemm_plan* plan) {
    const bya_mx_gemm_call c = {A, a_scales, W, w_scales, bias, (void*)C, res, gate0, gate1, nullptr, nullptr, a_fmt, w_fmt, MX_E4M3, 0};
    return mx_call(&c, d, mx_kernel_option(), stream, plan);
}

int mx_quant(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, const void* q_codes,
             const void* q_scales, const bya_gemm_desc* d, int32_t a_fmt, int32_t w_fmt, int32_t out_fmt, hipStream_t stream,
             bya_gemm_plan* plan) {
    if (!q_scales) return BYA_ERR_SHAPE;
    const bya_mx_gemm_call c = {A, a_scales, W, w_scales, bias, (void*)q_codes, nullptr, nullptr, nullptr, (void*)q_scales, nullptr,
                                a_fmt, w_fmt, out_fmt, 0};
    return mx_call(&c, d, mx_kernel_option(), stream, plan);
}

int mx_qkn_on(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, const void* C, int32_t fmt,
              int32_t w_fmt, const bya_gemm_desc* d, const bya_qknorm_desc* n, int32_t kernel, hipStream_t stream, bya_gemm_plan* plan) {
    if (!n || kernel < 0 || kernel > 2) return BYA_ERR_SHAPE;            // (16, the flag bit of bya_gemm_mx_call, is no kernel here)
    const bya_mx_gemm_call c = {A, a_scales, W, w_scales, bias, (void*)C, nullptr, nullptr, nullptr, nullptr, n, fmt, w_fmt, MX_E4M3, 0};
    return mx_call(&c, d, MxKernel{kernel, false, false}, stream, plan);
}
}  // namespace

// Any MX GEMM of this file with its kernel named by an ARGUMENT (no option is read): the epilogue is chosen by which of
// `norm` / `q_scales` is set, kernel = 0 is the old entry point of that epilogue under option mx_kernel = 0, and kernel = 1 / 2
// admit e4m3 x e4m3 AND e4m3 x e2m1 launches to the persistent 256 x 256 kernel (gemm_mx_v4.hip), the same bits.  With
// BYA_MX_KERNEL_FP6 added (17 / 18; 16 = 0) launches with e2m3 activations and / or e2m3 output of the quantising epilogue are
// admitted as well, by the same rule; without it they stay on the tiled kernel.
extern "C" int bya_gemm_mx_call(const bya_mx_gemm_call* call, const bya_gemm_desc* desc, hipStream_t stream) {
    MxKernel k;
    if (!mx_kernel_of_call(call, &k)) return BYA_ERR_SHAPE;
    return mx_call(call, desc, k, stream, nullptr);
}

extern "C" int bya_gemm_mx_call_plan(const bya_mx_gemm_call* call, const bya_gemm_desc* desc, bya_gemm_plan* plan) {
    MxKernel k;
    if (!plan || !mx_kernel_of_call(call, &k)) return BYA_ERR_SHAPE;
    return mx_call(call, desc, k, nullptr, plan);
}

// Activations e4m3 / e2m3, weights in the same format or in e2m1; the kernel by option mx_kernel
extern "C" int bya_gemm_mx_mixed(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                                 void* C, const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d,
                                 int32_t a_fmt, int32_t w_fmt, hipStream_t stream) {
    return mx_mixed(A, a_scales, W, w_scales, bias, C, res, gate0, gate1, d, a_fmt, w_fmt, stream, nullptr);
}

extern "C" int bya_gemm_mx_mixed_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                      const void* bias, const void* C, const void* res, const void* gate0, const void* gate1,
                                      const bya_gemm_desc* d, int32_t a_fmt, int32_t w_fmt, bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return mx_mixed(A, a_scales, W, w_scales, bias, C, res, gate0, gate1, d, a_fmt, w_fmt, nullptr, p);
}

// Both operands in one format: e4m3 or e2m3 (e2m1 activations are not offered)
extern "C" int bya_gemm_mx(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                           void* C, const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d,
                           int32_t fmt, hipStream_t stream) {
    if (fmt != MX_E4M3 && fmt != MX_E2M3) return BYA_ERR_SHAPE;
    return mx_mixed(A, a_scales, W, w_scales, bias, C, res, gate0, gate1, d, fmt, fmt, stream, nullptr);
}

extern "C" int bya_gemm_mx_plan(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                                const void* C, const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d,
                                int32_t fmt, bya_gemm_plan* p) {
    if (!p || (fmt != MX_E4M3 && fmt != MX_E2M3)) return BYA_ERR_SHAPE;
    return mx_mixed(A, a_scales, W, w_scales, bias, C, res, gate0, gate1, d, fmt, fmt, nullptr, p);
}

// bya_gemm_mx_mixed whose epilogue writes the MX codes and scale bytes of its bf16-rounded result: byte for byte
// bya_gemm_mx_mixed followed by bya_quantize_mx(out_fmt), without the bf16 tensor.  The stores are plain 64-bit-addressed
// vector stores, so no launch is cut into row chunks.
extern "C" int bya_gemm_mx_quant(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                                 void* q_codes, void* q_scales, const bya_gemm_desc* d, int32_t a_fmt, int32_t w_fmt,
                                 int32_t out_fmt, hipStream_t stream) {
    return mx_quant(A, a_scales, W, w_scales, bias, q_codes, q_scales, d, a_fmt, w_fmt, out_fmt, stream, nullptr);
}

extern "C" int bya_gemm_mx_quant_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                      const void* bias, const void* q_codes, const void* q_scales, const bya_gemm_desc* d,
                                      int32_t a_fmt, int32_t w_fmt, int32_t out_fmt, bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return mx_quant(A, a_scales, W, w_scales, bias, q_codes, q_scales, d, a_fmt, w_fmt, out_fmt, nullptr, p);
}

// bya_gemm_mx_mixed of the packed q|k|v (or q|k) projection with the per-head q/k LayerNorm(64) + RoPE in its epilogue: bit for
// bit bya_gemm_mx_mixed(..., n_split) followed by bya_qknorm_rope, q and k written once.  The kernel is named by an ARGUMENT
// (no option is read): 0 = the tiled kernel of mx_path, as every MX GEMM; 1 = the persistent 256 x 256 kernel
// (gemm256p_mx_kernel<MX_EPI_QKN>, the same bits) where the launch fills it and is eligible, else the tiled one; 2 (tests):
// without the tile count.  Always one launch.
extern "C" int bya_gemm_mx_qkv_norm_rope_on(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                            const void* bias, void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* d,
                                            const bya_qknorm_desc* n, int32_t kernel, hipStream_t stream) {
    return mx_qkn_on(A, a_scales, W, w_scales, bias, C, fmt, w_fmt, d, n, kernel, stream, nullptr);
}

extern "C" int bya_gemm_mx_qkv_norm_rope_on_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                                 const void* bias, const void* C, int32_t fmt, int32_t w_fmt,
                                                 const bya_gemm_desc* d, const bya_qknorm_desc* n, int32_t kernel,
                                                 bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return mx_qkn_on(A, a_scales, W, w_scales, bias, C, fmt, w_fmt, d, n, kernel, nullptr, p);
}

// bya_gemm_mx_qkv_norm_rope_on that also records bya_qknorm_rope's score-bound statistics (include/bya.h), with
// bya_gemm_mx_call's `kernel` argument (so that e2m1 weights and, under BYA_MX_KERNEL_FP6, e2m3 operands reach the persistent
// kernel, whose STATS instances record them); where the launch would take a tiled kernel a table is answered BYA_ERR_UNSUPPORTED
namespace {
int mx_qkn_stats(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, const void* C,
                 int32_t fmt, int32_t w_fmt, const bya_gemm_desc* d, const bya_qknorm_desc* n, int32_t kernel, const QknStats& st,
                 hipStream_t stream, bya_gemm_plan* plan) {
    const bya_mx_gemm_call c = {A, a_scales, W, w_scales, bias, (void*)C, nullptr, nullptr, nullptr, nullptr, n, fmt, w_fmt, MX_E4M3, kernel};
    MxKernel k;
    if (!n || !mx_kernel_of_call(&c, &k)) return BYA_ERR_SHAPE;
    return mx_call(&c, d, k, stream, plan, st);
}
}  // namespace

extern "C" int bya_gemm_mx_qkv_norm_rope_stats(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                               const void* bias, void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* d,
                                               const bya_qknorm_desc* n, int32_t kernel, float* stats, int32_t stats_slots,
                                               hipStream_t stream) {
    return mx_qkn_stats(A, a_scales, W, w_scales, bias, C, fmt, w_fmt, d, n, kernel, QknStats{stats, stats_slots}, stream, nullptr);
}

extern "C" int bya_gemm_mx_qkv_norm_rope_stats_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                                    const void* bias, const void* C, int32_t fmt, int32_t w_fmt,
                                                    const bya_gemm_desc* d, const bya_qknorm_desc* n, int32_t kernel,
                                                    const float* stats, int32_t stats_slots, bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return mx_qkn_stats(A, a_scales, W, w_scales, bias, C, fmt, w_fmt, d, n, kernel, QknStats{const_cast<float*>(stats), stats_slots},
                        nullptr, p);
}

// ... on the tiled kernel (kernel = 0)
extern "C" int bya_gemm_mx_qkv_norm_rope(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                         const void* bias, void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* d,
                                         const bya_qknorm_desc* n, hipStream_t stream) {
    return mx_qkn_on(A, a_scales, W, w_scales, bias, C, fmt, w_fmt, d, n, 0, stream, nullptr);
}

extern "C" int bya_gemm_mx_qkv_norm_rope_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                              const void* bias, const void* C, int32_t fmt, int32_t w_fmt,
                                              const bya_gemm_desc* d, const bya_qknorm_desc* n, bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return mx_qkn_on(A, a_scales, W, w_scales, bias, C, fmt, w_fmt, d, n, 0, nullptr, p);
}
