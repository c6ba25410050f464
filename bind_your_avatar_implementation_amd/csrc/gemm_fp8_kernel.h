// Kernel template of the e4m3 GEMM (see gemm_fp8.hip for the description; two waves per SIMD, MFMA results in arch VGPRs).
#pragma once
#include "gemm_common.h"
#include "gemm_tile_qkn_epilogue.h"
#include <stdlib.h>

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int BK8 = 128;          // fp8 elements (= bytes) per K-tile
constexpr int FP8_GROUP_M = 8;    // row-tiles per group of the tile order (2 / 4 / 8 measured level: tools/fp8_gemm_zeros_probe.py)
constexpr float FP8_MAX = 448.0f; // largest finite e4m3fn

template <int ROWS, int NWAVES>
__device__ __forceinline__ void stage_tile8(const uint8_t* __restrict__ src, int ld, int row0, int row_max, int k0,
                                            char* lds_tile, int wave, int lane) {
    // ROWS x 128 bytes, 8 rows (1 KiB) per wave-instruction; 16-byte chunk c of row r lands at chunk c ^ ((r >> 1) & 7)
    constexpr int PER_WAVE = ROWS / NWAVES;
#pragma unroll
    for (int q = 0; q < PER_WAVE / 8; ++q) {
        const int rbase = wave * PER_WAVE + q * 8;
        const int rl = rbase + (lane >> 3);
        const int chunk = (lane & 7) ^ ((rl >> 1) & 7);
        int gr = row0 + rl;
        gr = gr < row_max ? gr : row_max;
        const uint8_t* g = src + (long long)gr * ld + k0 + chunk * 16;
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(g), LDS_PTR(lds_tile + rbase * 128), 16, 0, 0);
    }
}

// the 32 bytes k = 32 g .. 32 g + 31 of one row (A and W use the same lane -> k map, so the products pair up)
__device__ __forceinline__ i32x8 lds_frag8(const char* tile, int row, int g) {
    const int sw = (row >> 1) & 7;
    const i32x4 lo = *reinterpret_cast<const i32x4*>(tile + row * 128 + (((2 * g) ^ sw) << 4));
    const i32x4 hi = *reinterpret_cast<const i32x4*>(tile + row * 128 + (((2 * g + 1) ^ sw) << 4));
    return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_fp8_kernel(GemmArgs p, const float* __restrict__ sa,
                                                                          const float* __restrict__ sw, int GM) {
#define GEMM_FP8_BODY_QKN 0
#include "gemm_fp8_kernel_body.h"
#undef GEMM_FP8_BODY_QKN
}

// ... with the q/k-norm epilogue (GemmArgs::qkn_*)
template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N) void gemm_fp8_qkn_kernel(GemmArgs p, const float* __restrict__ sa,
                                                                              const float* __restrict__ sw, int GM) {
#define GEMM_FP8_BODY_QKN 1
#include "gemm_fp8_kernel_body.h"
#undef GEMM_FP8_BODY_QKN
}

// QKN: the instance with the q/k-norm epilogue (the caller has filled GemmArgs::qkn_*)
template <int BM, int BN, int WAVES_M, int WAVES_N, bool QKN = false>
int launch_fp8(const GemmArgs& a, const float* sa, const float* sw, int batch, hipStream_t s) {
    const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
    dim3 grid(tiles_m * tiles_n, 1, batch);
    const size_t lds = 2 * (BM + BN) * BK8;
    static std::atomic<unsigned long long> attr_done{0};
    auto go = [&](auto kern) {
        if (bya_allow_big_lds(reinterpret_cast<const void*>(kern), (int)lds, attr_done) != BYA_OK) return (int)BYA_ERR_LAUNCH;
        const int gm = FP8_GROUP_M;
        BYA_LAUNCH(kern, grid, dim3(64 * WAVES_M * WAVES_N), lds, s, a, sa, sw, gm);
        return hipGetLastError() == hipSuccess ? (int)BYA_OK : (int)BYA_ERR_LAUNCH;
    };
    if constexpr (QKN) return go(gemm_fp8_qkn_kernel<BM, BN, WAVES_M, WAVES_N>);
    else return go(gemm_fp8_kernel<BM, BN, WAVES_M, WAVES_N>);
}

}  // namespace

