// OCP MX block quantisation (include/bya.h, "MX weights"), shared by the standalone quantiser (gemm_mx.hip) and the
// LayerNorm-fused one (norm.hip).  One lane holds 8 consecutive values of a row; the 4 lanes (lane & 3 = 0..3) of an aligned
// quad hold one 32-element block.  Plain VALU arithmetic: the definition is RNE + saturation of x * 2^-E, and an exact
// power-of-two product followed by one rint is exactly that.
#pragma once
#include "bya_common.h"

// gemm_mx_v4.hip, called by gemm_mx.hip: the persistent one-wave-per-SIMD 256 x 256 kernel for e4m3 or e2m3 activations x
// weights in the same format or in e2m1 (args: GemmArgs).  quant: eligibility under the quantising epilogue; epi: MX_EPI_BF16,
// MX_EPI_QKN, or MX_E4M3 / MX_E2M3 = quantising to that format (qs: its scale bytes); a_fmt: MX_E4M3 or MX_E2M3; w_fmt: a_fmt
// or MX_E2M1
bool bya_gemm256p_mx_eligible(const void* args, bool quant);
int bya_launch_gemm256p_mx(const void* args, const uint8_t* sa, const uint8_t* sw, uint8_t* qs, int epi, int a_fmt, int w_fmt,
                           int batch, int gm, hipStream_t s);

namespace {

constexpr int MX_E4M3 = 0, MX_E2M3 = 2, MX_E2M1 = 4;                      // the instruction's cbsz / blgp codes
// the epilogue of an MX GEMM kernel (its QOUT parameter): the element format of the quantising one, or
constexpr int MX_EPI_BF16 = -1, MX_EPI_QKN = -2;                          // bf16 out; bf16 out with q/k-norm + RoPE (GemmArgs::qkn_*)
constexpr int MX_EPI_QKN_STATS = -3;      // the persistent kernel's alone: MX_EPI_QKN that records the score-bound statistics (qkn_stats)
__host__ __device__ constexpr int mx_emax(int fmt) { return fmt == MX_E4M3 ? 8 : 2; }                  // (e2m3 and e2m1: 2)
__host__ __device__ constexpr int mx_block_bytes(int fmt) { return fmt == MX_E4M3 ? 32 : fmt == MX_E2M3 ? 24 : 16; }

// |v| <= 7.5 after the clamp; e2m3 code = (exponent << 3) | mantissa with exponent bias 1.  In each binade the code is
// an affine function of v / step (step 1/8 below 2, 1/4 in [2, 4), 1/2 in [4, 8)), and rint (v_rndne_f32) is RNE on
// that count; a count that rounds up into the next binade lands on its first code, so ties go to the even code.
__device__ __forceinline__ uint32_t f32_to_e2m3(float v) {
    const uint32_t sign = (__float_as_uint(v) >> 26) & 0x20u;
    const float a = fminf(fabsf(v), 7.5f);
    uint32_t c;
    if (a < 2.0f) c = (uint32_t)__builtin_rintf(a * 8.0f);
    else if (a < 4.0f) c = (uint32_t)__builtin_rintf(a * 4.0f) + 8u;
    else c = (uint32_t)__builtin_rintf(a * 2.0f) + 16u;
    return sign | c;
}

// |v| <= 6 after the clamp; e2m1 code = (exponent << 1) | mantissa with exponent bias 1 (magnitudes 0, 0.5, 1, 1.5, 2, 3, 4,
// 6).  The same count of steps as f32_to_e2m3: step 1/2 below 2, 1 in [2, 4), 2 from 4.
__device__ __forceinline__ uint32_t f32_to_e2m1(float v) {
    const uint32_t sign = (__float_as_uint(v) >> 28) & 0x8u;
    const float a = fminf(fabsf(v), 6.0f);
    uint32_t c;
    if (a < 2.0f) c = (uint32_t)__builtin_rintf(a * 2.0f);
    else if (a < 4.0f) c = (uint32_t)__builtin_rintf(a) + 2u;
    else c = (uint32_t)__builtin_rintf(a * 0.5f) + 4u;
    return sign | c;
}

// The codes of 8 values of a 32-block whose |max| is `amax`, in registers: element i at bits 8i.. (fp8: 64 bits), 6i.. (fp6:
// 48 bits) or 4i.. (fp4: 32 bits) of the result; the block's scale byte in `sbyte`.  THE arithmetic of the format: the
// standalone and the LayerNorm-fused quantiser store these bits as they are (mx_quant8), the GEMM's quantising epilogue
// (gemm_mx.hip) stores their two halves, which sit 16 elements apart in its accumulator layout.
template <int FMT>
__device__ __forceinline__ uint64_t mx_quant8_bits(const float* v, float amax, uint32_t& sbyte) {
    sbyte = 127u;
    float inv = 0.0f;
    if (amax > 0.0f) {
        int e = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127 - mx_emax(FMT);    // subnormal amax: far below -127
        e = e < -127 ? -127 : (e > 127 ? 127 : e);
        sbyte = (uint32_t)(e + 127);
        inv = __uint_as_float((uint32_t)(127 - e) << 23);                               // 2^-E, E in [-127, 126]: normal
    }
    if constexpr (FMT == MX_E4M3) {
        uint32_t w[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
            w[h] = f32_to_e4m3(v[4 * h] * inv) | (f32_to_e4m3(v[4 * h + 1] * inv) << 8) |
                   (f32_to_e4m3(v[4 * h + 2] * inv) << 16) | (f32_to_e4m3(v[4 * h + 3] * inv) << 24);
        if (amax == 0.0f) w[0] = w[1] = 0u;                                            // -0 inputs: all-zero codes
        return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    } else if constexpr (FMT == MX_E2M1) {
        uint32_t bits = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) bits |= f32_to_e2m1(v[i] * inv) << (4 * i);
        if (amax == 0.0f) bits = 0;
        return bits;
    } else {
        uint64_t bits = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) bits |= (uint64_t)f32_to_e2m3(v[i] * inv) << (6 * i);
        if (amax == 0.0f) bits = 0;
        return bits;
    }
}

// Quantise the 8 values of this lane's share of a 32-block whose |max| over the quad is `amax`.  Writes the lane's codes
// (fp8: 8 bytes; fp6: 6 bytes = element i at bits 6i.., i = 0..7, since the lane's first element sits at bit 48 * (lane & 3)
// of the block; fp4: one dword, element i at bits 4i..) through `dst` = start of the lane's bytes, and returns the scale byte.
template <int FMT>
__device__ __forceinline__ uint32_t mx_quant8(const float* v, float amax, uint8_t* dst) {
    uint32_t sbyte;
    const uint64_t bits = mx_quant8_bits<FMT>(v, amax, sbyte);
    if constexpr (FMT == MX_E4M3) {
        u32x2 o; o[0] = (uint32_t)bits; o[1] = (uint32_t)(bits >> 32);
        *reinterpret_cast<u32x2*>(dst) = o;
    } else if constexpr (FMT == MX_E2M1) {
        *reinterpret_cast<uint32_t*>(dst) = (uint32_t)bits;
    } else {
        uint16_t* d16 = reinterpret_cast<uint16_t*>(dst);                               // 6 bytes at a 2-byte boundary
        d16[0] = (uint16_t)bits; d16[1] = (uint16_t)(bits >> 16); d16[2] = (uint16_t)(bits >> 32);
    }
    return sbyte;
}

// max |v| over the aligned lane quad (all four lanes must be active)
__device__ __forceinline__ float quad_amax(float a) {
    a = fmaxf(a, __shfl_xor(a, 1, 64));
    return fmaxf(a, __shfl_xor(a, 2, 64));
}

}  // namespace
