// fp8 (OCP e4m3) "NT" GEMM on the block-scaled CDNA4 matrix instruction, and the row quantiser that feeds it:
//     C[m,n] = epi( sa[m] * sw[n] * sum_k A8[m,k] * W8[n,k] ),   A8 = fp8(A / sa),  W8 = fp8(W / sw)
// BASELINE configs[4] ("fp8 weights on CDNA4 fp8 MFMA"): the four big Linears of a DiT block
// (attn1.to_q|k|v, attn1.to_out, ff.net.0.proj, ff.net.2 -- models/transformer.py:241-260 via diffusers Attention /
// FeedForward) with per-output-channel weight scales fixed at load time and per-row activation scales taken on the fly.
// The reference has no fp8 path; parity is against the CPU restatement run on the same
// fake-quantised operands (tests/test_fp8_gpu.py).
//
// v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands runs at twice the bf16 rate per clock (MI355X_MICROARCH.md, matrix
// cores): 128 k per instruction, 32 consecutive bytes of one row per lane, both block scales fixed at 2^0 -- the row
// and channel scales are fp32 and are applied to the accumulators in the epilogue.  One K-tile is 128 fp8 = 128-byte LDS
// rows, i.e. exactly the staging / XOR-swizzle image of the bf16 128 x 128 kernel (gemm.hip) at twice the FLOPs per byte.
// Same epilogue as every other GEMM here (bias, activation, gate, residual, q|k|v split): gemm_common.h.
#include "gemm_fp8_kernel.h"
#include "options.h"

bool bya_gemm256p_fp8_eligible(const void* args);                                                       // gemm_fp8_v4.hip
int bya_launch_gemm256p_fp8(const void* args, const float* sa, const float* sw, int batch, int gm, hipStream_t s);
// ... its q/k-norm instance (gemm_fp8_v4_qkn.hip; GemmArgs::qkn_* filled)
int bya_launch_gemm256p_fp8_qkn(const void* args, const float* sa, const float* sw, int batch, int gm, hipStream_t s);
// ... and that one with the score-bound statistics (gemm_fp8_v4_qkn_stats.hip; GemmArgs::qkn_stats* filled as well)
int bya_launch_gemm256p_fp8_qkn_stats(const void* args, const float* sa, const float* sw, int batch, int gm, hipStream_t s);

namespace {

// ---- row quantiser: one workgroup per row.  scale[m] = max|x[m,:]| / 448 (1 for an all-zero row),
// q[m,k] = e4m3( x[m,k] * (448 / max|x[m,:]|) ), round-to-nearest-even (f32_to_e4m3, bya_common.h).
constexpr int QT = 256, QV = 6;                 // threads per row, 8-element vectors per thread: K <= 12288

__global__ __launch_bounds__(QT) void quant_rows_fp8_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ q,
                                                            float* __restrict__ scale, int K, long long ldx, long long ldq) {
    __shared__ float red[QT / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const bf16_t* xr = x + (long long)row * ldx;
    const int nv = K / 8;
    u32x4 v[QV];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < QV; ++i) {
        const int c = tid + i * QT;
        v[i] = c < nv ? *reinterpret_cast<const u32x4*>(xr + c * 8) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int w = 0; w < 4; ++w) amax = fmaxf(amax, fmaxf(fabsf(bflo(v[i][w])), fabsf(bfhi(v[i][w]))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // 448 / amax correctly rounded to fp32 (NOT 448 * (1 / amax): the two differ in the last bit for one row in three, and
    // that moves exact ties such as 8.3125 * (448 / 12.25) = 304 to the other e4m3 neighbour -- 0.13 % of the bytes)
    const float inv = amax > 0.f ? (float)((double)FP8_MAX / (double)amax) : 0.f;
    if (tid == 0) scale[row] = amax > 0.f ? (float)((double)amax / (double)FP8_MAX) : 1.0f;
    uint8_t* qr = q + (long long)row * ldq;
#pragma unroll
    for (int i = 0; i < QV; ++i) {
        const int c = tid + i * QT;
        if (c < nv) {
            u32x2 o;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t w0 = v[i][2 * h], w1 = v[i][2 * h + 1];
                o[h] = f32_to_e4m3(bflo(w0) * inv) | (f32_to_e4m3(bfhi(w0) * inv) << 8) |
                       (f32_to_e4m3(bflo(w1) * inv) << 16) | (f32_to_e4m3(bfhi(w1) * inv) << 24);
            }
            *reinterpret_cast<u32x2*>(qr + c * 8) = o;
        }
    }
}

}  // namespace

extern "C" int bya_quantize_rows_fp8(const void* x, void* q, float* scale, int32_t M, int32_t K, int64_t ldx, int64_t ldq,
                                     hipStream_t stream) {
    if (!x || !q || !scale || M <= 0 || K <= 0) return BYA_ERR_SHAPE;
    if (K % 8 || K > 8 * QT * QV) return BYA_ERR_SHAPE;
    if (ldx < K || ldq < K || ldx % 8 || ldq % 8) return BYA_ERR_ALIGN;
    if (((uintptr_t)x & 15) || ((uintptr_t)q & 7)) return BYA_ERR_ALIGN;
    BYA_LAUNCH(quant_rows_fp8_kernel, dim3(M), dim3(QT), 0, stream, (const bf16_t*)x, (uint8_t*)q, scale, K, (long long)ldx,
               (long long)ldq);
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}

namespace {
// bya_gemm_fp8's arguments -> GemmArgs; BYA_OK or the error that rejects them
int fp8_args(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias, const void* C,
             const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d, GemmArgs* out) {
    if (!A8 || !W8 || !a_scale || !w_scale || !C || !d) return BYA_ERR_SHAPE;
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->batch <= 0) return BYA_ERR_SHAPE;
    if (d->K % BK8 != 0 || d->N % 4 != 0) return BYA_ERR_SHAPE;
    if (d->lda % 16 || d->ldw % 16) return BYA_ERR_ALIGN;
    if (((uintptr_t)A8 | (uintptr_t)W8 | (uintptr_t)w_scale) & 15) return BYA_ERR_ALIGN;
    const int rc = gemm_epilogue_check(C, res, bias, gate0, gate1, d, act_on_big_tiles(d->act));      // none / GELU(tanh): the DiT Linears
    if (rc != BYA_OK) return rc;
    gemm_fill_args(A8, W8, bias, C, res, gate0, gate1, d, out);
    return BYA_OK;
}

// Two 128 x 128 workgroups per CU (4 waves, 64 KiB LDS ring each) cover each other's barrier and LDS-DMA waits; a
// 256 x 256 form (8 waves, 128 KiB ring, one workgroup per CU, half the L2 -> LDS bytes per FLOP) measured 4-16 %
// slower on the four DiT shapes with this simple two-barrier loop, a one-wave-per-SIMD instantiation 8-20 % slower under
// hipcc's schedule (profiles/history/r2_fp8_probe.txt; both removed from the tree in round 3).
// ... until the loop was placed by hand: gemm_fp8_v4.hip (one wave per SIMD, persistent) takes every launch that is big
// enough to fill its 256 x 256 tiles; BYA_FP8_KERNEL=128 (read per call: A/B runs) keeps everything on the kernel above.
// `a`: the whole launch (tile count), `piece`: one row chunk of it (eligibility).
inline int fp8_path(const GemmArgs& a, int batch, const GemmArgs& piece) {
    const long long tiles256 = (long long)((a.M + 255) / 256) * ((a.N + 255) / 256) * batch;
    const bool big = !bya_opt(BYA_OPT_FP8_KERNEL) && tiles256 >= 200;        // (about a round of its 256 workgroups, or more)
    return big && bya_gemm256p_fp8_eligible(&piece) ? BYA_GEMM_PATH_P256 : BYA_GEMM_PATH_T128X128;
}
constexpr int FP8_P256_GROUP_M = 4;        // row-tiles per group of the persistent kernel's tile order

// bya_gemm_fp8 (plan == nullptr) and bya_gemm_fp8_plan: one body, so the query answers what the launch does
int fp8_gemm(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias, const void* C,
             const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d, hipStream_t stream, bya_gemm_plan* plan) {
    GemmArgs a;
    const int rc = fp8_args(A8, a_scale, W8, w_scale, bias, C, res, gate0, gate1, d, &a);
    if (rc != BYA_OK) return rc;
    return gemm_row_chunks(a, d->batch, 1, plan, [&](const GemmArgs& piece, int batch, long long row0) {
        const int path = fp8_path(a, d->batch, piece);
        if (plan) return gemm_plan_whole(plan, path, 1);
        if (path == BYA_GEMM_PATH_P256)
            return bya_launch_gemm256p_fp8(&piece, a_scale + row0, w_scale, batch, FP8_P256_GROUP_M, stream);
        return launch_fp8<128, 128, 2, 2>(piece, a_scale + row0, w_scale, batch, stream);
    });
}
}  // namespace

extern "C" int bya_gemm_fp8(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias,
                            void* C, const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d,
                            hipStream_t stream) {
    return fp8_gemm(A8, a_scale, W8, w_scale, bias, C, res, gate0, gate1, d, stream, nullptr);
}

extern "C" int bya_gemm_fp8_plan(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias,
                                 const void* C, const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* d,
                                 bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return fp8_gemm(A8, a_scale, W8, w_scale, bias, C, res, gate0, gate1, d, nullptr, p);
}

namespace {
// bya_gemm_fp8_qkv_norm_rope's arguments -> GemmArgs; BYA_ERR_UNSUPPORTED: not this epilogue's shape (the caller keeps
// bya_gemm_fp8 + bya_qknorm_rope); malformed arguments: the errors of fp8_args and of the norm descriptor (gemm_common.h)
int fp8_qkn_args(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias, const void* C,
                 const bya_gemm_desc* d, const bya_qknorm_desc* n, const QknStats& st, GemmArgs* out) {
    const int rc0 = qkn_norm_desc_check(d, n);
    if (rc0 != BYA_OK) return rc0;
    const int rcs = qkn_stats_check(st);
    if (rcs != BYA_OK) return rcs;
    const int rc = fp8_args(A8, a_scale, W8, w_scale, bias, C, nullptr, nullptr, nullptr, d, out);
    if (rc != BYA_OK) return rc;
    // there is no residual argument: a descriptor that describes one is not this entry point's launch
    if (d->ldres != 0 || d->res_batch_stride != 0) return BYA_ERR_UNSUPPORTED;
    return qkn_head_args(C, d, n, st, out);
}

// the launch (plan == nullptr) and its plan query: one body, so the query answers what the launch does
int fp8_qkn(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias, const void* C,
            const bya_gemm_desc* d, const bya_qknorm_desc* n, const QknStats& st, hipStream_t stream, bya_gemm_plan* plan) {
    GemmArgs a;
    const int rc = fp8_qkn_args(A8, a_scale, W8, w_scale, bias, C, d, n, st, &a);
    if (rc != BYA_OK) return rc;
    // bya_gemm_fp8's own choice for this descriptor (one row chunk: qkn_head_args): the two kernels differ in last bits, so
    // following it is what keeps fused == two launches in every option state
    const int path = fp8_path(a, d->batch, a);
    // the score-bound statistics (bya_gemm_fp8_qkv_norm_rope_stats) are the persistent kernel's: the tiled one declines them
    if (a.qkn_stats && path != BYA_GEMM_PATH_P256) return BYA_ERR_UNSUPPORTED;
    if (plan) return gemm_plan_whole(plan, path, 1);
    if (path == BYA_GEMM_PATH_P256)
        return a.qkn_stats ? bya_launch_gemm256p_fp8_qkn_stats(&a, a_scale, w_scale, d->batch, FP8_P256_GROUP_M, stream)
                           : bya_launch_gemm256p_fp8_qkn(&a, a_scale, w_scale, d->batch, FP8_P256_GROUP_M, stream);
    return launch_fp8<128, 128, 2, 2, true>(a, a_scale, w_scale, d->batch, stream);
}
}  // namespace

// bya_gemm_fp8 of the packed q|k|v (or q|k) projection with the per-head q/k LayerNorm(64) + RoPE in its epilogue: bit for bit
// bya_gemm_fp8(..., n_split) followed by bya_qknorm_rope on the kernel bya_gemm_fp8 would take, q and k written once.  Always
// one launch.
extern "C" int bya_gemm_fp8_qkv_norm_rope(const void* A8, const float* a_scale, const void* W8, const float* w_scale,
                                          const void* bias, void* C, const bya_gemm_desc* d, const bya_qknorm_desc* n,
                                          hipStream_t stream) {
    return fp8_qkn(A8, a_scale, W8, w_scale, bias, C, d, n, QknStats{}, stream, nullptr);
}

extern "C" int bya_gemm_fp8_qkv_norm_rope_plan(const void* A8, const float* a_scale, const void* W8, const float* w_scale,
                                               const void* bias, const void* C, const bya_gemm_desc* d,
                                               const bya_qknorm_desc* n, bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return fp8_qkn(A8, a_scale, W8, w_scale, bias, C, d, n, QknStats{}, nullptr, p);
}

// ... that also records bya_qknorm_rope's score-bound statistics (include/bya.h): on path P256 (gemm256p_fp8_qkn_stats_kernel);
// where the launch would take the tiled kernel a table is answered BYA_ERR_UNSUPPORTED
extern "C" int bya_gemm_fp8_qkv_norm_rope_stats(const void* A8, const float* a_scale, const void* W8, const float* w_scale,
                                                const void* bias, void* C, const bya_gemm_desc* d, const bya_qknorm_desc* n,
                                                float* stats, int32_t stats_slots, hipStream_t stream) {
    return fp8_qkn(A8, a_scale, W8, w_scale, bias, C, d, n, QknStats{stats, stats_slots}, stream, nullptr);
}

extern "C" int bya_gemm_fp8_qkv_norm_rope_stats_plan(const void* A8, const float* a_scale, const void* W8, const float* w_scale,
                                                     const void* bias, const void* C, const bya_gemm_desc* d,
                                                     const bya_qknorm_desc* n, const float* stats, int32_t stats_slots,
                                                     bya_gemm_plan* p) {
    if (!p) return BYA_ERR_SHAPE;
    return fp8_qkn(A8, a_scale, W8, w_scale, bias, C, d, n, QknStats{const_cast<float*>(stats), stats_slots}, nullptr, p);
}
