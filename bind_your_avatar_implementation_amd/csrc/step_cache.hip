// First-block step cache (include/bya.h, "First-block step cache"): the three streaming passes over the
// resident joint stream x [B, S, D] bf16 -- probe, capture, apply -- and the probe's one-workgroup finish.  HBM-bound: 16-byte
// loads and stores, eight bf16 per lane, a grid-stride walk whose grid depends on n alone.  No atomics: the probe's two sums
// go through per-workgroup fp64 partials in fixed slots, so the same inputs give the same 16 bytes on every run.
#include "bya_common.h"
#include "../../include/bya.h"

namespace {

constexpr int WG = 256;                 // lanes of a workgroup
constexpr int VEC = 8;                  // bf16 per lane and pass (one 16-byte vector)
constexpr int MAX_GRID = 2048;          // 256 CUs x 8 workgroups; the finish launch adds at most this many partials

// bf16_rne of the definition: round to nearest even, and every NaN becomes the one quiet NaN 0x7fc0 (converters disagree on a
// NaN's bits), so that a written tensor is a function of the VALUES it was computed from, bit for bit
__device__ __forceinline__ uint32_t bf16_rne(float f) { return f != f ? 0x7fc0u : (uint32_t)f2bf(f); }
__device__ __forceinline__ u32x4 pack8_rne(const float* f) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = bf16_rne(f[2 * i]) | (bf16_rne(f[2 * i + 1]) << 16);
    return v;
}

inline int ok() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? BYA_OK : -(1000 + (int)e); }

// the lanes of a wave in a fixed butterfly (the order depends on nothing but the lane ids)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// r_new = bf16(x - E); E = x; partials[2 wg] += sum |r_new - r_ref|, partials[2 wg + 1] += sum |r_ref| (terms fp32, sums fp64).
// A lane adds its own terms in pass order, element order inside a pass; then the wave's butterfly; then wave 0..3 in order.
template <bool HAS_REF>
__global__ __launch_bounds__(WG) void step_cache_probe_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ E,
                                                              const bf16_t* __restrict__ r_ref, bf16_t* __restrict__ r_new,
                                                              double* __restrict__ partials, long long nvec) {
    double num = 0.0, den = 0.0;
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < nvec; i += (long long)gridDim.x * WG) {
        const u32x4 xr = *reinterpret_cast<const u32x4*>(x + i * VEC);
        float xv[8], ev[8], rv[8];
        unpack8(xr, xv);
        unpack8(*reinterpret_cast<const u32x4*>(E + i * VEC), ev);
#pragma unroll
        for (int e = 0; e < 8; ++e) ev[e] = xv[e] - ev[e];
        const u32x4 rn = pack8_rne(ev);
        *reinterpret_cast<u32x4*>(r_new + i * VEC) = rn;
        *reinterpret_cast<u32x4*>(E + i * VEC) = xr;
        if (HAS_REF) {
            unpack8(rn, ev);                         // r_new enters the sums as stored: rounded
            unpack8(*reinterpret_cast<const u32x4*>(r_ref + i * VEC), rv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                num += (double)fabsf(ev[e] - rv[e]);
                den += (double)fabsf(rv[e]);
            }
        }
    }
    __shared__ double part[2][WG / 64];
    num = wave_sum_f64(num);
    den = wave_sum_f64(den);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = num;
        part[1][threadIdx.x >> 6] = den;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = part[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < WG / 64; ++w) s += part[threadIdx.x][w];
        partials[2 * (long long)blockIdx.x + threadIdx.x] = s;
    }
}

// sums[0] = partials[0] + partials[2] + ..., sums[1] = partials[1] + partials[3] + ...: each by ONE lane, in index order
// (lane 0 of wave 0 and lane 0 of wave 1), out of LDS the whole workgroup filled.
__global__ __launch_bounds__(WG) void step_cache_finish_kernel(const double* __restrict__ partials, double* __restrict__ sums,
                                                               int grid) {
    __shared__ double slots[2 * MAX_GRID];
    for (int i = threadIdx.x; i < 2 * grid; i += WG) slots[i] = partials[i];
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {
        const int which = threadIdx.x >> 6;
        double s = 0.0;
        for (int g = 0; g < grid; ++g) s += slots[2 * g + which];
        sums[which] = s;
    }
}

// R = bf16(x - E)
__global__ __launch_bounds__(WG) void step_cache_capture_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ E,
                                                                bf16_t* __restrict__ R, long long nvec) {
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < nvec; i += (long long)gridDim.x * WG) {
        float xv[8], ev[8];
        unpack8(*reinterpret_cast<const u32x4*>(x + i * VEC), xv);
        unpack8(*reinterpret_cast<const u32x4*>(E + i * VEC), ev);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] -= ev[e];
        *reinterpret_cast<u32x4*>(R + i * VEC) = pack8_rne(xv);
    }
}

// x = bf16(x + R), in place
__global__ __launch_bounds__(WG) void step_cache_apply_kernel(bf16_t* __restrict__ x, const bf16_t* __restrict__ R, long long nvec) {
    for (long long i = (long long)blockIdx.x * WG + threadIdx.x; i < nvec; i += (long long)gridDim.x * WG) {
        float xv[8], rv[8];
        unpack8(*reinterpret_cast<const u32x4*>(x + i * VEC), xv);
        unpack8(*reinterpret_cast<const u32x4*>(R + i * VEC), rv);
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] += rv[e];
        *reinterpret_cast<u32x4*>(x + i * VEC) = pack8_rne(xv);
    }
}

// the one grid of the three passes: a function of n alone
int plan_of(int64_t n, bya_step_cache_plan_info* p) {
    if (n <= 0 || n % VEC) return BYA_ERR_SHAPE;
    const long long nvec = n / VEC;
    long long grid = (nvec + WG - 1) / WG;
    if (grid > MAX_GRID) grid = MAX_GRID;
    p->grid = (int32_t)grid;
    p->vec = VEC;
    p->wg_pass_elems = WG * VEC;
    p->passes = (int32_t)((nvec + grid * WG - 1) / (grid * WG));
    p->partials_bytes = 2 * (int64_t)sizeof(double) * grid;
    return BYA_OK;
}

inline bool misaligned(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) != 0;
}

int probe_plan_of(const void* x, const void* E, const void* r_ref, const void* r_new, int64_t n, bya_step_cache_plan_info* p) {
    if (!x || !E || !r_new) return BYA_ERR_SHAPE;
    bya_step_cache_plan_info q;
    const int rc = plan_of(n, &q);
    if (rc != BYA_OK) return rc;
    if (misaligned(x, E, r_ref, r_new)) return BYA_ERR_ALIGN;
    *p = q;
    return BYA_OK;
}

}  // namespace

extern "C" int bya_step_cache_probe_plan(const void* x, const void* E, const void* r_ref, const void* r_new, int64_t n,
                                         bya_step_cache_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    return probe_plan_of(x, E, r_ref, r_new, n, plan);
}

extern "C" int bya_step_cache_probe(const void* x, void* E, const void* r_ref, void* r_new, double* partials, double* sums,
                                    int64_t n, hipStream_t stream) {
    if (!partials || !sums) return BYA_ERR_SHAPE;
    bya_step_cache_plan_info pl;
    const int rc = probe_plan_of(x, E, r_ref, r_new, n, &pl);
    if (rc != BYA_OK) return rc;
    if (((uintptr_t)partials | (uintptr_t)sums) & 7) return BYA_ERR_ALIGN;
    const long long nvec = n / VEC;
    if (r_ref)
        BYA_LAUNCH(step_cache_probe_kernel<true>, dim3((unsigned)pl.grid), dim3(WG), 0, stream, (const bf16_t*)x, (bf16_t*)E,
                   (const bf16_t*)r_ref, (bf16_t*)r_new, partials, nvec);
    else
        BYA_LAUNCH(step_cache_probe_kernel<false>, dim3((unsigned)pl.grid), dim3(WG), 0, stream, (const bf16_t*)x, (bf16_t*)E,
                   (const bf16_t*)nullptr, (bf16_t*)r_new, partials, nvec);
    const int first = ok();
    if (first != BYA_OK) return first;
    BYA_LAUNCH(step_cache_finish_kernel, dim3(1), dim3(WG), 0, stream, (const double*)partials, sums, (int)pl.grid);
    return ok();
}

extern "C" int bya_step_cache_capture(const void* x, const void* E, void* R, int64_t n, hipStream_t stream) {
    if (!x || !E || !R) return BYA_ERR_SHAPE;
    bya_step_cache_plan_info pl;
    const int rc = plan_of(n, &pl);
    if (rc != BYA_OK) return rc;
    if (misaligned(x, E, R, nullptr)) return BYA_ERR_ALIGN;
    BYA_LAUNCH(step_cache_capture_kernel, dim3((unsigned)pl.grid), dim3(WG), 0, stream, (const bf16_t*)x, (const bf16_t*)E,
               (bf16_t*)R, (long long)(n / VEC));
    return ok();
}

extern "C" int bya_step_cache_apply(void* x, const void* R, int64_t n, hipStream_t stream) {
    if (!x || !R) return BYA_ERR_SHAPE;
    bya_step_cache_plan_info pl;
    const int rc = plan_of(n, &pl);
    if (rc != BYA_OK) return rc;
    if (misaligned(x, R, nullptr, nullptr)) return BYA_ERR_ALIGN;
    BYA_LAUNCH(step_cache_apply_kernel, dim3((unsigned)pl.grid), dim3(WG), 0, stream, (bf16_t*)x, (const bf16_t*)R,
               (long long)(n / VEC));
    return ok();
}
