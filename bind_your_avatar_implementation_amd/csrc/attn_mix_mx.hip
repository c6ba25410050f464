// The MX-output instances of the <= 32-key kv-mix (bya_attn_kv_mix_mx, bya_attn_kv_mix_mx_seg, bya_attn_kv_mix_mx_batch; the body
// and its second epilogue: attn_mix32.h).  A translation unit of their own because it is built without the SLP vectoriser (build.py, NO_SLP_SOURCES): the
// quantiser arithmetic stays free of packed-fp32 VALU instructions, like the standalone and the LayerNorm-fused quantisers.  The
// arithmetic per element is that of the bf16 instances in attn.hip (the vectoriser pairs operations, it does not reorder or
// contract them), which tests/test_mx_cross_out_gpu.py checks byte for byte.
#include "attn_mix32.h"

namespace {

// the MX-output instances (bya_attn_kv_mix_mx); resource numbers: DESIGN.md section 11
__global__ __launch_bounds__(256, 2) void attn_kv_mix32_mx_kernel_d64(MixMxArgs pm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<64, true>(pm.a, smem, &pm.mx);
}
__global__ __launch_bounds__(256) void attn_kv_mix32_mx_kernel_d128(MixMxArgs pm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<128, true>(pm.a, smem, &pm.mx);
}
// ... and the one that takes its rows from a segment table (bya_attn_kv_mix_mx_seg: head_dim 64 alone, the audio path's)
__global__ __launch_bounds__(256, 2) void attn_kv_mix32_mx_seg_kernel_d64(MixMxSegArgs pm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<64, true, true>(pm.a, smem, &pm.mx, &pm.seg);
}
// ... and the ones whose blockIdx.y is the sample of a batch (bya_attn_kv_mix_mx_batch): the same body on that sample's pointers
__global__ __launch_bounds__(256, 2) void attn_kv_mix32_mx_batch_kernel_d64(MixMxBatchArgs pm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const MixArgs a = mix_sample_args(pm.a, pm.s);
    const ByaMixMxOut mx = mix_sample_out(pm.mx, pm.s);
    attn_mix32_body<64, true>(a, smem, &mx);
}
__global__ __launch_bounds__(256) void attn_kv_mix32_mx_batch_kernel_d128(MixMxBatchArgs pm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const MixArgs a = mix_sample_args(pm.a, pm.s);
    const ByaMixMxOut mx = mix_sample_out(pm.mx, pm.s);
    attn_mix32_body<128, true>(a, smem, &mx);
}

}  // namespace

int bya_launch_attn_kv_mix32_mx(const void* q, const void* k, const void* v, const void* r, const void* af, float* wsum,
                                const bya_attn_mix_desc& desc, const bya_attn_kv_mix_plan_info& plan, const ByaMixMxOut& out,
                                const bya_attn_mix_segments* seg, const ByaMixSampleStrides* batch, hipStream_t stream) {
    MixMxArgs m;
    mix_args_of(q, k, v, r, af, wsum, &desc, plan.row_chunks, m.a);
    m.mx = out;
    const dim3 grid((unsigned)plan.grid);
    const size_t lds = (size_t)plan.lds_bytes;
    if (seg) {                                      // (head_dim 64: 4 identities make 48 KiB with the patches, never big_lds)
        const MixMxSegArgs ms{m.a, m.mx, *seg};
        BYA_LAUNCH(attn_kv_mix32_mx_seg_kernel_d64, grid, dim3(256), lds, stream, ms);
        return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
    }
    if (batch) {                                    // one sample's grid in x, the samples in y
        const MixMxBatchArgs mb{m.a, m.mx, *batch};
        const dim3 bgrid((unsigned)plan.grid, (unsigned)batch->n);
        if (plan.big_lds) {
            static std::atomic<unsigned long long> bbig64{0}, bbig128{0};
            const int rc = desc.head_dim == 64
                ? bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_mx_batch_kernel_d64), 160 * 1024, bbig64)
                : bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_mx_batch_kernel_d128), 160 * 1024, bbig128);
            if (rc != BYA_OK) return rc;
        }
        if (desc.head_dim == 64) BYA_LAUNCH(attn_kv_mix32_mx_batch_kernel_d64, bgrid, dim3(256), lds, stream, mb);
        else BYA_LAUNCH(attn_kv_mix32_mx_batch_kernel_d128, bgrid, dim3(256), lds, stream, mb);
        return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
    }
    if (plan.big_lds) {
        static std::atomic<unsigned long long> big64{0}, big128{0};
        const int rc = desc.head_dim == 64
            ? bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_mx_kernel_d64), 160 * 1024, big64)
            : bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_mx_kernel_d128), 160 * 1024, big128);
        if (rc != BYA_OK) return rc;
    }
    if (desc.head_dim == 64) BYA_LAUNCH(attn_kv_mix32_mx_kernel_d64, grid, dim3(256), lds, stream, m);
    else BYA_LAUNCH(attn_kv_mix32_mx_kernel_d128, grid, dim3(256), lds, stream, m);
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}
