// The bf16 instances of the <= 32-key kv-mix whose blockIdx.y is the sample of a batch (bya_attn_kv_mix_batch; the body:
// attn_mix32.h, on the sample's pointers: mix_sample_args; the checks and the plan: attn.hip, next to bya_attn_kv_mix's).  One
// launch for the [uncond, cond] pair of a guided step, where bya_attn_kv_mix needs one launch per sample.  A translation unit of
// its own, like attn_mix_seg.hip, so that attn.hip's count of packed-fp32 instructions, which tests/test_abi_cpu.py watches, stays
// where it was; it is compiled with attn.hip's flags, so the body is the same code under the same compiler settings as the
// single-sample instances (tests/test_batch_launch_gpu.py: byte for byte).  The MX-output twins sit with the other MX instances
// in attn_mix_mx.hip.
#include "attn_mix32.h"

namespace {

__global__ __launch_bounds__(256, 2) void attn_kv_mix32_batch_kernel_d64(MixBatchArgs pb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<64>(mix_sample_args(pb.a, pb.s), smem);
}
__global__ __launch_bounds__(256) void attn_kv_mix32_batch_kernel_d128(MixBatchArgs pb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<128>(mix_sample_args(pb.a, pb.s), smem);
}

}  // namespace

int bya_launch_attn_kv_mix32_batch(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                                   const bya_attn_mix_desc& desc, const bya_attn_kv_mix_plan_info& plan,
                                   const ByaMixSampleStrides& batch, hipStream_t stream) {
    MixBatchArgs b;
    mix_args_of(q, k, v, r, af, wsum, &desc, plan.row_chunks, b.a);
    b.a.z = (bf16_t*)z; b.a.z_grp = desc.z_grp; b.a.z_row = desc.z_row;
    b.s = batch;
    const dim3 grid((unsigned)plan.grid, (unsigned)batch.n);     // one sample's grid in x, the samples in y
    const size_t lds = (size_t)plan.lds_bytes;
    if (plan.big_lds) {
        static std::atomic<unsigned long long> big64{0}, big128{0};
        const int rc = desc.head_dim == 64
            ? bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_batch_kernel_d64), 160 * 1024, big64)
            : bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_batch_kernel_d128), 160 * 1024, big128);
        if (rc != BYA_OK) return rc;
    }
    if (desc.head_dim == 64) BYA_LAUNCH(attn_kv_mix32_batch_kernel_d64, grid, dim3(256), lds, stream, b);
    else BYA_LAUNCH(attn_kv_mix32_batch_kernel_d128, grid, dim3(256), lds, stream, b);
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}
