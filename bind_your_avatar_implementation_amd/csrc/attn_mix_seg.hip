// The bf16 instance of the <= 32-key kv-mix that takes its rows from a segment table (bya_attn_kv_mix_seg; the body: attn_mix32.h,
// SEG = true; the checks and the plan: attn.hip, next to bya_attn_kv_mix's).  One launch for the partial frames a
// sequence-parallel rank holds, where bya_attn_kv_mix needs one launch per partial frame.  A translation unit of its own so
// that attn.hip's count of packed-fp32 instructions, which tests/test_abi_cpu.py watches, stays where it was.  The MX-output
// twin sits with the other MX instances in attn_mix_mx.hip.
#include "attn_mix32.h"

namespace {

// (head_dim 64 alone: the audio cross-attention is the only caller; resource numbers: DESIGN.md section 11)
__global__ __launch_bounds__(256, 2) void attn_kv_mix32_seg_kernel_d64(MixSegArgs ps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<64, false, true>(ps.a, smem, nullptr, &ps.seg);
}

}  // namespace

int bya_launch_attn_kv_mix32_seg(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                                 const bya_attn_mix_desc& desc, const bya_attn_kv_mix_plan_info& plan,
                                 const bya_attn_mix_segments& seg, hipStream_t stream) {
    MixSegArgs s;
    mix_args_of(q, k, v, r, af, wsum, &desc, plan.row_chunks, s.a);
    s.a.z = (bf16_t*)z; s.a.z_row = desc.z_row;
    s.seg = seg;
    BYA_LAUNCH(attn_kv_mix32_seg_kernel_d64, dim3((unsigned)plan.grid), dim3(256), (size_t)plan.lds_bytes, stream, s);
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}
