// Shared by the attention translation units (attn.hip: compiler-scheduled kernels, MFMA results in arch VGPRs;
// attn_w4.hip: the hand-placed one-wave-per-SIMD joint-attention kernel, accumulators in AGPRs).
#pragma once
#include "bya_common.h"
#include "mx_common.h"
#include "../../include/bya.h"

namespace {

struct AttnArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
    int heads, nb1, nb2, Sq, Skv, nqt;
    long long q_s1, q_s2, q_row, k_s1, k_s2, k_row, v_s1, v_s2, v_row, o_s1, o_s2, o_row;
    float scale_log2;  // scale * log2(e)
    int prescaled;     // scores already in exp2 units (scale folded into k by the producer)
    float score_bound; // > 0: |score| <= bound guaranteed by the caller -> static-offset softmax (no running maximum)
    float* sk_part;    // stream-K exchange slots / flags of the joint-attention kernel (attn_w4.hip; set by its launcher)
    unsigned* sk_flags;
    int o_wide;        // o and its strides are 16-byte aligned: the epilogue stores 16 bytes per lane (store_o_tile)
    // data-dependent score bound (bya_attn_desc.bound_dev; attn_w4.hip): squared norms [slots][2][bound_heads], this launch's
    // bh at column bound_bh0 + bh; heads whose bound exceeds bound_limit are left to the running-maximum kernel, which
    // runs with only_flagged = fallback and skips every other head
    const float* bound_dev; int bound_slots, bound_heads, bound_bh0; float bound_limit;
    int* fallback;
    const int* only_flagged;
};

// The MX-output instances (bya_attn_fwd_mx) take AttnArgs with o / o_s1 / o_s2 / o_row addressing the CODES, in bytes, plus
// where the e8m0 scale bytes go (strides in bytes as well).  The bf16 instances' kernel argument stays AttnArgs alone.
struct AttnMxOut { uint8_t* scales; long long s1, s2, row; int fmt; };   // fmt: MX_E4M3 / MX_E2M3
struct AttnMxArgs { AttnArgs a; AttnMxOut mx; };

constexpr int KV_TILE = 64;

// XOR applied to the 16-byte chunk index of LDS row `row` (both on the staging source and on the reads):
//  K (ds_read_b128, 32 rows x one chunk per half-wave): 128-B rows -> (row>>1)&7, 256-B rows -> row&15
//  V (ds_read_b64_tr_b16, 4 rows x 64 B per half-wave):  128-B rows -> ((row>>1)&1)<<2, 256-B rows -> (row&3)<<2
// One 32-column tile of an output row block, O^T accumulator layout: lane (r, hf) holds row r's columns 8 gq + 4 hf ..+3
// in acc[4 gq ..+3].  As it stands that is four 8-byte stores per lane, each instruction touching 32 rows with 16 bytes.
// wide: the half-waves trade pieces first (v_permlane32_swap: lanes 32-63 of the first operand <-> lanes 0-31 of the
// second), after which a lower lane holds columns 16 k ..+7 and its partner 16 k + 8 ..+7 -- two 16-byte stores per
// lane, 32 contiguous bytes per row and instruction: half the store instructions and requests, same bytes.  The short
// attention launches (router: 21 key tiles per workgroup) are store-issue-bound in their tail.
__device__ __forceinline__ void store_o_tile(bf16_t* orow_d, const f32x16& acc, float inv, int hf, bool valid, bool wide) {
    uint32_t w[4][2];
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        w[gq][0] = pack2bf(acc[gq * 4 + 0] * inv, acc[gq * 4 + 1] * inv);
        w[gq][1] = pack2bf(acc[gq * 4 + 2] * inv, acc[gq * 4 + 3] * inv);
    }
    if (wide) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const auto s0 = __builtin_amdgcn_permlane32_swap(w[2 * k][0], w[2 * k + 1][0], false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(w[2 * k][1], w[2 * k + 1][1], false, false);
            u32x4 o;
            o[0] = s0[0]; o[1] = s1[0]; o[2] = s0[1]; o[3] = s1[1];
            if (valid) *reinterpret_cast<u32x4*>(orow_d + 16 * k + 8 * hf) = o;
        }
    } else if (valid) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            u32x2 o;
            o[0] = w[gq][0]; o[1] = w[gq][1];
            *reinterpret_cast<u32x2*>(orow_d + gq * 8 + hf * 4) = o;
        }
    }
}

// The MX epilogue of one head_dim-64 head: both 32-column tiles of a row leave as one MX block each -- the codes and the scale
// byte bya_quantize_mx would write for the bf16 row store_o_tile stores.  v = bf16(acc * inv) is that stored value; the block
// |max| is the maximum over the lane's 16 values and its partner's (one v_permlane32_swap); mx_quant8_bits gives the codes of
// the lane's four 4-column pieces (gq = 0..3: columns 8 gq + 4 hf ..+3; 32 bits each as e4m3, 24 as e2m3).  Two more swaps trade
// pieces so that lane hf holds columns 16 hf ..+15 of the block: the lower lane keeps its gq 0, 1 and gets the partner's, the
// upper lane keeps its gq 2, 3.  Each lane then stores 16 (e4m3) or 12 (e2m3) contiguous bytes, 4-byte aligned, per tile, and
// lane hf stores the scale byte of tile hf.  crow: the row's codes of this head, srow: its two scale bytes.
template <int FMT>
__device__ __forceinline__ void store_mx_head(uint8_t* crow, uint8_t* srow, const f32x16& acc0, const f32x16& acc1, float inv,
                                              int hf, bool valid) {
    constexpr int PIECE_BITS = FMT == MX_E4M3 ? 32 : 24;
    constexpr uint32_t PIECE_MASK = FMT == MX_E4M3 ? 0xffffffffu : 0xffffffu;
    uint32_t sb[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const f32x16& acc = d ? acc1 : acc0;
        float v[16], amax = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] = bf2f(f2bf(acc[i] * inv));
            amax = fmaxf(amax, fabsf(v[i]));
        }
        const auto am = __builtin_amdgcn_permlane32_swap(__float_as_uint(amax), __float_as_uint(amax), false, false);
        amax = fmaxf(__uint_as_float(am[0]), __uint_as_float(am[1]));
        const uint64_t lo = mx_quant8_bits<FMT>(v, amax, sb[d]), hi = mx_quant8_bits<FMT>(v + 8, amax, sb[d]);
        const auto s0 = __builtin_amdgcn_permlane32_swap((uint32_t)lo & PIECE_MASK, (uint32_t)hi & PIECE_MASK, false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap((uint32_t)(lo >> PIECE_BITS) & PIECE_MASK,
                                                         (uint32_t)(hi >> PIECE_BITS) & PIECE_MASK, false, false);
        if constexpr (FMT == MX_E4M3) {
            const uint32_t o[4] = {s0[0], s0[1], s1[0], s1[1]};
            if (valid) __builtin_memcpy(__builtin_assume_aligned(crow + 32 * d + 16 * hf, 4), o, 16);
        } else {
            const uint32_t o[3] = {s0[0] | (s0[1] << 24), (s0[1] >> 8) | (s1[0] << 16), (s1[0] >> 16) | (s1[1] << 8)};
            if (valid) __builtin_memcpy(__builtin_assume_aligned(crow + 24 * d + 12 * hf, 4), o, 12);
        }
    }
    if (valid) srow[hf] = (uint8_t)(hf ? sb[1] : sb[0]);
}

template <int D> __device__ __forceinline__ int kswz(int row) { return D == 64 ? ((row >> 1) & 7) : (row & 15); }
template <int D> __device__ __forceinline__ int vswz(int row) { return D == 64 ? (((row >> 1) & 1) << 2) : ((row & 3) << 2); }

}  // namespace

// defined in attn_w4.hip: joint attention, head_dim 64, scores pre-scaled and bounded (one wave per SIMD, 512 query rows
// per workgroup); called from bya_attn_fwd
int bya_launch_attn_w4(const void* args, hipStream_t stream);
// the same launch with the MX epilogue: args = AttnMxArgs, fmt = MX_E4M3 / MX_E2M3
int bya_launch_attn_w4_mx(const void* args, int fmt, hipStream_t stream);
// its launch decisions (the launcher calls this too): grid, rows per workgroup, whether the stream-K grid runs and where it
// cuts.  ws_present: -1 = the current device's registered workspace decides, 0 / 1 = assume none / one (host-side queries)
struct bya_attn_w4_plan { int grid, q_tile, stream_k, sk_rem, sk_cut; };
void bya_plan_attn_w4(const void* args, int ws_present, bya_attn_w4_plan* plan);
