// Flash-attention forward for gfx950, head_dim 64 / 128, no mask, arbitrary Sq / Skv (tails masked).
//
// Replaces F.scaled_dot_product_attention inside diffusers' CogVideoXAttnProcessor2_0 (joint 17776-token
// self-attention, models/transformer.py:208,241), the default SDPA processor of the router's spatial
// attention (models/router.py:476) and of the audio cross-attention (models/audio_model.py:253), and the
// hand-rolled softmax attention of PerceiverCrossAttention / PerceiverAttention (models/router.py:264-270,
// 68-71; their q*s, k*s with s = d^-1/4 is scale = d^-1/2 on the product).
//
// Structure (v1): block = 4 waves x 32 query rows = 128 rows of one (batch, head); K/V tiles of 64 keys
// staged by global_load_lds_dwordx4 into a 2-deep LDS ring (source-side XOR swizzles: K for the
// ds_read_b128 A-operand reads, V for the ds_read_b64_tr_b16 transposed reads).
// QK^T is issued "swapped" (S^T = K.Q^T, v_mfma_f32_32x32x16_bf16) so a query row lives on one lane
// (+ its partner lane+32): the online softmax is an in-register reduction plus one cross-half exchange,
// and the S^T accumulator is directly the B operand of O^T += V^T.P^T (no LDS round trip for P).
// Blocks of one (batch, head) are dealt to one XCD so its K/V stream is served by that XCD's L2.
#include "attn_common.h"
#include "attn_mix32.h"         // lds_read128 .. pv_mfma, MixArgs, attn_mix32_body
#include "gemm_persistent.h"      // xcd_range
#include "routing_weights.h"
#include <stdlib.h>
#include "options.h"

namespace {

// (The build knobs BYA_ATTN_KPREFETCH / OCC / RING of rounds 2-4 -- all K fragment reads of a tile up front: +-1 % on the static-bound
// kernel, -30 % on the running-maximum one (profiles/history/r2_attn_ablation.json); a third K/V stage: no gain -- are gone since
// round 6; 2 is the ring depth they left.)
constexpr int ATTN_RING = 2;     // K/V stages in LDS
constexpr int Q_PER_WAVE = 32;
constexpr int Q_PER_BLOCK = 128;

// Stage a [64 keys][D] bf16 tile (rows of D*2 bytes) into LDS, lane-linear image, swizzled source (kswz / vswz:
// attn_common.h).
template <int D, bool IS_V>
__device__ __forceinline__ void stage_kv(const bf16_t* __restrict__ src, long long row_stride, int kv0, int kv_max,
                                         char* lds_tile, int wave, int lane) {
    constexpr int ROW_BYTES = D * 2;
    constexpr int ROWS_PER_INSTR = 1024 / ROW_BYTES;        // 8 (D=64) or 4 (D=128)
    constexpr int CHUNKS = ROW_BYTES / 16;                   // 8 or 16
    constexpr int INSTR_PER_WAVE = (KV_TILE / ROWS_PER_INSTR) / 4;
#pragma unroll
    for (int q = 0; q < INSTR_PER_WAVE; ++q) {
        const int rbase = (wave * INSTR_PER_WAVE + q) * ROWS_PER_INSTR;
        const int rl = rbase + lane / CHUNKS;
        const int slot = lane % CHUNKS;
        const int chunk = slot ^ (IS_V ? vswz<D>(rl) : kswz<D>(rl));
        int gr = kv0 + rl;
        gr = gr < kv_max ? gr : kv_max;
        const bf16_t* g = src + (long long)gr * row_stride + chunk * 8;
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(g), LDS_PTR(lds_tile + rbase * ROW_BYTES), 16, 0, 0);
    }
}

constexpr float RESCALE_THR = 6.0f;   // skip the O rescale while the running max grows by < 2^6 (P stays < 64)

// One 64-key tile: S^T = K.Q^T, online softmax, O^T += V^T.P^T.
// TAIL: only the first kv_valid keys of the tile exist (scores of the rest are forced to -inf -> P = 0).
//
// VALU diet (the kernel is VALU-issue-bound at head_dim 64: rocprofv3 SQ_ACTIVE_INST_VALU was 1.7x the MFMA busy
// time): q is pre-scaled by scale*log2(e) when it is loaded, and the running maximum is subtracted BY THE MATRIX PIPE:
// each score chain starts with one extra MFMA  ones[32 x 16] . mfrag[16 x 32]  whose B operand carries -m_run of the
// lane's query row (split into two bf16 terms, k = 0 and 1), so the accumulator already holds  s*c - m_run  and the
// common path is ONE v_exp_f32 per score (no per-element fma/sub; +2 MFMAs per tile, which the matrix pipe has room
// for).  m_run moves only when some row's maximum grows by more than 2^RESCALE_THR (wave-uniform branch); the first
// tile always sets it.  m_run is kept equal to the two-term bf16 value actually subtracted, so the algebra is exact.
// PRESCALED = true: the caller already folded scale*log2(e) into k (bya_qknorm_rope's k_scale applies it in fp32
// BEFORE k is rounded to bf16, so there is no extra rounding): scores are in exp2 units, one v_exp per score.
// false: scores and m_run stay in raw units and c = scale*log2(e) is applied in fp32 right before the exp
// (one extra v_mul per score).  Things tried and measured slower on MI355X (kept out of the tree): a 3-stage ring with
// S(t+1) issued before softmax(t) at 2 waves/SIMD (884 vs 910 TFLOP/s), two 32-row query blocks per wave sharing the
// K/V fragments (884 vs 933), pre-scaling q in the kernel (faster, but the second rounding of q costs 1e-3 accuracy).
// BOUNDED (with PRESCALED): the caller guarantees |score| <= B in exp2 units (the engine derives B from the q/k
// LayerNorm weights: ||LN(x) * gamma + beta|| <= 8 max|gamma| + ||beta||, RoPE is a rotation) and passes it in ``c``.
// Softmax is shift-invariant and with B <= 48 nothing can overflow or vanish without a shift at all: every
// P = exp2(s) lies in [2^-48, 2^48] (bf16 and fp32 share the 8-bit exponent; a row sum stays below 2^48 * Skv), so the
// whole maximum machinery -- 16 v_max3, the lane swap, the ballot, the rescale path and the two extra MFMAs --
// disappears from the tile and the score chains start from the MFMA's inline zero.
template <int D, bool TAIL, bool PRESCALED, bool BOUNDED = false>
__device__ __forceinline__ void attn_tile(const char* kt, const uint32_t (&vbase)[D / 32], const bf16x8 (&qf)[D / 16],
                                          f32x16 (&oacc)[D / 32], const bf16x8& ones, bf16x8& mfrag, float& m_run,
                                          float& l_run, bool first, int kv_valid, int r, int hf, float c) {
    const float thr = PRESCALED ? RESCALE_THR : RESCALE_THR / c;
    constexpr int ROW_BYTES = D * 2, DSTEPS = D / 16, DT = D / 32;
    f32x16 sacc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[u][i] = 0.f;
        if (!BOUNDED) sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, mfrag, sacc[u], 0, 0, 0);  // = -m_run everywhere
        const int krow = u * 32 + r;
#pragma unroll
        for (int s = 0; s < DSTEPS; ++s) {
            const int chunk = 2 * s + hf;
            const int off = krow * ROW_BYTES + ((chunk ^ kswz<D>(krow)) << 4);
            const bf16x8 kf = (BYA_ATTN_ABLATE & 2) ? qf[(s + 1 + u) % DSTEPS] : *reinterpret_cast<const bf16x8*>(kt + off);   // (+ u: no CSE of the two chains)
            sacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sacc[u], 0, 0, 0);
        }
    }
    // first V fragments can fly while the softmax runs
    VFrag<D> fa, fb;
    v_issue<D, 0>(fa, vbase);

    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (TAIL) {
                const int kv = u * 32 + (i & 3) + 8 * (i >> 2) + 4 * hf;
                if (kv >= kv_valid) sacc[u][i] = -INFINITY;
            }
            if (!BOUNDED) mx = fmaxf(mx, sacc[u][i]);
        }
    if (!BOUNDED) {
    {   // partner lane (lane ^ 32) holds the other 32 keys of this query row: one v_permlane32_swap, no LDS
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));        // row maximum RELATIVE to m_run
    }
    if (first || __builtin_amdgcn_ballot_w64(mx > thr) != 0) {      // wave-uniform slow path (rare)
        float delta = first ? mx : fmaxf(mx, 0.f);
        // new reference = a value exactly representable as hi + lo (two bf16 terms); delta is what really changes
        const float m_want = m_run + delta;
        const float m_hi = bf2f(f2bf(m_want));
        const float m_lo = bf2f(f2bf(m_want - m_hi));
        const float m_new = m_hi + m_lo;
        delta = m_new - m_run;
        if (!first) {
            const float alpha = __builtin_amdgcn_exp2f(PRESCALED ? -delta : -delta * c);
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[d][i] *= alpha;
        }
        m_run = m_new;
        if (hf == 0) {                               // lanes 0..31 carry k = 0..7 of the B operand
            mfrag[0] = (__bf16)(-m_hi);
            mfrag[1] = (__bf16)(-m_lo);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[u][i] -= delta;    // this tile's scores were taken against the old m_run
    }
    }
    float psum = 0.f;
    bf16x8 pf[4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float sv = PRESCALED ? sacc[u][tt * 8 + e] : sacc[u][tt * 8 + e] * c;
                const float pv = (BYA_ATTN_ABLATE & 1) ? fmaf(sv, 0.015625f, 1.0f) : __builtin_amdgcn_exp2f(sv);
                if (!(BYA_ATTN_ABLATE & 16)) psum += pv;
                pf[u * 2 + tt][e] = (__bf16)pv;
            }
    l_run += psum;

    // O^T += V^T . P^T, k-step ks covers tile keys 16ks + 8(e>>2) + 4hf + (e&3); reads run one step ahead.
    v_issue<D, 1>(fb, vbase);
    lgkm_wait<2 * DT>();
    pv_mfma<D>(fa, pf[0], oacc);
    v_issue<D, 2>(fa, vbase);
    lgkm_wait<2 * DT>();
    pv_mfma<D>(fb, pf[1], oacc);
    v_issue<D, 3>(fb, vbase);
    lgkm_wait<2 * DT>();
    pv_mfma<D>(fa, pf[2], oacc);
    lgkm_wait<0>();
    pv_mfma<D>(fb, pf[3], oacc);
}

// MX (head_dim 64 only): the MX epilogue (store_mx_head, attn_common.h) instead of the bf16 one; mx = the scale bytes and the
// format.  The format is a run-time, wave-uniform branch around the two epilogues, not a template parameter: one more copy
// of the hot loop per softmax variant instead of two.
template <int D, bool PRESCALED, bool BOUNDED = false, bool MX = false>
__device__ __forceinline__ void attn_fwd_body(const AttnArgs& p, char* smem, const AttnMxOut* mx = nullptr) {
    constexpr int ROW_BYTES = D * 2;
    constexpr int TILE_BYTES = KV_TILE * ROW_BYTES;
    constexpr int DSTEPS = D / 16;   // k-steps of the QK^T product
    constexpr int DT = D / 32;       // 32-row tiles of O^T
    constexpr int RING = ATTN_RING;
    // LDS ring: stage b holds K at smem + b*2*TILE_BYTES and V right behind it

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hf = lane >> 5;

    // block -> (bh, q-tile): blocks with equal (blockIdx % 8) share an XCD; give each XCD whole (batch, head)s.
    // When the (batch, head) count is not a multiple of 8 -- e.g. 6 heads per rank under head-parallel sharding, 26
    // (id, frame) pairs x 8 heads is fine -- every XCD takes a CONTIGUOUS eighth of the (head, q-tile) order instead:
    // it then works on one or two heads at a time (their K/V fit its L2) and every CU stays busy.  (Plain block order
    // spread every head over all eight L2s: 930 instead of 1150 TFLOP/s at 6 heads x 17776 tokens.)
    const int nbh = p.nb1 * p.nb2 * p.heads;
    int bh, qt;
    if (nbh % 8 == 0) {
        const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        bh = (j / p.nqt) * 8 + xcd;
        qt = j % p.nqt;
    } else {
        const int total = nbh * p.nqt, xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        const XcdRange xr = xcd_range(total, xcd);
        if (j >= xr.end - xr.base) return;
        bh = (xr.base + j) / p.nqt;
        qt = (xr.base + j) % p.nqt;
    }
    if (bh >= nbh) return;
    if (p.only_flagged && !p.only_flagged[bh]) return;       // second pass of the device-bound form: flagged heads only
    const int head = bh % p.heads;
    const int b12 = bh / p.heads;
    const int b1 = b12 / p.nb2, b2 = b12 % p.nb2;

    const bf16_t* Q = p.q + b1 * p.q_s1 + b2 * p.q_s2 + (long long)head * D;
    const bf16_t* K = p.k + b1 * p.k_s1 + b2 * p.k_s2 + (long long)head * D;
    const bf16_t* V = p.v + b1 * p.v_s1 + b2 * p.v_s2 + (long long)head * D;
    bf16_t* O = p.o + b1 * p.o_s1 + b2 * p.o_s2 + (long long)head * D;

    // ---- Q fragments (B operand of S^T = K.Q^T): lane (r,hf) holds Q[q0+r][16s + 8hf .. +7]
    const int q0 = qt * Q_PER_BLOCK + wave * Q_PER_WAVE;
    int qrow = q0 + r;
    const bool q_valid = qrow < p.Sq;
    qrow = q_valid ? qrow : p.Sq - 1;
    bf16x8 qf[DSTEPS];
#pragma unroll
    for (int s = 0; s < DSTEPS; ++s) {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(Q + (long long)qrow * p.q_row + s * 16 + hf * 8);
        qf[s] = __builtin_bit_cast(bf16x8, raw);
    }

    f32x16 oacc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[d][i] = 0.f;
    bf16x8 ones, mfrag;                  // A = 1 at k = 0, 1 (lanes 0..31), B = (-m_hi, -m_lo) of the lane's query row
#pragma unroll
    for (int e = 0; e < 8; ++e) { ones[e] = (__bf16)((hf == 0 && e < 2) ? 1.0f : 0.0f); mfrag[e] = (__bf16)0.0f; }
    float m_run = 0.f, l_run = 0.f;

    // per-lane LDS byte offsets of the transposed V reads inside a V tile (everything but the k-step is
    // lane-constant; the k-step and the lo/hi half go into the instruction's immediate offset)
    const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
    uint32_t voff[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        const int row = 4 * hf + tq;
        const int chunk = 4 * d + 2 * (g & 1) + (tp >> 1);
        voff[d] = row * ROW_BYTES + ((chunk ^ vswz<D>(row)) << 4) + (tp & 1) * 8;
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);

    // LDS-DMA staging through buffer_load ... lds: loop-invariant per-lane offsets, the tile advances in the scalar
    // offset, keys past Skv are outside the descriptor -> zeros land in LDS (their scores are masked in the tail tile).
    constexpr int ROWS_PER_INSTR = 1024 / ROW_BYTES, CHUNKS = ROW_BYTES / 16, NPIECE = 16 / ROWS_PER_INSTR;
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(
        (void*)K, 0, (int)(((long long)(p.Skv - 1) * p.k_row + D) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(
        (void*)V, 0, (int)(((long long)(p.Skv - 1) * p.v_row + D) * 2), 0x00020000);
    uint32_t kvo[NPIECE], vvo[NPIECE];
#pragma unroll
    for (int q = 0; q < NPIECE; ++q) {
        const int row = wave * 16 + q * ROWS_PER_INSTR + lane / CHUNKS, slot = lane % CHUNKS;
        kvo[q] = (uint32_t)row * (uint32_t)(p.k_row * 2) + ((slot ^ kswz<D>(row)) << 4);
        vvo[q] = (uint32_t)row * (uint32_t)(p.v_row * 2) + ((slot ^ vswz<D>(row)) << 4);
    }
    const int k_tile_stride = KV_TILE * (int)p.k_row * 2, v_tile_stride = KV_TILE * (int)p.v_row * 2;
    auto stage = [&](int t) {
        char* st = smem + (RING == 2 ? (t & 1) : (t % 3)) * 2 * TILE_BYTES + wave * 16 * ROW_BYTES;
#pragma unroll
        for (int q = 0; q < NPIECE; ++q) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, LDS_PTR(st + q * 1024), 16, kvo[q], t * k_tile_stride, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, LDS_PTR(st + TILE_BYTES + q * 1024), 16, vvo[q],
                                                     t * v_tile_stride, 0, 0);
        }
    };

    const int ntiles = (p.Skv + KV_TILE - 1) / KV_TILE;
    const int nfull = p.Skv / KV_TILE;
    stage(0);
    if (RING == 3 && ntiles > 1) stage(1);
    int slot = 0;                                         // ring slot of tile t

    for (int t = 0; t < nfull; ++t) {                     // full tiles: no masking code in the hot loop
        if constexpr (RING == 3) {
            // tile t has landed once all but the 2 NPIECE younger requests (tile t + 1) are done; raw barrier: a
            // __syncthreads() would drain the LDS-DMA in flight.  Tile t + 2 goes where tile t - 1 was: everybody is past it.
            if (t + 1 < ntiles) { if constexpr (NPIECE == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_barrier" ::: "memory");
            if (t + 2 < ntiles) stage(t + 2);
        } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < ntiles && (!(BYA_ATTN_ABLATE & 8) || t == 0)) stage(t + 1);
        }
        const char* kt = smem + slot * 2 * TILE_BYTES;
        uint32_t vbase[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) vbase[d] = lds0 + slot * 2 * TILE_BYTES + TILE_BYTES + voff[d];
        slot = (slot + 1 == RING) ? 0 : slot + 1;
        int tz = t;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(tz));                       // opaque: keeps hipcc from peeling the first iteration
#endif
        attn_tile<D, false, PRESCALED, BOUNDED>(kt, vbase, qf, oacc, ones, mfrag, m_run, l_run, tz == 0, KV_TILE, r, hf,
                                                BOUNDED ? p.score_bound : p.scale_log2);
    }
    if (nfull < ntiles) {                                 // ragged last tile
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* kt = smem + slot * 2 * TILE_BYTES;
        uint32_t vbase[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) vbase[d] = lds0 + slot * 2 * TILE_BYTES + TILE_BYTES + voff[d];
        attn_tile<D, true, PRESCALED, BOUNDED>(kt, vbase, qf, oacc, ones, mfrag, m_run, l_run, nfull == 0,
                                               p.Skv - nfull * KV_TILE, r, hf, BOUNDED ? p.score_bound : p.scale_log2);
    }

    // ---- epilogue: O[q][d] = O^T[d][q] / l ; lane (r,hf) holds d = 32dt + (i&3) + 8(i>>2) + 4hf
    const auto lsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
    const float l_tot = __uint_as_float(lsw[0]) + __uint_as_float(lsw[1]);
    const float inv = 1.0f / l_tot;
    if constexpr (MX) {
        static_assert(D == 64, "one MX block per 32-column tile, two per head");
        const long long row = q_valid ? q0 + r : 0;
        uint8_t* crow = reinterpret_cast<uint8_t*>(p.o) + b1 * p.o_s1 + b2 * p.o_s2 + row * p.o_row + (long long)head * 2 * mx_block_bytes(mx->fmt);
        uint8_t* srow = mx->scales + b1 * mx->s1 + b2 * mx->s2 + row * mx->row + 2 * head;
        if (mx->fmt == MX_E4M3) store_mx_head<MX_E4M3>(crow, srow, oacc[0], oacc[1], inv, hf, q_valid);
        else store_mx_head<MX_E2M3>(crow, srow, oacc[0], oacc[1], inv, hf, q_valid);
    } else {
    bf16_t* orow = O + (long long)(q_valid ? q0 + r : 0) * p.o_row;
#pragma unroll
    for (int d = 0; d < DT; ++d) store_o_tile(orow + d * 32, oacc[d], inv, hf, q_valid, p.o_wide != 0);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Cross-attention onto a handful of keys per identity, with the router's masked combine in its epilogue
// (bya_attn_kv_mix): the audio cross-attention (32 keys per latent frame and identity, 48 heads of 64;
// models/audio_model.py:247-258) and the face Perceiver cross-attention (32 face tokens per identity, 16 heads of 128;
// models/router.py:255-270).  Both are followed in the reference by  hidden += sum_id w[n, id] * to_out(o[id, n, :])
// (models/transformer.py:821-832, 895-936); to_out is linear, so the engine mixes first and projects once --
// and the mix needs nothing but the attention outputs of ONE token.  Unfused that was: attention writes o for every
// identity (2 x 108 MB), bya_routed_mix reads them back and writes z.  Here a workgroup holds its 128 query rows (shared
// by all identities), runs the one-tile attention once per identity on the K / V of that identity and accumulates
//     z = sum_id w[n, id] * (O_id / l_id)      in fp32, rounded to bf16 once,
// so o never reaches HBM: q is read once, z written once.  The per-identity attention is attn_tile<TAIL> of the generic
// kernel above (single tile, running maximum, keys past Skv masked), the weights are routing_weights.h.
template <int D>
__device__ __forceinline__ void attn_mix_body(const MixArgs& p, char* smem) {
    constexpr int ROW_BYTES = D * 2, TILE_BYTES = KV_TILE * ROW_BYTES, DSTEPS = D / 16, DT = D / 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hf = lane >> 5;
    int bid = blockIdx.x;
    const int qt = bid % p.nqt; bid /= p.nqt;
    const int head = bid % p.heads;
    const int grp = bid / p.heads;
    const bf16_t* Q = p.q + grp * p.q_grp + (long long)head * D;
    bf16_t* Z = p.z + grp * p.z_grp + (long long)head * D;
    const int q0 = qt * Q_PER_BLOCK + wave * Q_PER_WAVE;
    int qrow = q0 + r;
    const bool q_valid = qrow < p.Sq;
    qrow = q_valid ? qrow : p.Sq - 1;
    bf16x8 qf[DSTEPS];
#pragma unroll
    for (int s = 0; s < DSTEPS; ++s)
        qf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Q + (long long)qrow * p.q_row + s * 16 + hf * 8));
    float w[4];
    routing_weights_of(p.mode, p.n_id, p.af, p.r + ((long long)grp * p.Sq + qrow) * p.n_id, w);
    if (p.wsum && head == 0 && hf == 0 && q_valid) {
        float ws = 0.f;
        for (int i = 0; i < p.n_id; ++i) ws += w[i];
        p.wsum[(long long)grp * p.Sq + qrow] = ws;
    }

    const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
    uint32_t voff[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        const int row = 4 * hf + tq;
        const int chunk = 4 * d + 2 * (g & 1) + (tp >> 1);
        voff[d] = row * ROW_BYTES + ((chunk ^ vswz<D>(row)) << 4) + (tp & 1) * 8;
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)((hf == 0 && e < 2) ? 1.0f : 0.0f);

    f32x16 zacc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) zacc[d][i] = 0.f;
    for (int id = 0; id < p.n_id; ++id) {
        char* st = smem + (id & 1) * 2 * TILE_BYTES;           // two stages
        auto stage_id = [&](int j) {
            char* dst = smem + (j & 1) * 2 * TILE_BYTES;
            stage_kv<D, false>(p.k + j * p.k_id + grp * p.k_grp + (long long)head * D, p.k_row, 0, p.Skv - 1, dst, wave, lane);
            stage_kv<D, true>(p.v + j * p.v_id + grp * p.v_grp + (long long)head * D, p.v_row, 0, p.Skv - 1, dst + TILE_BYTES, wave, lane);
        };
        // the K/V of the first TWO identities are requested together (one memory round trip and one rendezvous for the
        // common two-identity case: the kernel is latency-bound, 13 rounds of small workgroups); identity id + 1 >= 3
        // lands in the stage identity id - 1 has left while id computes
        if (id == 0) {
            stage_id(0);
            if (p.n_id > 1) stage_id(1);
        }
        if (id != 1) {                                          // identity 1 landed together with identity 0
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        if (id >= 1 && id + 1 < p.n_id) {
            if (id == 1) __syncthreads();                       // every wave is done with identity 0's stage
            stage_id(id + 1);
        }
        f32x16 oacc[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[d][i] = 0.f;
        bf16x8 mfrag;
#pragma unroll
        for (int e = 0; e < 8; ++e) mfrag[e] = (__bf16)0.0f;
        float m_run = 0.f, l_run = 0.f;
        uint32_t vbase[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) vbase[d] = lds0 + (id & 1) * 2 * TILE_BYTES + TILE_BYTES + voff[d];
        attn_tile<D, true, false>(st, vbase, qf, oacc, ones, mfrag, m_run, l_run, true, p.Skv, r, hf, p.scale_log2);
        const auto lsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
        const float sc = w[id] / (__uint_as_float(lsw[0]) + __uint_as_float(lsw[1]));
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int i = 0; i < 16; ++i) zacc[d][i] = fmaf(sc, oacc[d][i], zacc[d][i]);
    }
    if (q_valid) {
        bf16_t* zrow = Z + (long long)(q0 + r) * p.z_row;
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                u32x2 o;
                o[0] = pack2bf(zacc[d][gq * 4 + 0], zacc[d][gq * 4 + 1]);
                o[1] = pack2bf(zacc[d][gq * 4 + 2], zacc[d][gq * 4 + 3]);
                *reinterpret_cast<u32x2*>(zrow + d * 32 + gq * 8 + hf * 4) = o;
            }
    }
}

__global__ __launch_bounds__(256, 2) void attn_kv_mix32_kernel_d64(MixArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<64>(p, smem);
}
__global__ __launch_bounds__(256) void attn_kv_mix32_kernel_d128(MixArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix32_body<128>(p, smem);
}

__global__ __launch_bounds__(256, 2) void attn_kv_mix_kernel_d64(MixArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix_body<64>(p, smem);
}
__global__ __launch_bounds__(256) void attn_kv_mix_kernel_d128(MixArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_mix_body<128>(p, smem);
}

// ------------------------------------------------------------------------------------------------------------------
// (rounds 2-4 had a two-query-blocks-per-wave static-bound kernel here, attn_fwd_kernel_d64_bounded2 -- the joint attention
// until the hand-placed one-wave-per-SIMD kernel of attn_w4.hip replaced it, then its BYA_ATTN_W4=0 A/B arm; retired in round 5
// together with the one-block bounded instance: every bounded launch now runs attn_w4.hip.  git history has the code.)

// (plain __global__ wrappers: hipcc's host pass did not emit the launch stub of the templated kernel once its body
// used the buffer-resource builtins)
__global__ __launch_bounds__(256, 4) void attn_fwd_kernel_d64(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_fwd_body<64, false>(p, smem);
}
__global__ __launch_bounds__(256, 4) void attn_fwd_kernel_d64_prescaled(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_fwd_body<64, true>(p, smem);
}
// the MX-output instances (bya_attn_fwd_mx); resource numbers: DESIGN.md section 11
template <bool PRESCALED>
__global__ __launch_bounds__(256, 4) void attn_fwd_mx_kernel_d64(AttnMxArgs pm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_fwd_body<64, PRESCALED, false, true>(pm.a, smem, &pm.mx);
}
__global__ __launch_bounds__(256) void attn_fwd_kernel_d128(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    attn_fwd_body<128, false>(p, smem);
}

inline float static_bound_limit() { return BYA_ATTN_BOUND_LIMIT; }

// Which softmax variant a (validated or not) descriptor selects: the ONE statement of that choice (bya_attn_variant,
// bya_attn_plan and the launcher all go through it).
inline int attn_variant_of(const bya_attn_desc* d) {
    if (d->head_dim == 128) return d->scores_prescaled ? BYA_ERR_UNSUPPORTED : BYA_ATTN_D128;
    if (d->head_dim != 64) return BYA_ERR_UNSUPPORTED;
    if (!d->scores_prescaled) return BYA_ATTN_D64_RUNNING_MAX;
    if (d->bound_dev && d->fallback_flags) return BYA_ATTN_D64_DEVICE_BOUND_W4;
    // a usable static bound keeps every P = exp2(s) and every row sum a normal number: |s| <= 90; otherwise the
    // running-maximum kernel runs
    if (!(d->score_bound > 0.f && d->score_bound <= static_bound_limit())) return BYA_ATTN_D64_PRESCALED;
    return BYA_ATTN_D64_STATIC_BOUND_W4;
}

// Argument checks of bya_attn_fwd and the kernel arguments they lead to (shared with bya_attn_plan, which has no q / k / v).
int attn_args_of(const void* q, const void* k, const void* v, void* o, const bya_attn_desc* d, AttnArgs& a) {
    if (!q || !k || !v || !o || !d) return BYA_ERR_SHAPE;
    if (d->head_dim != 64 && d->head_dim != 128) return BYA_ERR_UNSUPPORTED;
    if (d->heads <= 0 || d->nb1 <= 0 || d->nb2 <= 0 || d->Sq <= 0 || d->Skv <= 0) return BYA_ERR_SHAPE;
    if ((d->q_row | d->k_row | d->v_row | d->q_s1 | d->q_s2 | d->k_s1 | d->k_s2 | d->v_s1 | d->v_s2) % 8) return BYA_ERR_ALIGN;
    if ((d->o_row | d->o_s1 | d->o_s2) % 4) return BYA_ERR_ALIGN;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return BYA_ERR_ALIGN;
    if ((uintptr_t)o & 7) return BYA_ERR_ALIGN;
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)o;
    a.heads = d->heads; a.nb1 = d->nb1; a.nb2 = d->nb2; a.Sq = d->Sq; a.Skv = d->Skv;
    a.nqt = (d->Sq + Q_PER_BLOCK - 1) / Q_PER_BLOCK;
    a.q_s1 = d->q_s1; a.q_s2 = d->q_s2; a.q_row = d->q_row;
    a.k_s1 = d->k_s1; a.k_s2 = d->k_s2; a.k_row = d->k_row;
    a.v_s1 = d->v_s1; a.v_s2 = d->v_s2; a.v_row = d->v_row;
    a.o_s1 = d->o_s1; a.o_s2 = d->o_s2; a.o_row = d->o_row;
    a.o_wide = !((uintptr_t)o & 15) && (d->o_s1 | d->o_s2 | d->o_row) % 8 == 0 && !bya_ref_form(BYA_REF_ATTN_NARROW_STORE);
    a.scale_log2 = d->scale * 1.4426950408889634f;
    a.prescaled = d->scores_prescaled;
    if (a.prescaled && d->head_dim != 64) return BYA_ERR_UNSUPPORTED;
    a.score_bound = (a.prescaled && d->score_bound > 0.f && d->score_bound <= static_bound_limit()) ? d->score_bound : 0.f;
    a.sk_part = nullptr; a.sk_flags = nullptr;
    a.bound_dev = nullptr; a.bound_slots = 0; a.bound_heads = 0; a.bound_bh0 = 0; a.bound_limit = BYA_ATTN_BOUND_LIMIT;
    a.fallback = nullptr; a.only_flagged = nullptr;
    if (d->bound_dev && a.prescaled) {
        if (!d->fallback_flags || d->bound_slots < 1 || d->bound_slots > 64 || d->bound_bh0 < 0 ||
            d->bound_bh0 + d->nb1 * d->nb2 * d->heads > d->bound_heads) return BYA_ERR_SHAPE;
        if (((uintptr_t)d->bound_dev | (uintptr_t)d->fallback_flags) & 3) return BYA_ERR_ALIGN;
        a.bound_dev = d->bound_dev; a.bound_slots = d->bound_slots; a.bound_heads = d->bound_heads; a.bound_bh0 = d->bound_bh0;
        a.fallback = d->fallback_flags;
    }
    return BYA_OK;
}

// The launch decisions of bya_attn_fwd for checked arguments: which kernel(s), which grid, which store width.
// ws_present: -1 = the current device's registered stream-K workspace decides, 0 / 1 = assume none / one.
void attn_plan_of(const AttnArgs& a, int D, int ws_present, bya_attn_plan_info* p) {
    const int nbh = a.nb1 * a.nb2 * a.heads;
    p->grid = (nbh * a.nqt + 7) / 8 * 8;           // whole groups of 8 (one block per XCD); surplus blocks exit at once
    p->q_tile = Q_PER_BLOCK;
    p->stream_k = 0; p->sk_rem = 0; p->sk_cut = 0;
    p->o_wide = a.o_wide;
    p->second_launch = 0;
    if (D == 128) { p->variant = BYA_ATTN_D128; return; }
    if (!a.prescaled) { p->variant = BYA_ATTN_D64_RUNNING_MAX; return; }
    if (!a.bound_dev && !(a.score_bound > 0.f)) { p->variant = BYA_ATTN_D64_PRESCALED; return; }
    // data-dependent bound: the static kernel serves every head whose bound is usable and flags the others, the
    // running-maximum kernel right behind it serves exactly those (its other workgroups exit at once)
    p->variant = a.bound_dev ? BYA_ATTN_D64_DEVICE_BOUND_W4 : BYA_ATTN_D64_STATIC_BOUND_W4;
    p->second_launch = a.bound_dev ? 1 : 0;
    bya_attn_w4_plan w;
    bya_plan_attn_w4(&a, ws_present, &w);
    p->grid = w.grid; p->q_tile = w.q_tile; p->stream_k = w.stream_k; p->sk_rem = w.sk_rem; p->sk_cut = w.sk_cut;
}

template <int D>
int launch_attn(const AttnArgs& a, hipStream_t s) {
    bya_attn_plan_info pl;
    attn_plan_of(a, D, -1, &pl);
    const int nbh = a.nb1 * a.nb2 * a.heads;
    dim3 grid((nbh * a.nqt + 7) / 8 * 8);          // the 128-row kernels' grid (pl.grid unless the hand-placed kernel runs first)
    const size_t lds = (size_t)ATTN_RING * 2 * KV_TILE * D * 2;
    switch (pl.variant) {
        case BYA_ATTN_D64_DEVICE_BOUND_W4: {
            const int rc = bya_launch_attn_w4(&a, s);
            if (rc != BYA_OK) return rc;
            AttnArgs b = a;
            b.bound_dev = nullptr; b.score_bound = 0.f; b.only_flagged = a.fallback; b.fallback = nullptr;
            BYA_LAUNCH(attn_fwd_kernel_d64_prescaled, grid, dim3(256), lds, s, b);
            break;
        }
        case BYA_ATTN_D64_STATIC_BOUND_W4: return bya_launch_attn_w4(&a, s);
        case BYA_ATTN_D64_PRESCALED: BYA_LAUNCH(attn_fwd_kernel_d64_prescaled, grid, dim3(256), lds, s, a); break;
        case BYA_ATTN_D64_RUNNING_MAX: BYA_LAUNCH(attn_fwd_kernel_d64, grid, dim3(256), lds, s, a); break;
        default: BYA_LAUNCH(attn_fwd_kernel_d128, grid, dim3(256), lds, s, a); break;
    }
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}

// bya_attn_fwd_mx's arguments -> kernel arguments (shared with bya_attn_mx_plan): the descriptor's checks are those of
// bya_attn_fwd with an aligned stand-in for o, then a.o / a.o_* address the codes in bytes.
int attn_mx_args_of(const void* q, const void* k, const void* v, void* codes, void* scales, const bya_attn_desc* d, int out_fmt,
                    int64_t c_s1, int64_t c_s2, int64_t c_row, int64_t sc_s1, int64_t sc_s2, int64_t sc_row, AttnMxArgs& m) {
    if (!q || !k || !v || !codes || !scales || !d) return BYA_ERR_SHAPE;
    if (d->head_dim != 64) return BYA_ERR_UNSUPPORTED;                               // one MX block per 32 columns, two per head
    if (out_fmt != MX_E4M3 && out_fmt != MX_E2M3) return BYA_ERR_UNSUPPORTED;       // e2m1 is never an activation format
    if (d->o_s1 || d->o_s2 || d->o_row) return BYA_ERR_SHAPE;                        // there is no bf16 output: its strides stay 0
    const int rc = attn_args_of(q, k, v, reinterpret_cast<void*>((uintptr_t)16), d, m.a);
    if (rc != BYA_OK) return rc;
    const long long row_bytes = (long long)d->heads * 2 * mx_block_bytes(out_fmt);
    if (c_row < row_bytes || sc_row < 2LL * d->heads || c_s1 < 0 || c_s2 < 0 || sc_s1 < 0 || sc_s2 < 0) return BYA_ERR_SHAPE;
    if (((uintptr_t)codes | (uintptr_t)c_s1 | (uintptr_t)c_s2 | (uintptr_t)c_row) & 3) return BYA_ERR_ALIGN;   // 4-byte stores
    m.a.o = static_cast<bf16_t*>(codes); m.a.o_s1 = c_s1; m.a.o_s2 = c_s2; m.a.o_row = c_row; m.a.o_wide = 0;
    m.mx.scales = static_cast<uint8_t*>(scales); m.mx.s1 = sc_s1; m.mx.s2 = sc_s2; m.mx.row = sc_row; m.mx.fmt = out_fmt;
    return BYA_OK;
}

// the launches of launch_attn<64>, MX instances: same plan, same second launch for the flagged heads
int launch_attn_mx(const AttnMxArgs& m, int fmt, hipStream_t s) {
    const AttnArgs& a = m.a;
    bya_attn_plan_info pl;
    attn_plan_of(a, 64, -1, &pl);
    const int nbh = a.nb1 * a.nb2 * a.heads;
    const dim3 grid((nbh * a.nqt + 7) / 8 * 8), block(256);
    const size_t lds = (size_t)ATTN_RING * 2 * KV_TILE * 64 * 2;
    auto running = [&](const AttnMxArgs& x, bool prescaled) {
        if (prescaled) BYA_LAUNCH(attn_fwd_mx_kernel_d64<true>, grid, block, lds, s, x);
        else BYA_LAUNCH(attn_fwd_mx_kernel_d64<false>, grid, block, lds, s, x);
    };
    switch (pl.variant) {
        case BYA_ATTN_D64_DEVICE_BOUND_W4: {
            const int rc = bya_launch_attn_w4_mx(&m, fmt, s);
            if (rc != BYA_OK) return rc;
            AttnMxArgs b = m;
            b.a.bound_dev = nullptr; b.a.score_bound = 0.f; b.a.only_flagged = a.fallback; b.a.fallback = nullptr;
            running(b, true);
            break;
        }
        case BYA_ATTN_D64_STATIC_BOUND_W4: return bya_launch_attn_w4_mx(&m, fmt, s);
        case BYA_ATTN_D64_PRESCALED: running(m, true); break;
        case BYA_ATTN_D64_RUNNING_MAX: running(m, false); break;
        default: return BYA_ERR_UNSUPPORTED;
    }
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}

// row chunks per (group, head) of the <= 32-key form: about three 32-row tiles per wave, and at least ~4 workgroups per CU in total
inline int mix32_row_chunks(int rows) {
    const int n32 = (rows + 31) / 32;
    const int nqc = (n32 + 11) / 12;
    return nqc < 1 ? 1 : nqc;
}

// bya_attn_kv_mix: argument checks and launch decisions in one place (launcher and bya_attn_kv_mix_plan).
// qkv: the q, k, v addresses OR-ed together (0 in the query: it has none).
int mix_plan_of(const void* z, const bya_attn_mix_desc* d, int has_af, uintptr_t qkv, bya_attn_kv_mix_plan_info* p) {
    if (!z || !d) return BYA_ERR_SHAPE;
    if (d->head_dim != 64 && d->head_dim != 128) return BYA_ERR_UNSUPPORTED;
    if (d->heads <= 0 || d->n_id < 1 || d->n_id > 4 || d->n_grp <= 0 || d->Sq <= 0 || d->Skv <= 0 || d->Skv > KV_TILE) return BYA_ERR_SHAPE;
    if (has_af && d->n_id < 2) return BYA_ERR_SHAPE;  // the audio mix (af . r) needs >= 2 streams; routing_weights_of has no 1-stream audio case
    if ((d->q_grp | d->q_row | d->k_id | d->k_grp | d->k_row | d->v_id | d->v_grp | d->v_row) % 8) return BYA_ERR_ALIGN;
    if ((d->z_grp | d->z_row) % 4) return BYA_ERR_ALIGN;
    if (qkv & 15) return BYA_ERR_ALIGN;
    if ((uintptr_t)z & 7) return BYA_ERR_ALIGN;
    p->head_dim = d->head_dim;
    if (d->Skv <= 32 && !bya_ref_form(BYA_REF_KV_MIX_GENERIC) && !((uintptr_t)z & 15) && (d->z_grp | d->z_row) % 8 == 0) {
        p->form = BYA_KV_MIX_MIX32;
        p->row_chunks = mix32_row_chunks(d->Sq);
        p->lds_bytes = (d->n_id * 2 + 4) * 32 * d->head_dim * 2;    // K, V per identity + a z patch per wave
        p->big_lds = p->lds_bytes > 64 * 1024;                      // four identities at head_dim 128: 96 KiB
    } else {
        p->form = BYA_KV_MIX_ONE_TILE;
        p->row_chunks = (d->Sq + Q_PER_BLOCK - 1) / Q_PER_BLOCK;
        p->lds_bytes = 2 * 2 * KV_TILE * d->head_dim * 2;
        p->big_lds = 0;
    }
    p->grid = (int32_t)((long long)p->row_chunks * d->heads * d->n_grp);
    return BYA_OK;
}

// bya_attn_kv_mix_mx: argument checks and launch decisions (launcher and bya_attn_kv_mix_mx_plan).  The descriptor's checks
// and the plan are bya_attn_kv_mix's with an aligned stand-in for z; the MX epilogue exists on the <= 32-key form alone.
int mix_mx_plan_of(const void* codes, const void* scales, const bya_attn_mix_desc* d, int has_af, uintptr_t qkv, int out_fmt,
                   int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row, bya_attn_kv_mix_plan_info* p) {
    if (!codes || !scales || !d) return BYA_ERR_SHAPE;
    if (out_fmt != MX_E4M3 && out_fmt != MX_E2M3) return BYA_ERR_UNSUPPORTED;       // e2m1 is never an activation format
    if (d->z_grp || d->z_row) return BYA_ERR_SHAPE;                                  // there is no bf16 output: its strides stay 0
    const int rc = mix_plan_of(reinterpret_cast<const void*>((uintptr_t)16), d, has_af, qkv, p);
    if (rc != BYA_OK) return rc;
    if (p->form != BYA_KV_MIX_MIX32) return BYA_ERR_UNSUPPORTED;                     // Skv > 32, or the generic form asked for
    const long long blocks = (long long)d->heads * d->head_dim / 32;
    if (((uintptr_t)codes | (uintptr_t)c_grp | (uintptr_t)c_row) & 3) return BYA_ERR_ALIGN;      // (the entry's rule: e4m3 codes leave as dwords; e2m3's 2-byte stores would need less)
    if (c_row < blocks * mx_block_bytes(out_fmt) || sc_row < blocks || c_grp < 0 || sc_grp < 0) return BYA_ERR_SHAPE;
    return BYA_OK;
}

// bya_attn_kv_mix_seg / _mx_seg, before the grouped entry's own checks: the table against the descriptor (n_grp = the K / V
// groups it may name, Sq = the rows of q, r, z and wsum), and no group stride on anything the table addresses by row.
int mix_seg_check(const bya_attn_mix_segments* s, const bya_attn_mix_desc* d) {
    if (!s || !d) return BYA_ERR_SHAPE;
    if (s->n < 1 || s->n > BYA_MIX_MAX_SEGMENTS || d->q_grp || d->z_grp) return BYA_ERR_SHAPE;
    long long end = 0;                                          // ascending, no overlap: a segment starts at or behind the last one's end
    for (int i = 0; i < s->n; ++i) {
        if (s->len[i] <= 0 || s->grp[i] < 0 || s->grp[i] >= d->n_grp || s->start[i] < end) return BYA_ERR_SHAPE;
        end = (long long)s->start[i] + s->len[i];
        if (end > d->Sq) return BYA_ERR_SHAPE;
    }
    return BYA_OK;
}

// ... and behind them: the segment form exists on the <= 32-key form at head_dim 64 alone (the caller then issues the launches
// per segment); its row chunks are those of the LONGEST segment, its grid one workgroup per (segment, head, row chunk).
int mix_seg_plan_of(const bya_attn_mix_segments* s, const bya_attn_mix_desc* d, bya_attn_kv_mix_plan_info* p) {
    if (p->form != BYA_KV_MIX_MIX32 || d->head_dim != 64) return BYA_ERR_UNSUPPORTED;
    int longest = 0;
    for (int i = 0; i < s->n; ++i) longest = s->len[i] > longest ? s->len[i] : longest;
    p->row_chunks = mix32_row_chunks(longest);
    p->grid = (int32_t)((long long)p->row_chunks * d->heads * s->n);
    return BYA_OK;
}

// bya_attn_kv_mix_batch / _mx_batch, behind the single-sample entry's own checks (p = its plan): the sample strides.  `out` /
// `out_extent`: the strides of the outputs that are present (z; or codes, scales; wsum where given) and what ONE sample covers of
// each, in the stride's unit -- samples must not overlap.  The batch exists on the <= 32-key form alone.  On success p->grid is
// the whole launch's: the single-sample grid (returned in *grid1, blockIdx.x) times n (blockIdx.y).
int mix_batch_plan_of(int32_t n, const int64_t (&in)[5], const int64_t* out, const long long* out_extent, int n_out,
                      bya_attn_kv_mix_plan_info* p, int* grid1) {
    if (n < 1 || n > 65535) return BYA_ERR_SHAPE;
    if ((in[0] | in[1] | in[2] | in[3] | in[4]) < 0) return BYA_ERR_SHAPE;
    if ((in[0] | in[1] | in[2]) % 8) return BYA_ERR_ALIGN;                       // q, k, v: 16-byte loads in every sample
    for (int i = 0; i < n_out; ++i)
        if (out[i] < 0 || out_extent[i] < 0 || (n > 1 && out[i] < out_extent[i])) return BYA_ERR_SHAPE;
    if (p->form != BYA_KV_MIX_MIX32) return BYA_ERR_UNSUPPORTED;
    if ((long long)p->grid * n > 0x7fffffffLL) return BYA_ERR_SHAPE;
    *grid1 = p->grid;
    p->grid *= n;
    return BYA_OK;
}

// what one sample covers of an output whose row n of group g starts at g * grp + n * row and is `width` wide (-1: a negative
// stride, which the batch entries refuse: nothing could be said about overlap)
inline long long mix_extent(const bya_attn_mix_desc* d, long long grp, long long row, long long width) {
    if (grp < 0 || row < 0) return -1;
    return (d->n_grp - 1) * grp + (d->Sq - 1) * row + width;
}

// (every sample takes the form sample 0 takes: a z stride that is no multiple of 8 elements would send the odd samples to the
// generic form, so it is declined like that form)
int mix_batch_all_of(const void* z, const bya_attn_mix_desc* d, int has_af, uintptr_t qkv, int has_wsum, const bya_attn_mix_samples& b,
                     bya_attn_kv_mix_plan_info* p, int* grid1, ByaMixSampleStrides& s) {
    int rc = mix_plan_of(z, d, has_af, qkv, p);
    if (rc != BYA_OK) return rc;
    if (b.z % 4) return BYA_ERR_ALIGN;
    const int64_t in[5] = {b.q, b.k, b.v, b.r, has_af ? b.af : 0};
    const int64_t out[2] = {b.z, b.wsum};
    const long long ext[2] = {mix_extent(d, d->z_grp, d->z_row, (long long)d->heads * d->head_dim), (long long)d->n_grp * d->Sq};
    rc = mix_batch_plan_of(b.n, in, out, ext, has_wsum ? 2 : 1, p, grid1);
    if (rc != BYA_OK) return rc;
    if (b.z % 8) return BYA_ERR_UNSUPPORTED;
    s = ByaMixSampleStrides{b.q, b.k, b.v, b.r, in[4], b.z, has_wsum ? b.wsum : 0, 0, 0, b.n};
    return BYA_OK;
}

int mix_mx_batch_all_of(const void* codes, const void* scales, const bya_attn_mix_desc* d, int has_af, uintptr_t qkv, int has_wsum,
                        int out_fmt, int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row, const bya_attn_mix_mx_samples& b,
                        bya_attn_kv_mix_plan_info* p, int* grid1, ByaMixSampleStrides& s) {
    int rc = mix_mx_plan_of(codes, scales, d, has_af, qkv, out_fmt, c_grp, c_row, sc_grp, sc_row, p);
    if (rc != BYA_OK) return rc;
    if (b.codes & 3) return BYA_ERR_ALIGN;
    const long long blocks = (long long)d->heads * d->head_dim / 32;
    const int64_t in[5] = {b.q, b.k, b.v, b.r, has_af ? b.af : 0};
    const int64_t out[3] = {b.codes, b.scales, b.wsum};
    const long long ext[3] = {mix_extent(d, c_grp, c_row, blocks * mx_block_bytes(out_fmt)), mix_extent(d, sc_grp, sc_row, blocks),
                              (long long)d->n_grp * d->Sq};
    rc = mix_batch_plan_of(b.n, in, out, ext, has_wsum ? 3 : 2, p, grid1);
    if (rc != BYA_OK) return rc;
    s = ByaMixSampleStrides{b.q, b.k, b.v, b.r, in[4], 0, has_wsum ? b.wsum : 0, b.codes, b.scales, b.n};
    return BYA_OK;
}

}  // namespace

// Which kernel a descriptor selects (reported to the host so tests and bench.py can say which softmax variant ran).
extern "C" int bya_attn_variant(const bya_attn_desc* d) {
    if (!d) return BYA_ERR_SHAPE;
    return attn_variant_of(d);
}

extern "C" int bya_attn_plan(const bya_attn_desc* d, const void* o, int32_t workspace_assumed, bya_attn_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    AttnArgs a;
    const void* const aligned = reinterpret_cast<const void*>((uintptr_t)16);      // q, k, v stand-ins: the query has none
    const int rc = attn_args_of(aligned, aligned, aligned, const_cast<void*>(o), d, a);
    if (rc != BYA_OK) return rc;
    attn_plan_of(a, d->head_dim, workspace_assumed, plan);
    return BYA_OK;
}

extern "C" int bya_attn_fwd(const void* q, const void* k, const void* v, void* o, const bya_attn_desc* d,
                            hipStream_t stream) {
    AttnArgs a;
    const int rc = attn_args_of(q, k, v, o, d, a);
    if (rc != BYA_OK) return rc;
    return d->head_dim == 64 ? launch_attn<64>(a, stream) : launch_attn<128>(a, stream);
}

extern "C" int bya_attn_mx_plan(const bya_attn_desc* d, const void* codes, const void* scales, int32_t out_fmt, int64_t c_s1,
                               int64_t c_s2, int64_t c_row, int64_t sc_s1, int64_t sc_s2, int64_t sc_row,
                               int32_t workspace_assumed, bya_attn_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    AttnMxArgs m;
    const void* const aligned = reinterpret_cast<const void*>((uintptr_t)16);      // q, k, v stand-ins: the query has none
    const int rc = attn_mx_args_of(aligned, aligned, aligned, const_cast<void*>(codes), const_cast<void*>(scales), d, out_fmt,
                                   c_s1, c_s2, c_row, sc_s1, sc_s2, sc_row, m);
    if (rc != BYA_OK) return rc;
    attn_plan_of(m.a, 64, workspace_assumed, plan);
    return BYA_OK;
}

extern "C" int bya_attn_fwd_mx(const void* q, const void* k, const void* v, void* codes, void* scales, const bya_attn_desc* d,
                              int32_t out_fmt, int64_t c_s1, int64_t c_s2, int64_t c_row, int64_t sc_s1, int64_t sc_s2,
                              int64_t sc_row, hipStream_t stream) {
    AttnMxArgs m;
    const int rc = attn_mx_args_of(q, k, v, codes, scales, d, out_fmt, c_s1, c_s2, c_row, sc_s1, sc_s2, sc_row, m);
    if (rc != BYA_OK) return rc;
    return launch_attn_mx(m, out_fmt, stream);
}

extern "C" int bya_attn_kv_mix_plan(const void* z, const void* af, const bya_attn_mix_desc* d, bya_attn_kv_mix_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info p;
    const int rc = mix_plan_of(z, d, af != nullptr, 0, &p);
    if (rc == BYA_OK) *plan = p;
    return rc;
}

extern "C" int bya_attn_kv_mix(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                               const bya_attn_mix_desc* d, hipStream_t stream) {
    if (!q || !k || !v || !r || !z || !d) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info pl;
    const int prc = mix_plan_of(z, d, af != nullptr, (uintptr_t)q | (uintptr_t)k | (uintptr_t)v, &pl);
    if (prc != BYA_OK) return prc;
    MixArgs a;
    mix_args_of(q, k, v, r, af, wsum, d, pl.row_chunks, a);
    a.z = (bf16_t*)z; a.z_grp = d->z_grp; a.z_row = d->z_row;
    const dim3 grid((unsigned)pl.grid);
    const size_t lds = (size_t)pl.lds_bytes;
    if (pl.form == BYA_KV_MIX_MIX32) {
        if (pl.big_lds) {
            static std::atomic<unsigned long long> big64{0}, big128{0};
            const int rc = d->head_dim == 64
                ? bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_kernel_d64), 160 * 1024, big64)
                : bya_allow_big_lds(reinterpret_cast<const void*>(attn_kv_mix32_kernel_d128), 160 * 1024, big128);
            if (rc != BYA_OK) return rc;
        }
        if (d->head_dim == 64) BYA_LAUNCH(attn_kv_mix32_kernel_d64, grid, dim3(256), lds, stream, a);
        else BYA_LAUNCH(attn_kv_mix32_kernel_d128, grid, dim3(256), lds, stream, a);
        return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
    }
    if (d->head_dim == 64) BYA_LAUNCH(attn_kv_mix_kernel_d64, grid, dim3(256), lds, stream, a);
    else BYA_LAUNCH(attn_kv_mix_kernel_d128, grid, dim3(256), lds, stream, a);
    return hipGetLastError() == hipSuccess ? BYA_OK : BYA_ERR_LAUNCH;
}

extern "C" int bya_attn_kv_mix_mx_plan(const void* codes, const void* scales, const void* af, const bya_attn_mix_desc* d,
                                      int32_t out_fmt, int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row,
                                      bya_attn_kv_mix_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info p;
    const int rc = mix_mx_plan_of(codes, scales, d, af != nullptr, 0, out_fmt, c_grp, c_row, sc_grp, sc_row, &p);
    if (rc == BYA_OK) *plan = p;
    return rc;
}

extern "C" int bya_attn_kv_mix_mx(const void* q, const void* k, const void* v, const void* r, const void* af, void* codes,
                                  void* scales, float* wsum, const bya_attn_mix_desc* d, int32_t out_fmt, int64_t c_grp,
                                  int64_t c_row, int64_t sc_grp, int64_t sc_row, hipStream_t stream) {
    if (!q || !k || !v || !r) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info pl;
    const int prc = mix_mx_plan_of(codes, scales, d, af != nullptr, (uintptr_t)q | (uintptr_t)k | (uintptr_t)v, out_fmt, c_grp,
                                   c_row, sc_grp, sc_row, &pl);
    if (prc != BYA_OK) return prc;
    ByaMixMxOut out;
    out.codes = static_cast<uint8_t*>(codes); out.scales = static_cast<uint8_t*>(scales);
    out.c_grp = c_grp; out.c_row = c_row; out.s_grp = sc_grp; out.s_row = sc_row; out.fmt = out_fmt;
    return bya_launch_attn_kv_mix32_mx(q, k, v, r, af, wsum, *d, pl, out, nullptr, nullptr, stream);
}

extern "C" int bya_attn_kv_mix_seg_plan(const void* z, const void* af, const bya_attn_mix_desc* d, const bya_attn_mix_segments* seg,
                                       bya_attn_kv_mix_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info p;
    int rc = mix_seg_check(seg, d);
    if (rc == BYA_OK) rc = mix_plan_of(z, d, af != nullptr, 0, &p);
    if (rc == BYA_OK) rc = mix_seg_plan_of(seg, d, &p);
    if (rc == BYA_OK) *plan = p;
    return rc;
}

extern "C" int bya_attn_kv_mix_seg(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                                   const bya_attn_mix_desc* d, const bya_attn_mix_segments* seg, hipStream_t stream) {
    if (!q || !k || !v || !r || !z) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info pl;
    int rc = mix_seg_check(seg, d);
    if (rc == BYA_OK) rc = mix_plan_of(z, d, af != nullptr, (uintptr_t)q | (uintptr_t)k | (uintptr_t)v, &pl);
    if (rc == BYA_OK) rc = mix_seg_plan_of(seg, d, &pl);
    if (rc != BYA_OK) return rc;
    return bya_launch_attn_kv_mix32_seg(q, k, v, r, af, z, wsum, *d, pl, *seg, stream);
}

extern "C" int bya_attn_kv_mix_mx_seg_plan(const void* codes, const void* scales, const void* af, const bya_attn_mix_desc* d,
                                          const bya_attn_mix_segments* seg, int32_t out_fmt, int64_t c_grp, int64_t c_row,
                                          int64_t sc_grp, int64_t sc_row, bya_attn_kv_mix_plan_info* plan) {
    if (!plan || c_grp || sc_grp) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info p;
    int rc = mix_seg_check(seg, d);
    if (rc == BYA_OK) rc = mix_mx_plan_of(codes, scales, d, af != nullptr, 0, out_fmt, c_grp, c_row, sc_grp, sc_row, &p);
    if (rc == BYA_OK) rc = mix_seg_plan_of(seg, d, &p);
    if (rc == BYA_OK) *plan = p;
    return rc;
}

extern "C" int bya_attn_kv_mix_mx_seg(const void* q, const void* k, const void* v, const void* r, const void* af, void* codes,
                                      void* scales, float* wsum, const bya_attn_mix_desc* d, const bya_attn_mix_segments* seg,
                                      int32_t out_fmt, int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row,
                                      hipStream_t stream) {
    if (!q || !k || !v || !r || c_grp || sc_grp) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info pl;
    int rc = mix_seg_check(seg, d);
    if (rc == BYA_OK) rc = mix_mx_plan_of(codes, scales, d, af != nullptr, (uintptr_t)q | (uintptr_t)k | (uintptr_t)v, out_fmt, c_grp,
                                          c_row, sc_grp, sc_row, &pl);
    if (rc == BYA_OK) rc = mix_seg_plan_of(seg, d, &pl);
    if (rc != BYA_OK) return rc;
    ByaMixMxOut out;
    out.codes = static_cast<uint8_t*>(codes); out.scales = static_cast<uint8_t*>(scales);
    out.c_grp = 0; out.c_row = c_row; out.s_grp = 0; out.s_row = sc_row; out.fmt = out_fmt;
    return bya_launch_attn_kv_mix32_mx(q, k, v, r, af, wsum, *d, pl, out, seg, nullptr, stream);
}

extern "C" int bya_attn_kv_mix_batch_plan(const void* z, const void* af, const bya_attn_mix_desc* d, bya_attn_mix_samples batch,
                                         bya_attn_kv_mix_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info p;
    ByaMixSampleStrides s;
    int grid1;
    const int rc = mix_batch_all_of(z, d, af != nullptr, 0, batch.wsum != 0, batch, &p, &grid1, s);
    if (rc == BYA_OK) *plan = p;
    return rc;
}

extern "C" int bya_attn_kv_mix_batch(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                                     const bya_attn_mix_desc* d, bya_attn_mix_samples batch, hipStream_t stream) {
    if (!q || !k || !v || !r || !z || !d) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info pl;
    ByaMixSampleStrides s;
    int grid1;
    const int rc = mix_batch_all_of(z, d, af != nullptr, (uintptr_t)q | (uintptr_t)k | (uintptr_t)v, wsum != nullptr || batch.wsum != 0, batch, &pl, &grid1, s);
    if (rc != BYA_OK) return rc;
    pl.grid = grid1;
    return bya_launch_attn_kv_mix32_batch(q, k, v, r, af, z, wsum, *d, pl, s, stream);
}

extern "C" int bya_attn_kv_mix_mx_batch_plan(const void* codes, const void* scales, const void* af, const bya_attn_mix_desc* d,
                                            int32_t out_fmt, int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row,
                                            bya_attn_mix_mx_samples batch, bya_attn_kv_mix_plan_info* plan) {
    if (!plan) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info p;
    ByaMixSampleStrides s;
    int grid1;
    const int rc = mix_mx_batch_all_of(codes, scales, d, af != nullptr, 0, batch.wsum != 0, out_fmt, c_grp, c_row, sc_grp, sc_row, batch,
                                       &p, &grid1, s);
    if (rc == BYA_OK) *plan = p;
    return rc;
}

extern "C" int bya_attn_kv_mix_mx_batch(const void* q, const void* k, const void* v, const void* r, const void* af, void* codes,
                                        void* scales, float* wsum, const bya_attn_mix_desc* d, int32_t out_fmt, int64_t c_grp,
                                        int64_t c_row, int64_t sc_grp, int64_t sc_row, bya_attn_mix_mx_samples batch,
                                        hipStream_t stream) {
    if (!q || !k || !v || !r) return BYA_ERR_SHAPE;
    bya_attn_kv_mix_plan_info pl;
    ByaMixSampleStrides s;
    int grid1;
    const int rc = mix_mx_batch_all_of(codes, scales, d, af != nullptr, (uintptr_t)q | (uintptr_t)k | (uintptr_t)v,
                                       wsum != nullptr || batch.wsum != 0, out_fmt, c_grp, c_row, sc_grp, sc_row, batch, &pl, &grid1, s);
    if (rc != BYA_OK) return rc;
    pl.grid = grid1;
    ByaMixMxOut out;
    out.codes = static_cast<uint8_t*>(codes); out.scales = static_cast<uint8_t*>(scales);
    out.c_grp = c_grp; out.c_row = c_row; out.s_grp = sc_grp; out.s_row = sc_row; out.fmt = out_fmt;
    return bya_launch_attn_kv_mix32_mx(q, k, v, r, af, wsum, *d, pl, out, nullptr, &s, stream);
}
