// The <= 32-key form of bya_attn_kv_mix (attn_mix32_body) and the fragment helpers it shares with the attention kernels of
// attn.hip.  Four translation units instantiate it: attn.hip (the bf16 instances), attn_mix_seg.hip (the bf16 instance that
// takes its rows from a segment table, bya_attn_kv_mix_seg), attn_mix_batch.hip (the bf16 instances whose blockIdx.y is the sample
// of a batch, bya_attn_kv_mix_batch) and attn_mix_mx.hip (the MX-output instances of all three, built without the SLP vectoriser
// like every translation unit that holds a quantiser: build.py, NO_SLP_SOURCES).
#pragma once
#include "attn_common.h"
#include "routing_weights.h"

// Where the MX-output instances write (bya_attn_kv_mix_mx): strides in BYTES, fmt = MX_E4M3 / MX_E2M3.  A named type with
// external linkage: it crosses from attn.hip to attn_mix_mx.hip in bya_launch_attn_kv_mix32_mx's signature.
struct ByaMixMxOut { uint8_t* codes; uint8_t* scales; long long c_grp, c_row, s_grp, s_row; int fmt; };
// What separates the samples of a batch launch (bya_attn_kv_mix_batch / _mx_batch): elements of each pointer's type, codes and
// scales in BYTES; n samples.  External linkage for the same reason.
struct ByaMixSampleStrides { long long q, k, v, r, af, z, wsum, codes, scales; int n; };

namespace {

// Ablation build (tools/attn_ablate.py; NEVER defined in the product build): a bit mask of work to leave out of the hot
// loop, results become meaningless, only the time is read.  1: v_exp -> one FMA, 2: K fragments read from LDS once per
// block instead of per tile, 4: V fragments likewise, 8: no K/V staging after the first tile, 16: no row-sum adds.
#ifndef BYA_ATTN_ABLATE
#define BYA_ATTN_ABLATE 0
#endif

// ds_read_b64_tr_b16 through inline asm: the builtin makes hipcc drain the in-flight LDS-DMA of the NEXT tile
// (s_waitcnt vmcnt(0)) in the middle of the loop; an asm read is invisible to that bookkeeping.  Waits for these
// reads are counted by hand (lgkmcnt), always followed by sched_barrier(0) so no MFMA is hoisted above the wait.
template <int OFF>
__device__ __forceinline__ s16x4 lds_tr_read(uint32_t addr) {
    s16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}

template <int OFF>
__device__ __forceinline__ bf16x8 lds_read128(uint32_t addr) {
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
    return v;
}

template <int N>
__device__ __forceinline__ void lgkm_wait() {
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(N) : "memory");
    __builtin_amdgcn_sched_barrier(0);
}

template <int D>
struct VFrag {
    s16x4 lo[D / 32], hi[D / 32];
};

template <int D, int KS>
__device__ __forceinline__ void v_issue(VFrag<D>& f, const uint32_t (&vbase)[D / 32]) {
    constexpr int RB = D * 2;
    if ((BYA_ATTN_ABLATE & 4) && KS >= 2) return;          // ablation: half of the V reads (k-steps 2, 3 reuse 0, 1)
#pragma unroll
    for (int d = 0; d < D / 32; ++d) {
        f.lo[d] = lds_tr_read<KS * 16 * RB>(vbase[d]);
        f.hi[d] = lds_tr_read<KS * 16 * RB + 8 * RB>(vbase[d]);
    }
}

template <int D>
__device__ __forceinline__ void pv_mfma(const VFrag<D>& f, const bf16x8& pf, f32x16 (&oacc)[D / 32]) {
    typedef __attribute__((ext_vector_type(8))) short s16x8;
#pragma unroll
    for (int d = 0; d < D / 32; ++d) {
        const s16x8 both = {f.lo[d][0], f.lo[d][1], f.lo[d][2], f.lo[d][3], f.hi[d][0], f.hi[d][1], f.hi[d][2], f.hi[d][3]};
        oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, both), pf, oacc[d], 0, 0, 0);
    }
}

// Kernel arguments of bya_attn_kv_mix (the kernels and what they compute: attn.hip).
struct MixArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* z; const bf16_t* r; const bf16_t* af; float* wsum;
    int heads, n_id, n_grp, Sq, Skv, nqt, mode;
    long long q_grp, q_row, k_id, k_grp, k_row, v_id, v_grp, v_row, z_grp, z_row;
    float scale_log2;
};
// The MX-output instances of the <= 32-key form (bya_attn_kv_mix_mx) take MixArgs with z = nullptr plus a ByaMixMxOut.  The bf16
// instances' kernel argument stays MixArgs alone.
struct MixMxArgs { MixArgs a; ByaMixMxOut mx; };
// The segment instances (bya_attn_kv_mix_seg / _mx_seg) carry the caller's table by value behind them: no device memory, so a
// captured graph holds it.  There MixArgs.n_grp / Sq bound the table (checked on the host) and the kernel reads neither.
struct MixSegArgs { MixArgs a; bya_attn_mix_segments seg; };
struct MixMxSegArgs { MixArgs a; ByaMixMxOut mx; bya_attn_mix_segments seg; };
// The batch instances (bya_attn_kv_mix_batch / _mx_batch): sample blockIdx.y of a launch is the single-sample launch with every
// pointer advanced by its stride (ByaMixSampleStrides).  By value like the segment table.
struct MixBatchArgs { MixArgs a; ByaMixSampleStrides s; };
struct MixMxBatchArgs { MixArgs a; ByaMixMxOut mx; ByaMixSampleStrides s; };

// the arguments of sample blockIdx.y: what attn_mix32_body gets in a batch instance.  The body below it is the single-sample
// launch's, blockIdx.x walks the (group, head, row chunk) of ONE sample as there: a row's arithmetic does not know the batch.
__device__ __forceinline__ MixArgs mix_sample_args(const MixArgs& a, const ByaMixSampleStrides& s) {
    const long long b = blockIdx.y;
    MixArgs p = a;
    p.q += b * s.q; p.k += b * s.k; p.v += b * s.v; p.r += b * s.r;
    if (p.af) p.af += b * s.af;
    if (p.z) p.z += b * s.z;
    if (p.wsum) p.wsum += b * s.wsum;
    return p;
}
__device__ __forceinline__ ByaMixMxOut mix_sample_out(const ByaMixMxOut& o, const ByaMixSampleStrides& s) {
    const long long b = blockIdx.y;
    ByaMixMxOut m = o;
    m.codes += b * s.codes; m.scales += b * s.scales;
    return m;
}

// bya_attn_kv_mix's descriptor -> kernel arguments (z and its strides: the bf16 entry's alone)
inline void mix_args_of(const void* q, const void* k, const void* v, const void* r, const void* af, float* wsum,
                        const bya_attn_mix_desc* d, int row_chunks, MixArgs& a) {
    a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.z = nullptr;
    a.r = (const bf16_t*)r; a.af = (const bf16_t*)af; a.wsum = wsum;
    a.heads = d->heads; a.n_id = d->n_id; a.n_grp = d->n_grp; a.Sq = d->Sq; a.Skv = d->Skv;
    a.nqt = row_chunks; a.mode = af ? 1 : 0;
    a.q_grp = d->q_grp; a.q_row = d->q_row; a.k_id = d->k_id; a.k_grp = d->k_grp; a.k_row = d->k_row;
    a.v_id = d->v_id; a.v_grp = d->v_grp; a.v_row = d->v_row; a.z_grp = 0; a.z_row = 0;
    a.scale_log2 = d->scale * 1.4426950408889634f;
}

// ---- the <= 32-key form (both callers: 32 audio context tokens per frame, 32 face tokens per identity) --------------
// attn_mix_body runs ONE 128-row query tile per workgroup: stage K / V (64-row tiles, half of them padding), rendezvous,
// attention on a 64-key tile with the upper half masked, store -- 6864 workgroups per audio launch, each a serial chain
// of memory round trips with a barrier in the middle, twice the MFMAs and exps the 32 keys need: 87 us for 218 MB.
// Here a workgroup owns one (group, head) and a CHUNK of its query rows: the K / V of every identity are staged once
// (32 rows each) and stay in LDS, after the one rendezvous every wave walks its own 32-row tiles (tile w, w + 4, ... of the
// chunk) with no further barrier: per tile 4 K-fragment reads, D / 16 MFMAs for S^T, one softmax over 32 keys (two lanes per
// query), D / 16 MFMAs for O^T, per identity.  blockIdx runs over the heads fastest, so the workgroups in flight
// together read the 128-byte head segments of the SAME rows (whole 6-KiB rows over a short time, not one segment per
// row spread over the launch).  Arithmetic per element is that of attn_tile<TAIL> on a first tile (the two-term bf16
// maximum, the order of the row sum, k-steps 0 and 1 of P.V) -- so results are BIT-IDENTICAL to attn_mix_body and, for
// one-hot masks, to bya_attn_fwd's rows (tests/test_kernels_gpu.py).
template <int D>
__device__ __forceinline__ void stage_kv32(const bf16_t* __restrict__ src, long long row_stride, int kv_max, char* lds_tile,
                                           int wave, int lane, bool is_v) {
    constexpr int ROW_BYTES = D * 2, ROWS_PER_INSTR = 1024 / ROW_BYTES, CHUNKS = ROW_BYTES / 16;
    for (int q = wave; q < 32 / ROWS_PER_INSTR; q += 4) {
        const int rbase = q * ROWS_PER_INSTR;
        const int rl = rbase + lane / CHUNKS;
        const int slot = lane % CHUNKS;
        const int chunk = slot ^ (is_v ? vswz<D>(rl) : kswz<D>(rl));
        const int gr = rl < kv_max ? rl : kv_max;
        const bf16_t* g = src + (long long)gr * row_stride + chunk * 8;
        __builtin_amdgcn_global_load_lds(GLOBAL_PTR(g), LDS_PTR(lds_tile + rbase * ROW_BYTES), 16, 0, 0);
    }
}

//
// MX = true (bya_attn_kv_mix_mx): the second epilogue.  z is the operand of the cross-attention's to_out and nothing else reads
// it, so the lane that re-reads 8 consecutive bf16 columns of a row from the patch quantises them instead of storing them: the
// 32-column MX block of a row is the aligned lane quad (chunks ch & ~3 .. + 3 of one row: lanes 4 k .. 4 k + 3, since a row
// has 8 or 16 chunks), |max| over the quad by two cross-lane moves (quad_amax, no LDS), then mx_quant8 -- the standalone
// quantiser's lane shape and its arithmetic, on the bf16 value in the patch: byte for byte bya_attn_kv_mix followed by
// bya_quantize_mx on the [rows, heads * D] matrix, which is never written.  All 64 lanes take part in the |max| (rows past Sq
// hold the clamped row's values, whole quads of them, and store nothing).  The format is a wave-uniform branch.
//
// SEG = true (bya_attn_kv_mix_seg / _mx_seg): what a workgroup's "group" is -- which K / V block, where its rows start in q / r /
// z / wsum / the MX pair, how many there are -- comes from entry blockIdx / (heads * nqt) of `seg` instead of one uniform Sq, and
// nqt is the chunk count of the LONGEST segment: a workgroup whose share of its segment's tiles is empty leaves before it stages
// anything (uniform over the workgroup, so the one barrier stays legal).  Everything below those few lines is the same code:
// a row's arithmetic does not know which form runs, and a tile's padding lanes repeat the last row of their OWN segment, as in
// the one-launch-per-segment form this replaces.
template <int D, bool MX = false, bool SEG = false>
__device__ __forceinline__ void attn_mix32_body(const MixArgs& p, char* smem, const ByaMixMxOut* mx = nullptr,
                                                const bya_attn_mix_segments* seg = nullptr) {
    constexpr int ROW_BYTES = D * 2, KV_BYTES = 32 * ROW_BYTES, DSTEPS = D / 16, DT = D / 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hf = lane >> 5;
    int bid = blockIdx.x;
    const int head = bid % p.heads; bid /= p.heads;
    const int chunk = bid % p.nqt;                               // nqt = row chunks per (group, head) in this form
    const int grp = bid / p.nqt;                                 // (SEG: the segment)
    // the workgroup's rows: Sq of them against K / V group kgrp; the first is row row0 of r and wsum, q_off / z_off elements
    // into q / z and c_off / s_off bytes into the MX pair
    int kgrp = grp, Sq = p.Sq;
    long long row0 = (long long)grp * p.Sq, q_off = grp * p.q_grp, z_off = 0, c_off = 0, s_off = 0;
    if constexpr (SEG) {
        kgrp = seg->grp[grp]; Sq = seg->len[grp]; row0 = seg->start[grp];
        q_off = row0 * p.q_row;
        if constexpr (MX) { c_off = row0 * mx->c_row; s_off = row0 * mx->s_row; }
        else z_off = row0 * p.z_row;
    } else {
        if constexpr (MX) { c_off = grp * mx->c_grp; s_off = grp * mx->s_grp; }
        else z_off = grp * p.z_grp;
    }
    const int n32 = (Sq + 31) >> 5;
    const int t0 = (int)((long long)n32 * chunk / p.nqt), t1 = (int)((long long)n32 * (chunk + 1) / p.nqt);
    if constexpr (SEG) if (t0 >= t1) return;                     // a segment shorter than the longest one's chunk count
    const bf16_t* Q = p.q + q_off + (long long)head * D;
    bf16_t* Z = nullptr;
    if constexpr (!MX) Z = p.z + z_off + (long long)head * D;

    for (int id = 0; id < p.n_id; ++id) {
        stage_kv32<D>(p.k + id * p.k_id + kgrp * p.k_grp + (long long)head * D, p.k_row, p.Skv - 1, smem + id * 2 * KV_BYTES,
                      wave, lane, false);
        stage_kv32<D>(p.v + id * p.v_id + kgrp * p.v_grp + (long long)head * D, p.v_row, p.Skv - 1,
                      smem + id * 2 * KV_BYTES + KV_BYTES, wave, lane, true);
    }
    const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
    uint32_t voff[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        const int row = 4 * hf + tq;
        const int ch = 4 * d + 2 * (g & 1) + (tp >> 1);
        voff[d] = row * ROW_BYTES + ((ch ^ vswz<D>(row)) << 4) + (tp & 1) * 8;
    }
    const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
    uint32_t koff[DSTEPS];
#pragma unroll
    for (int s = 0; s < DSTEPS; ++s) koff[s] = r * ROW_BYTES + (((2 * s + hf) ^ kswz<D>(r)) << 4);
    const float c = p.scale_log2;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                             // K / V of every identity are in LDS; no barrier below

    // (measured and dropped: q as whole head segments by LDS-DMA into the wave's patch + ds_read_b128 fragments -- audio
    // level, face 42 -> 49 us; q requested one tile ahead in registers -- +35 registers, one wave per SIMD less, level)
    for (int t = t0 + wave; t < t1; t += 4) {
        int qrow = t * 32 + r;
        const bool q_valid = qrow < Sq;
        qrow = q_valid ? qrow : Sq - 1;
        bf16x8 qf[DSTEPS];
#pragma unroll
        for (int s = 0; s < DSTEPS; ++s)
            qf[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Q + (long long)qrow * p.q_row + s * 16 + hf * 8));
        float w[4];
        routing_weights_of(p.mode, p.n_id, p.af, p.r + (row0 + qrow) * p.n_id, w);
        if (p.wsum && head == 0 && hf == 0 && q_valid) {
            float ws = 0.f;
            for (int i = 0; i < p.n_id; ++i) ws += w[i];
            p.wsum[row0 + qrow] = ws;
        }
        char* zb = smem + p.n_id * 2 * KV_BYTES + wave * KV_BYTES;
        constexpr int CHUNKS = ROW_BYTES / 16;
        f32x16 zacc[DT];
        for (int id = 0; id < p.n_id; ++id) {
            const uint32_t kb = lds0 + id * 2 * KV_BYTES, vb = kb + KV_BYTES;
            // S^T = K . Q^T (32 keys x 32 queries): lane (q = r, hf) gets keys (i & 3) + 8 (i >> 2) + 4 hf
            bf16x8 kf[DSTEPS];
#pragma unroll
            for (int s = 0; s < DSTEPS; ++s) kf[s] = lds_read128<0>(kb + koff[s]);
            f32x16 sacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
            lgkm_wait<0>();
#pragma unroll
            for (int s = 0; s < DSTEPS; ++s) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[s], sacc, 0, 0, 0);
            // the V fragments fly under the softmax
            VFrag<D> fa, fb;
            uint32_t vbase[DT];
#pragma unroll
            for (int d = 0; d < DT; ++d) vbase[d] = vb + voff[d];
            v_issue<D, 0>(fa, vbase);
            v_issue<D, 1>(fb, vbase);
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kv = (i & 3) + 8 * (i >> 2) + 4 * hf;
                if (kv >= p.Skv) sacc[i] = -INFINITY;
                mx = fmaxf(mx, sacc[i]);
            }
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
                mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            }
            // the reference point attn_tile takes on a first tile: the maximum as a two-term bf16 value
            const float m_hi = bf2f(f2bf(mx));
            const float m_lo = bf2f(f2bf(mx - m_hi));
            const float m_new = m_hi + m_lo;
            float psum = 0.f;
            bf16x8 pf[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pv = __builtin_amdgcn_exp2f((sacc[tt * 8 + e] - m_new) * c);
                    psum += pv;
                    pf[tt][e] = (__bf16)pv;
                }
            const auto lsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(psum), __float_as_uint(psum), false, false);
            const float sc = w[id] / (__uint_as_float(lsw[0]) + __uint_as_float(lsw[1]));
            f32x16 oacc[DT];
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[d][i] = 0.f;
            lgkm_wait<2 * DT>();
            pv_mfma<D>(fa, pf[0], oacc);
            lgkm_wait<0>();
            pv_mfma<D>(fb, pf[1], oacc);
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) zacc[d][i] = id == 0 ? fmaf(sc, oacc[d][i], 0.f) : fmaf(sc, oacc[d][i], zacc[d][i]);
        }
        // ---- z through this wave's LDS patch, stored as WHOLE head segments: a lane holds 8-byte pieces of its row (d = 32 dt
        // + 8 gq + 4 hf ..+3); stored as they stand that is 8 DT instructions each touching 32 rows with 16 bytes -- sixteen
        // partial-line requests per 128-byte segment.  Re-read row-major, 16 bytes per lane: every request a full line.
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                u32x2 o;
                o[0] = pack2bf(zacc[d][gq * 4 + 0], zacc[d][gq * 4 + 1]);
                o[1] = pack2bf(zacc[d][gq * 4 + 2], zacc[d][gq * 4 + 3]);
                *reinterpret_cast<u32x2*>(zb + r * ROW_BYTES + (((4 * d + gq) ^ (r & 7)) << 4) + 8 * hf) = o;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if constexpr (MX) {
            // (not unrolled: one copy of the two quantisers per kernel -- the walk is store-bound, and the translation unit's
            // count of packed-fp32 instructions, which tests/test_abi_cpu.py watches, stays where it was)
#pragma nounroll
            for (int j = 0; j < 32 * CHUNKS / 64; ++j) {
                const int idx = j * 64 + lane, row = idx / CHUNKS, ch = idx % CHUNKS;
                float v[8];
                unpack8(*reinterpret_cast<const u32x4*>(zb + row * ROW_BYTES + ((ch ^ (row & 7)) << 4)), v);
                float amax = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(v[e]));
                amax = quad_amax(amax);
                if (t * 32 + row < Sq) {
                    const long long grow = t * 32 + row;
                    uint8_t* crow = mx->codes + c_off + grow * mx->c_row;
                    uint32_t sb;
                    if (mx->fmt == MX_E4M3) sb = mx_quant8<MX_E4M3>(v, amax, crow + head * D + 8 * ch);
                    else sb = mx_quant8<MX_E2M3>(v, amax, crow + head * (D * 3 / 4) + 6 * ch);
                    if ((ch & 3) == 0) mx->scales[s_off + grow * mx->s_row + head * (D / 32) + (ch >> 2)] = (uint8_t)sb;
                }
            }
        } else {
#pragma unroll
        for (int j = 0; j < 32 * CHUNKS / 64; ++j) {
            const int idx = j * 64 + lane, row = idx / CHUNKS, ch = idx % CHUNKS;
            const u32x4 o = *reinterpret_cast<const u32x4*>(zb + row * ROW_BYTES + ((ch ^ (row & 7)) << 4));
            if (t * 32 + row < Sq) *reinterpret_cast<u32x4*>(Z + (long long)(t * 32 + row) * p.z_row + ch * 8) = o;
        }
        }
        __builtin_amdgcn_wave_barrier();                         // the patch is rewritten by the next tile
    }
}

}  // namespace

// defined in attn_mix_mx.hip: the launch of the MX-output instances of the <= 32-key form for checked arguments (q .. wsum and
// desc as for bya_attn_kv_mix, plan = its launch decisions, out = where the codes and scale bytes go, seg = NULL or the checked
// table of the segment instance, batch = NULL or the checked sample strides of the batch instance -- never both; plan.grid is
// then the grid of ONE sample); called from bya_attn_kv_mix_mx, bya_attn_kv_mix_mx_seg and bya_attn_kv_mix_mx_batch
int bya_launch_attn_kv_mix32_mx(const void* q, const void* k, const void* v, const void* r, const void* af, float* wsum,
                                const bya_attn_mix_desc& desc, const bya_attn_kv_mix_plan_info& plan, const ByaMixMxOut& out,
                                const bya_attn_mix_segments* seg, const ByaMixSampleStrides* batch, hipStream_t stream);
// defined in attn_mix_seg.hip: the launch of the bf16 segment instance for checked arguments; called from bya_attn_kv_mix_seg
int bya_launch_attn_kv_mix32_seg(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                                 const bya_attn_mix_desc& desc, const bya_attn_kv_mix_plan_info& plan,
                                 const bya_attn_mix_segments& seg, hipStream_t stream);
// defined in attn_mix_batch.hip: the launch of the bf16 batch instances for checked arguments (plan.grid = the grid of ONE sample,
// batch = the checked sample strides); called from bya_attn_kv_mix_batch
int bya_launch_attn_kv_mix32_batch(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                                   const bya_attn_mix_desc& desc, const bya_attn_kv_mix_plan_info& plan,
                                   const ByaMixSampleStrides& batch, hipStream_t stream);
