// Shared by the GEMM translation units (gemm.hip, gemm_v4 / v5 / v6.hip, gemm_fp8.hip, gemm_fp8_v4.hip, gemm_fp8_v4_qkn.hip,
// gemm_fp8_v4_qkn_stats.hip, gemm_mx.hip, gemm_mx_v4.hip) and the implicit-GEMM convolution (vae.hip): argument block, fused
// epilogue, LDS read helper, and the host side every GEMM entry point shares -- descriptor -> GemmArgs, the epilogue-side
// checks, the row cut, the plan fill.
#pragma once
#include "bya_common.h"
#include "../../include/bya.h"

namespace {

struct GemmArgs {
    const bf16_t* A; const bf16_t* W; const bf16_t* bias; bf16_t* C; const bf16_t* res;
    const bf16_t* gate0; const bf16_t* gate1;
    int M, N, K;
    int lda, ldw, ldc, ldres;
    long long a_bs, c_bs, res_bs, gate_bs;
    int gate_split;
    int act;
    float leaky;
    int n_split;            // > 0: output column n goes to C + (n / n_split) * c_split_stride, column n % n_split
    long long c_split_stride;
    const float* bias_rowscale;   // optional fp32 [batch*M]: bias is multiplied by bias_rowscale[z*M + m]
    float alpha;                  // scales (acc + bias) after the activation (local_face_scale)
    // split-K workspace of the persistent kernel (gemm_v4.hip; bya_set_gemm_workspace): 256 slabs of 256 x 256 fp32 behind
    // 1024 counters; null = the last, partial round of tiles is not split
    float* ws_slabs;
    unsigned* ws_counters;
    int gm = 4;                   // persistent kernel: group-M width of the tile order (gemm_v4.hip; chosen per shape by its launchers)
    // Implicit-GEMM 3 x 3 x 3 convolution on the persistent kernel (bya_vae_conv3d; gemm_v4.hip, CONV instance): A is the
    // zero-padded channels-last input [To + 2, Hp, Wp, C] seen as a matrix of pixels x C (lda = C), row m of the product is
    // the padded pixel m of the OUTPUT grid [To, Hp, Wp] (rows with h >= H or w >= W are computed and dropped), K-tile t is
    // the 64-channel group t % cpg of tap t / cpg = (dt, dh, dw): the same rows, ((dt Hp + dh) Wp + dw) pixels further on.
    // q/k LayerNorm(64) + RoPE in the packed q|k|v projection's epilogue (bya_gemm_qkv_norm_rope; gemm_v4.hip, QKN instance):
    // columns [0, qkn_width) are q, [qkn_width, 2 qkn_width) k, the rest v (untouched); per 64-column head row the arithmetic
    // of qknorm_math.h on the bf16-ROUNDED projection (what the two-launch path reads back), rows >= qkn_text_rows rotated
    const bf16_t* qkn_w[2] = {nullptr, nullptr};
    const bf16_t* qkn_b[2] = {nullptr, nullptr};
    const float* qkn_cos = nullptr; const float* qkn_sin = nullptr;
    int qkn_text_rows = 0, qkn_width = 0;
    float qkn_eps = 0.f, qkn_kscale = 1.f;
    int conv_cpg_log2 = -1;            // log2(C / 64); < 0: plain GEMM
    int conv_Hp = 0, conv_Wp = 0, conv_H = 0, conv_W = 0, conv_To = 0;
    long long conv_a_bytes = 0;        // bytes of the padded input from A on (reads past it return zeros)
    // the q/k-norm epilogue's score-bound statistics (the *_stats entry points; STATS instances only; at the end, so that every
    // other field keeps its place in the kernels' argument block): fp32 [qkn_stats_slots][2][qkn_stats_nbh], entry
    // z * (qkn_width / 64) + head of the tensor (qkn_stats_args)
    float* qkn_stats = nullptr;
    int qkn_stats_slots = 0, qkn_stats_nbh = 0;
};

constexpr size_t GEMM_WS_COUNTER_BYTES = 4096, GEMM_WS_SLAB_BYTES = 256 * 256 * 4, GEMM_WS_SLABS = 256;
constexpr size_t GEMM_WS_BYTES = GEMM_WS_COUNTER_BYTES + GEMM_WS_SLABS * GEMM_WS_SLAB_BYTES;

constexpr int BK = 64;  // bf16 elements per K tile = 128-byte LDS rows

template <int V> struct IntTag { static constexpr int value = V; };

// The pipelined 256x256 kernels instantiate their (fully unrolled, 128-accumulator) epilogue for these activations only --
// none, GELU(tanh) of the DiT MLP and its A/B twin; every other activation sits on small GEMMs that run on the 128x128
// kernel (pick_tile), so seven copies of a 3000-line epilogue are not carried around (they also cost registers: the
// seven-way merge made hipcc copy half the accumulators).
__host__ __device__ constexpr bool act_on_big_tiles(int act) { return act == 0 || act == 1 || act == 6; }
template <typename F>
__device__ __forceinline__ void dispatch_act_big(int act, F&& f) {
    switch (act) {
        case 1: f(IntTag<1>{}); break;
        case 6: f(IntTag<6>{}); break;
        default: f(IntTag<0>{}); break;
    }
}

template <int ACT>
__device__ __forceinline__ float apply_act(float v, float leaky) {
    if constexpr (ACT == 1) return gelu_tanh(v);
    else if constexpr (ACT == 2) return gelu_erf(v);
    else if constexpr (ACT == 3) return v > 0.f ? v : 0.f;
    else if constexpr (ACT == 4) return silu(v);
    else if constexpr (ACT == 5) return v > 0.f ? v : v * leaky;
    else if constexpr (ACT == 6) return gelu_tanh_ieee(v);
    else return v;
}


// Epilogue for 4 consecutive output columns n4..n4+3 of row m: + bias -> act -> * gate[row type] -> + residual -> bf16
template <typename F>
__device__ __forceinline__ void dispatch_act(int act, F&& f) {
    switch (act) {
        case 1: f(IntTag<1>{}); break;
        case 2: f(IntTag<2>{}); break;
        case 3: f(IntTag<3>{}); break;
        case 4: f(IntTag<4>{}); break;
        case 5: f(IntTag<5>{}); break;
        case 6: f(IntTag<6>{}); break;
        default: f(IntTag<0>{}); break;
    }
}

// Fused epilogue of one wave: the lane holds C[m_j][n_i .. n_i + 3] for m_j = m_base + 16 j, n_i = n_base + 16 i
// (the transposed 16x16x32 accumulator layout of every GEMM kernel here), acc[i][j] = the four columns.
//   v = alpha * act(acc + rowscale[m] * bias[n]);  v *= gate[row type][n];  v += res[m][n];  C[m][n] = bf16(v)
// Everything the epilogue READS (bias, both gate vectors, the residual rows, the per-row bias scale) is requested up front
// in one burst, with clamped addresses instead of branches, and only then consumed: a load inside the per-tile bounds
// branch made hipcc wait for it -- and, since vmcnt counts stores too, for the previous tile's store -- once per
// 16x16 tile, 32 to 64 serialized memory round trips per wave (measured: the gate + residual epilogue cost 32 % of the
// attention-output GEMM, 780 vs 1152 TFLOP/s).  The residual may alias C (x += ...): a lane only ever reads the
// elements it later writes.
template <int ACT, int NI, int NJ, int IB = NI>
__device__ __forceinline__ void epilogue_block(const GemmArgs& p, int z, int m_base, int n_base, const f32x4 (&acc)[NI][NJ]) {
    // IB = column groups per burst: the burst's residual values occupy IB * NJ * 2 registers (the 8-wave kernel has only
    // 256 registers per lane with 128 of them accumulators, so it bursts one column group at a time).
    // Residual loads and C stores go through buffer descriptors: 32-bit per-lane byte offsets (one register per row, no
    // 64-bit pointer per access) and the hardware range check instead of branches -- an element outside M x N gets the
    // offset 0xffffffff, whose load returns zero and whose store is dropped.  The descriptors reach 2 GiB from their base:
    // the host side (gemm_row_chunks below) cuts a launch whose C or residual rows span more than that into row chunks.
    static_assert(NI % IB == 0, "burst size must divide the tile");
    const bool has_res = p.res != nullptr, has_gate = p.gate0 != nullptr, has_bias = p.bias != nullptr;
    const bool has_rs = p.bias_rowscale != nullptr;
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((has_res ? p.res : p.C) + (long long)z * p.res_bs), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(p.C + (long long)z * p.c_bs), 0, 0x7fffffff, 0x00020000);
    const char* g0base = reinterpret_cast<const char*>(p.gate0 + (long long)z * p.gate_bs);
    const char* g1base = reinterpret_cast<const char*>(p.gate1 + (long long)z * p.gate_bs);
    float rs[NJ];
    bool mok[NJ];
    uint32_t roff[NJ], coff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int m = m_base + 16 * j;
        mok[j] = m < p.M;
        const uint32_t mc = mok[j] ? (uint32_t)m : 0u;
        rs[j] = has_rs ? p.bias_rowscale[(long long)z * p.M + mc] : 1.0f;
        roff[j] = mok[j] ? mc * (uint32_t)(p.ldres * 2) : 0xffffffffu;
        coff[j] = mok[j] ? mc * (uint32_t)(p.ldc * 2) : 0xffffffffu;
    }
#pragma unroll
    for (int ib = 0; ib < NI; ib += IB) {
        u32x2 bv[IB], g0[IB], g1[IB], rv[IB][NJ];
        bool nok[IB];
        uint32_t ncb[IB];
#pragma unroll
        for (int ii = 0; ii < IB; ++ii) {
            const int n4 = n_base + 16 * (ib + ii);
            nok[ii] = n4 < p.N;
            ncb[ii] = nok[ii] ? (uint32_t)n4 * 2u : 0u;
            bv[ii] = has_bias ? *reinterpret_cast<const u32x2*>(reinterpret_cast<const char*>(p.bias) + ncb[ii]) : u32x2{0u, 0u};
            if (has_gate) {
                g0[ii] = *reinterpret_cast<const u32x2*>(g0base + ncb[ii]);
                g1[ii] = *reinterpret_cast<const u32x2*>(g1base + ncb[ii]);
            }
            if (has_res) {
#pragma unroll
                for (int j = 0; j < NJ; ++j)       // (0xffffffff + a column offset wraps: clamp invalid rows explicitly)
                    rv[ii][j] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(
                        rsR, mok[j] ? roff[j] + ncb[ii] : 0xffffffffu, 0, 0));
            }
        }
#pragma unroll
        for (int ii = 0; ii < IB; ++ii) {
            const int n4 = n_base + 16 * (ib + ii);
            uint32_t colb = (uint32_t)n4 * 2u;
            if (p.n_split > 0) colb = ((uint32_t)(n4 / p.n_split) * (uint32_t)p.c_split_stride + (uint32_t)(n4 % p.n_split)) * 2u;
            const float b4[4] = {bflo(bv[ii][0]), bfhi(bv[ii][0]), bflo(bv[ii][1]), bfhi(bv[ii][1])};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int m = m_base + 16 * j;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v[e] = p.alpha * apply_act<ACT>(fmaf(rs[j], b4[e], acc[ib + ii][j][e]), p.leaky);
                if (has_gate) {
                    const u32x2 gv = m < p.gate_split ? g0[ii] : g1[ii];
                    v[0] *= bflo(gv[0]); v[1] *= bfhi(gv[0]); v[2] *= bflo(gv[1]); v[3] *= bfhi(gv[1]);
                }
                if (has_res) {
                    v[0] += bflo(rv[ii][j][0]); v[1] += bfhi(rv[ii][j][0]);
                    v[2] += bflo(rv[ii][j][1]); v[3] += bfhi(rv[ii][j][1]);
                }
                u32x2 o;
                o[0] = pack2bf(v[0], v[1]);
                o[1] = pack2bf(v[2], v[3]);
                __builtin_amdgcn_raw_buffer_store_b64(o, rsC, (mok[j] && nok[ii]) ? coff[j] + colb : 0xffffffffu, 0, 0);
            }
        }
    }
}

// 16 bytes of LDS into a 16-byte register tuple (bf16x8 fragments, the i32x4 halves of an e4m3 fragment)
template <int OFF, typename T>
__device__ __forceinline__ void ds_read128(T& dst, uint32_t addr) {
    static_assert(sizeof(T) == 16, "one ds_read_b128");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(OFF));
}

// ---- host side: the 2 GiB reach of the epilogue's buffer descriptors ---------------------------------------------------
// Every epilogue here addresses C and the residual as  base(z) + 32-bit byte offset  under num_records = 0x7fffffff: an
// element whose byte offset reaches 2^31 - 1 would be silently dropped on store and read as zero (and offsets past 4 GiB
// would wrap onto valid rows).  97 frames at 720 x 1280 are 90226 joint rows: the MLP's [90226, 12288] bf16 activation is
// 2.2 GB.  Such a launch is cut into row chunks (and batch entries) that each stay inside the reach (gemm_row_chunks); `run(args,
// batch, row0)` launches one piece, row0 = index of its first row in per-row side arrays ([batch * M] fp32 scales).
inline long long gemm_span_bytes(const GemmArgs& a, int M, bool res) {
    const long long ld = res ? a.ldres : a.ldc;
    const long long col = (!res && a.n_split > 0) ? (long long)(a.N / a.n_split - 1) * a.c_split_stride + a.n_split - 1
                                                  : (long long)a.N - 1;
    return ((long long)(M - 1) * ld + col) * 2 + 16;          // + the widest access of any epilogue
}

inline bool gemm_rows_reachable(const GemmArgs& a, int M) {
    constexpr long long REACH = 0x7fffffffLL;
    return gemm_span_bytes(a, M, false) < REACH && (!a.res || gemm_span_bytes(a, M, true) < REACH);
}

// rows per chunk: a.M when the whole launch is in reach, 0 when not even one 256-row block is (strides too large)
inline int gemm_chunk_rows(const GemmArgs& a) {
    if (gemm_rows_reachable(a, a.M)) return a.M;
    int chunk = a.M;
    while (chunk > 256 && !gemm_rows_reachable(a, chunk)) chunk = ((chunk / 2 + 255) / 256) * 256;
    return gemm_rows_reachable(a, chunk) ? chunk : 0;
}

// The piece of launch `a` that starts at row m0 of batch entry z and has `rows` rows, as a launch of batch 1 (z = 0: of a's batch):
// every per-row and per-batch-entry base moves there -- A (a_elem_bytes per element: 2 for bf16, 1 for fp8 / MX codes), C, the
// residual, the per-row bias scale, both gate vectors -- and what counts rows from the launch's first one (gate_split, the
// q/k-norm epilogue's text rows and its rotary table, whose row of token m is m - text_rows) is re-based on m0.  Null pointers
// stay null (a null gate1 means one gate for every row).
inline GemmArgs gemm_rows(const GemmArgs& a, int z, int m0, int rows, int a_elem_bytes) {
    GemmArgs s = a;
    s.M = rows;
    s.A = reinterpret_cast<const bf16_t*>(reinterpret_cast<const char*>(a.A) +
                                          ((long long)z * a.a_bs + (long long)m0 * a.lda) * a_elem_bytes);
    s.C = a.C + (long long)z * a.c_bs + (long long)m0 * a.ldc;
    if (a.res) s.res = a.res + (long long)z * a.res_bs + (long long)m0 * a.ldres;
    if (a.gate0) s.gate0 = a.gate0 + (long long)z * a.gate_bs;
    if (a.gate1) s.gate1 = a.gate1 + (long long)z * a.gate_bs;
    if (a.bias_rowscale) s.bias_rowscale = a.bias_rowscale + (long long)z * a.M + m0;
    s.gate_split = a.gate_split > m0 ? a.gate_split - m0 : 0;
    s.qkn_text_rows = a.qkn_text_rows > m0 ? a.qkn_text_rows - m0 : 0;
    if (a.qkn_cos && m0 > a.qkn_text_rows) {
        s.qkn_cos = a.qkn_cos + (long long)(m0 - a.qkn_text_rows) * 64;
        s.qkn_sin = a.qkn_sin + (long long)(m0 - a.qkn_text_rows) * 64;
    }
    return s;
}

// A plan (include/bya.h bya_gemm_plan) of a whole launch on one path: no row split, no split-K
inline int gemm_plan_whole(bya_gemm_plan* p, int path, int row_chunks) {
    p->path = path; p->m0 = 0; p->tail = -1; p->split_k = 0; p->row_chunks = row_chunks;
    return BYA_OK;
}

// run(piece, batch, row0) for every piece of `a`.  A plan query (plan != nullptr; `run` then fills *plan instead of launching)
// sees the first piece only, which stands for all of them, and gets their number.
template <typename F>
int gemm_row_chunks(const GemmArgs& a, int batch, int a_elem_bytes, bya_gemm_plan* plan, F&& run) {
    const int chunk = gemm_chunk_rows(a);
    if (chunk == a.M) return run(a, batch, 0LL);
    if (chunk == 0) return BYA_ERR_UNSUPPORTED;        // a single 256-row block out of reach: strides too large
    for (int z = 0; z < batch; ++z)
        for (int m0 = 0; m0 < a.M; m0 += chunk) {
            const int rc = run(gemm_rows(a, z, m0, a.M - m0 < chunk ? a.M - m0 : chunk, a_elem_bytes), 1, (long long)z * a.M + m0);
            if (rc != BYA_OK) return rc;
            if (plan) {
                plan->row_chunks = batch * ((a.M + chunk - 1) / chunk);
                return BYA_OK;
            }
        }
    return BYA_OK;
}

// ---- host side: bya_gemm_desc -> GemmArgs.  The ONE place that copies a descriptor: a null gate1 means gate0 for every row,
// alpha 0 means 1, no split-K workspace (bya_gemm_bf16 installs its device's afterwards).
inline void gemm_fill_args(const void* A, const void* W, const void* bias, const void* C, const void* res, const void* gate0,
                           const void* gate1, const bya_gemm_desc* d, GemmArgs* out) {
    GemmArgs& a = *out;
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.bias = (const bf16_t*)bias; a.C = (bf16_t*)C;
    a.res = (const bf16_t*)res; a.gate0 = (const bf16_t*)gate0; a.gate1 = (const bf16_t*)(gate1 ? gate1 : gate0);
    a.M = d->M; a.N = d->N; a.K = d->K;
    a.lda = d->lda; a.ldw = d->ldw; a.ldc = d->ldc; a.ldres = d->ldres;
    a.a_bs = d->a_batch_stride; a.c_bs = d->c_batch_stride; a.res_bs = d->res_batch_stride;
    a.gate_bs = d->gate_batch_stride; a.gate_split = d->gate_split; a.act = d->act; a.leaky = 0.01f;
    a.n_split = d->n_split; a.c_split_stride = d->c_split_stride;
    a.bias_rowscale = d->bias_rowscale; a.alpha = d->alpha == 0.0f ? 1.0f : d->alpha;
    a.ws_counters = nullptr; a.ws_slabs = nullptr;
}

// ... and the epilogue side of the checks in front of it, behind the operand side's own (K tile, lda / ldw, A / W / scale
// pointers: by format): 8-byte epilogue accesses (BYA_ERR_ALIGN), the activation (act_ok: the format's kernels have it;
// BYA_ERR_UNSUPPORTED), the column split (BYA_ERR_SHAPE) -- in the order callers have always seen.
inline int gemm_epilogue_check(const void* C, const void* res, const void* bias, const void* gate0, const void* gate1,
                               const bya_gemm_desc* d, bool act_ok) {
    if (d->ldc % 4 || (res && d->ldres % 4)) return BYA_ERR_ALIGN;
    if (((uintptr_t)C | (uintptr_t)res | (uintptr_t)bias | (uintptr_t)gate0 | (uintptr_t)gate1) & 7) return BYA_ERR_ALIGN;
    if (!act_ok) return BYA_ERR_UNSUPPORTED;
    if (d->n_split < 0 || (d->n_split > 0 && (d->n_split % 4 || d->c_split_stride % 4 || res))) return BYA_ERR_SHAPE;
    return BYA_OK;
}

// ---- host side: the q/k-norm epilogue's arguments on the tiled / wide kernels that decide q, k or v per 64-column head
// (bya_gemm_mx_qkv_norm_rope, bya_gemm_fp8_qkv_norm_rope).  Two steps around the operand family's own argument function:
// qkn_norm_desc_check before it (a malformed norm descriptor: BYA_ERR_SHAPE), qkn_head_args behind it -- BYA_ERR_UNSUPPORTED:
// not this epilogue's shape (the caller keeps its GEMM + bya_qknorm_rope), BYA_ERR_ALIGN, else GemmArgs::qkn_* filled.
inline int qkn_norm_desc_check(const bya_gemm_desc* d, const bya_qknorm_desc* n) {
    if (!d || !n) return BYA_ERR_SHAPE;
    if (!n->qw || !n->qb || !n->kw || !n->kb || n->width <= 0 || n->text_rows < 0) return BYA_ERR_SHAPE;
    if (d->M > 0 && n->text_rows < d->M && (!n->cos || !n->sin)) return BYA_ERR_SHAPE;
    return BYA_OK;
}

// The score-bound statistics a fused q/k-norm launch is asked to record (the *_stats entry points of include/bya.h; the plain
// entry points pass none): bya_qknorm_rope's table and its slot count.
struct QknStats { float* stats = nullptr; int32_t slots = 0; };
// ... its own checks, before anything else looks at the launch: the slot count (BYA_ERR_SHAPE), the table's 4 bytes (BYA_ERR_ALIGN)
inline int qkn_stats_check(const QknStats& s) {
    if (s.stats && (s.slots < 1 || s.slots > 64)) return BYA_ERR_SHAPE;
    return ((uintptr_t)s.stats & 3) ? BYA_ERR_ALIGN : BYA_OK;
}
// QknStats -> GemmArgs::qkn_stats* (behind qkn_fill_norm and the entry point's own checks).  The table's entry of a head is the one the two-launch path's bya_qknorm_rope call raises:
// dense (n_split == width) z * heads + head; column blocks of whole heads with one batch entry (the head-parallel sharded
// step: its bya_qknorm_rope runs over [blocks, rows, n_split] with heads-per-block heads) the global head -- the same formula
// with z = 0.  Anything else is not a launch whose table this epilogue knows: BYA_ERR_UNSUPPORTED.
inline int qkn_stats_args(const bya_gemm_desc* d, const bya_qknorm_desc* n, const QknStats& s, GemmArgs* out) {
    if (!s.stats) return BYA_OK;
    const bool dense = d->n_split == n->width;
    const bool blocks = d->n_split > 0 && d->n_split < n->width && n->width % d->n_split == 0 && d->n_split % 64 == 0 && d->batch == 1;
    if (!dense && !blocks) return BYA_ERR_UNSUPPORTED;
    out->qkn_stats = s.stats; out->qkn_stats_slots = s.slots; out->qkn_stats_nbh = d->batch * (n->width / 64);
    return BYA_OK;
}

// bya_qknorm_desc -> GemmArgs::qkn_* (k_scale 0 means 1)
inline void qkn_fill_norm(const bya_qknorm_desc* n, GemmArgs* out) {
    GemmArgs& a = *out;
    a.qkn_w[0] = (const bf16_t*)n->qw; a.qkn_b[0] = (const bf16_t*)n->qb; a.qkn_w[1] = (const bf16_t*)n->kw; a.qkn_b[1] = (const bf16_t*)n->kb;
    a.qkn_cos = n->cos; a.qkn_sin = n->sin; a.qkn_text_rows = n->text_rows; a.qkn_width = n->width;
    a.qkn_eps = n->eps; a.qkn_kscale = n->k_scale == 0.0f ? 1.0f : n->k_scale;
}

inline int qkn_head_args(const void* C, const bya_gemm_desc* d, const bya_qknorm_desc* n, const QknStats& s, GemmArgs* out) {
    if ((d->N != 3 * n->width && d->N != 2 * n->width) || n->width % 64 != 0 || d->n_split <= 0 || d->act != 0 ||
        d->bias_rowscale || (d->alpha != 0.0f && d->alpha != 1.0f))
        return BYA_ERR_UNSUPPORTED;
    // eight consecutive columns leave as one 16-byte store
    if (d->n_split % 8 || d->c_split_stride % 8 || d->ldc % 8 || d->c_batch_stride % 8) return BYA_ERR_ALIGN;
    if (((uintptr_t)C | (uintptr_t)n->qw | (uintptr_t)n->qb | (uintptr_t)n->kw | (uintptr_t)n->kb | (uintptr_t)n->cos |
         (uintptr_t)n->sin) & 15) return BYA_ERR_ALIGN;
    GemmArgs& a = *out;
    a.act = 0; a.alpha = 1.0f; a.bias_rowscale = nullptr;
    qkn_fill_norm(n, out);
    // one launch: its rows and its rotary rows within the 2 GiB reach of the buffer descriptors
    if (!gemm_rows_reachable(a, a.M) || ((long long)a.M - a.qkn_text_rows) * 256 >= 0x7fffffffLL) return BYA_ERR_UNSUPPORTED;
    return qkn_stats_args(d, n, s, out);   // (which kernel path records them: the entry point, once it knows the path)
}

// Persistent kernels: group-M width of the tile order, in 256-row tiles, by shape: a long K sweep wants few row tiles per group
// (the W panel of a column tile is re-read by fewer row tiles, but each stays in flight longer), wide outputs want more
// (same-box sweep: tools/gemm_gm_probe.py, profiles/r6_k_gemm_gm_probe.json)
inline int gemm_group_m(const GemmArgs& a) { return a.K >= 8192 ? 2 : (a.N >= 8192 ? 8 : 4); }

}  // namespace

// defined in gemm_v4.hip (compiled with its own register-allocation flags: accumulators in AGPRs), called from
// bya_gemm_bf16: persistent one-wave-per-SIMD kernel with cross-tile prefetch and 16-byte epilogue accesses
int bya_launch_gemm256p(const void* args, int batch, hipStream_t stream);
int bya_launch_gemm256p_qkn(const void* args, int batch, hipStream_t stream);    // ... its QKN instance (bya_gemm_qkv_norm_rope)
int bya_gemm_split_min_ktiles();     // K-tiles per K-range below which the persistent kernel does not split a tile
int bya_gemm256p_split(const void* args, int batch);   // does bya_launch_gemm256p cut its last round along K?  0, 1 or 2
// defined in gemm_v5.hip: the persistent kernel with 128 x 256 tiles (three-stage ring) for row counts that leave the 256 x 256
// grid half empty; callers have checked v4_eligible() and K >= 4 K-tiles
int bya_launch_gemm128p(const void* args, int batch, hipStream_t stream);
int bya_launch_gemm128p_qkn(const void* args, int batch, hipStream_t stream);
// defined in gemm_v6.hip: the same tile with loader waves (the compute waves issue no vector-memory instruction in the K-loop)
int bya_launch_gemm128s(const void* args, int batch, hipStream_t stream);
