/*
 * bya.h -- C ABI of libbya_hip.so: the hand-written gfx950 (MI355X / CDNA4) kernels under the
 * Bind-Your-Avatar per-denoise-step hot path.
 *
 * The reference (Yubo-Shankui/Bind-Your-Avatar-Implementation) is pure Python: its hot path is
 * `BindyouravatarTransformer3DModel.forward` (models/transformer.py:615-964), called once per step by
 * `BindyouravatarPipeline.__call__` (models/pipeline_bindyouravatar.py:910-923).  It has no FFI of its
 * own; every op is a PyTorch dispatch.  This header is therefore the boundary a maintainer binds
 * (ctypes stub in INTEGRATION.md) and each entry point cites the reference dispatches it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM); tensors are row-major, bf16 (raw uint16) unless noted;
 *     fp32 for RoPE tables, fp32/int64 where stated.
 *   - functions only enqueue work on `stream`; they never allocate, never synchronise, never throw.
 *   - return value: 0 = ok, <0 = error (BYA_ERR_*): nothing was launched.
 *   - "rows" of the joint sequence are [text rows (Tt=226) | video rows (N = T*Ht*Wt)], S = Tt + N.
 */
#ifndef BYA_H
#define BYA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations below are its whole dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

enum { BYA_ACT_NONE = 0, BYA_ACT_GELU_TANH = 1, BYA_ACT_GELU_ERF = 2, BYA_ACT_RELU = 3, BYA_ACT_SILU = 4,
       BYA_ACT_LEAKY_RELU = 5,
       BYA_ACT_GELU_TANH_IEEE = 6 /* bya_gemm_bf16 only: GELU(tanh) through expf + IEEE division (A/B reference) */ };

/* library / build identification: returns the ABI version (bumped when a signature changes). */
int bya_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Process-wide options (round 6).  The entry points below are functions of their arguments and of THIS table only: the
 * library never reads the environment.  The host sets what it wants once, after loading the library (the Python module
 * maps its BYA_* environment variables onto these keys at import, ops.apply_env_options); a launch reads the table when
 * it is prepared, so a change applies to the launches enqueued after it.  bya_set_option returns BYA_ERR_SHAPE for an
 * unknown key or a value outside the key's range; bya_get_option writes the current value.
 * --------------------------------------------------------------------------------------------- */
enum bya_option {
    BYA_OPT_GEMM_SPLITK = 0,      /* 0 (default since the end of round 6): bya_gemm_bf16 never cuts a tile along K -- the rows
                                     behind the last full round of 256-row tiles run on 128-row tiles instead, as fast and without
                                     a hand-off (a shard's rows round like the whole's); 1: the tiles of a partial last round are
                                     split along K when a workspace is registered; 2: every split tile in two */
    BYA_OPT_GEMM_SPLITK_MIN = 1,  /* shortest K range (in 64-wide K tiles) a split may produce; 0 = the built-in default */
    BYA_OPT_GEMM_TILE = 2,        /* -1 (default): tile shape by the cost model; 0..6: force one (tests: every shape through
                                     every kernel) */
    BYA_OPT_GEMM_VARIANT = 3,     /* 0 (default): the one-wave-per-SIMD kernels (256 x 256 tiles, 128 x 256 where that fills the CUs
                                     better) where eligible; 1: the 8-wave kernel; 2: 256 x 256 only (A/B of the 128-row tile) */
    BYA_OPT_ATTN_STREAMK = 4,     /* 1 (default): the joint attention cuts the items of a partial last round between
                                     workgroups when a workspace is registered; 0: one workgroup per item */
    BYA_OPT_FP8_KERNEL = 5,       /* 0 (default): 256 x 256 fp8 kernel where a launch fills it; 1: always the 128 x 128 one */
    BYA_OPT_P2P_GROUPS = 6,       /* workgroups of a push / exchange launch (16..1024); 0 = the built-in default */
    BYA_OPT_REFERENCE_FORMS = 7,  /* bit mask, tests only: take the OLDER kernel form of an A/B the docs call closed; every
                                     form pair is bit-identical, which is what the tests that set these bits assert */
    BYA_OPT_MX_KERNEL = 8,        /* 0 (default): every MX GEMM on the tiled kernels of csrc/gemm_mx.hip; 1: e4m3 x e4m3 launches that
                                     fill the persistent 256 x 256 kernel (csrc/gemm_mx_v4.hip: at least 200 of its tiles, batch
                                     included, and eligible) run on it -- the same bits; 2 (tests): as 1 without the tile count.
                                     (e2m1 weights reach that kernel through bya_gemm_mx_call, which reads no option) */
    BYA_OPT_COUNT = 9
};
enum { BYA_REF_ROWGEMM_CHUNKED = 1,    /* N = 512 row GEMM: chunk-balanced kernel instead of the W-stationary one */
       BYA_REF_KV_MIX_GENERIC = 2,     /* bya_attn_kv_mix: the generic kernel instead of the <= 32-key one */
       BYA_REF_LN_GENERIC = 4,         /* bya_layernorm at 3072 columns: one row per wave instead of parameters in registers */
       BYA_REF_ROUTER_SCORES_WAVE = 8, /* bya_router_scores: keys per wave instead of keys in LDS */
       BYA_REF_ATTN_NARROW_STORE = 16  /* attention epilogues: 8-byte instead of 16-byte stores */ };
int bya_set_option(int32_t key, int32_t value);
int bya_get_option(int32_t key, int32_t* value);

/* Board calibration (diagnostic; csrc/calib.hip): 256 workgroups x 4 waves run `iters` sweeps of 64 v_mfma_f32_16x16x32_bf16 each
 * (a 128 x 128 x 32 wave tile: 2^20 FLOP per wave and sweep, BYA_CALIBRATION_FLOP_PER_ITER per launch and iteration) on the
 * operand fragments at `operands` (>= BYA_CALIBRATION_OPERAND_BYTES of bf16: gaussian for the rate the board sustains on real
 * data, zeros for its full clock).  The caller times the launch (HIP events) -- TFLOP/s = iters * BYA_CALIBRATION_FLOP_PER_ITER /
 * seconds / 1e12.  `sink`: 4 bytes of device memory (never written in practice).  No reference counterpart. */
#define BYA_CALIBRATION_OPERAND_BYTES (256LL * 256 * 16 * 16)
#define BYA_CALIBRATION_FLOP_PER_ITER (256.0 * 4 * 2.0 * 128 * 128 * 32)
int bya_mfma_calibration(const void* operands, int64_t operand_bytes, void* sink, int32_t iters, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GEMM:  C[z][m,n] = res[z][m,n] + gate[z][row-type(m)][n] * alpha * act( sum_k A[z][m,k] * W[n,k] + rowscale[m]*bias[n] )
 * Replaces every nn.Linear / 2x2-stride Conv2d-as-GEMM on the path: attn1.to_q/k/v/to_out,
 * ff.net.0.proj/ff.net.2 (models/transformer.py:241-260), perceiver to_q/to_out (models/router.py:253,275),
 * router to_q/to_k and the SpatialTemporalAttentionBlock projections + mlp (models/router.py:381-383,
 * 468-491), audio attn to_q/to_out (models/audio_model.py:253-256), patch_embed.proj/text_proj,
 * proj_out (models/transformer.py:690,949), and the step-invariant LocalFacialExtractor /
 * AudioProjModel linears (models/router.py:157-193, models/audio_model.py:78-114).
 * bias/res/gate0 may be NULL.  gate1==NULL means gate0 for all rows; rows m < gate_split use gate0.
 * Requirements: K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0, A/W 16-byte aligned.
 * --------------------------------------------------------------------------------------------- */
typedef struct bya_gemm_desc {
    int32_t M, N, K;          /* per batch entry */
    int32_t batch;            /* grid.z; A/C/res/gate advance by the *_batch_stride (elements) */
    int32_t lda, ldw, ldc, ldres;
    int64_t a_batch_stride, c_batch_stride, res_batch_stride, gate_batch_stride;
    int32_t gate_split;
    int32_t act;              /* BYA_ACT_* applied to (acc + bias) */
    int32_t n_split;          /* > 0: column n is written to C + (n / n_split) * c_split_stride, column n % n_split
                                 (one launch for the packed q|k|v projection writing three separate tensors) */
    int64_t c_split_stride;
    const float* bias_rowscale; /* optional fp32 [batch*M]: bias[n] is multiplied by bias_rowscale[z*M + m] */
    float alpha;              /* scales act(acc + bias); 0 is read as 1 */
} bya_gemm_desc;

int bya_gemm_bf16(const void* A, const void* W, const void* bias, void* C, const void* res,
                  const void* gate0, const void* gate1, const bya_gemm_desc* desc, hipStream_t stream);
/* Domain of the bf16 GEMMs (what the definition above promises for bya_gemm_bf16 on every plan path, with split-K and with a row
 * split, for bya_gemm_skinny_bf16 and for bya_rowgemm512 without LayerNorm, and what tests/test_gemm_bf16_cond_gpu.py holds each
 * of them to, element by element against fp64 on the very bits):
 *   operands   every finite bf16 value, subnormals (j * 2^-133, |j| <= 127) and +-255 * 2^120 included: v_mfma_f32_16x16x32_bf16
 *              keeps subnormal operands (measured: rows of nothing but subnormals times 2^120 come back bit-exact on every path,
 *              and a one-hot W returns all 65280 finite bit patterns of A unchanged).  NaN / Inf propagation is not specified.
 *   range      every partial sum, in any K order, and the result within fp32's finite range: sum_k |a_k w_k| below 2^126 is
 *              enough.  Products and sums below 2^-126 underflow gradually (multiples of 2^-149), they are not flushed.
 *   order      any K order: the sum is within 2 K 2^-24 sum_k |a_k w_k| of the exact one (one fp32 addition per product, each
 *              allowed to truncate); where every partial sum is exact in fp32 the result is the exact one rounded once, bit for
 *              bit, on every path.
 *   epilogue   in fp32 with ONE rounding, at the end: v = alpha * act(fma(rowscale, bias, sum)); v *= gate; v += res; bf16(v),
 *              round to nearest even.  No operand or intermediate is rounded to bf16 on the way -- not the gate, not
 *              gate * alpha, not rowscale * bias, not the value the residual is added to.
 * (DESIGN.md section 17 has the first run's figures.) */

/* The packed q|k|v projection of a DiT block WITH the per-head q/k LayerNorm(64, eps, affine) + interleaved-pair RoPE of
 * bya_qknorm_rope in its epilogue (reference models/transformer.py:200-209,241-245 = diffusers Attention.to_q/k/v followed by
 * CogVideoXAttnProcessor2_0's norm_q / norm_k / apply_rotary_emb): columns [0, width) of the product are q, [width, 2 width) k,
 * [2 width, 3 width) v (plain bias epilogue); desc->n_split / c_split_stride place them as for bya_gemm_bf16.  q and k are
 * normalised from the bf16-ROUNDED projection and with the arithmetic of csrc/qknorm_math.h, so the result equals
 * bya_gemm_bf16 followed by bya_qknorm_rope BIT FOR BIT -- q and k are just written once instead of written, read and written
 * again.  rows >= text_rows are rotated with cos / sin [rows - text_rows, 64] fp32 (row index = row of the launch, per batch
 * entry); k_scale as for bya_qknorm_rope.  N = 3 width (q | k | v) or, since round 6, N = 2 width (q | k alone: the sharded step
 * computes v first and pushes it to the peers underneath this launch).  Constraints: no activation / residual / gates, width % 128 == 0, the persistent
 * kernel's alignment rules; BYA_ERR_UNSUPPORTED otherwise (the caller then issues the two launches). */
typedef struct bya_qknorm_desc {
    const void* qw; const void* qb; const void* kw; const void* kb;   /* bf16 [64] each */
    const float* cos; const float* sin;
    int32_t text_rows;
    int32_t width;                                                      /* heads * 64 */
    float eps, k_scale;
} bya_qknorm_desc;
int bya_gemm_qkv_norm_rope(const void* A, const void* W, const void* bias, void* C, const bya_gemm_desc* desc,
                           const bya_qknorm_desc* norm, hipStream_t stream);
/* The fused q|k|v launches that ALSO record bya_qknorm_rope's score-bound statistics: bya_gemm_qkv_norm_rope_stats here,
 * bya_gemm_fp8_qkv_norm_rope_stats and bya_gemm_mx_qkv_norm_rope_stats below -- their entry point's arguments plus `stats`,
 * `stats_slots` in front of the stream.  (Entry points of their own and no new fields: bya_qknorm_desc and bya_mx_gemm_call keep
 * their size and bytes, so every existing caller's descriptors stay valid as they are.)
 * stats: bya_qknorm_rope's table, fp32 [stats_slots][2][batch * heads], zero-filled by the caller before the launch; NULL = the
 * plain entry point's launch.  The kernel raises (atomic maximum on the bit pattern of a non-negative float) entry
 * [workgroup index % stats_slots][0 = q, 1 = k][index] to the squared Euclidean norm of the finished, bf16-ROUNDED head rows as
 * it stores them; 1 <= stats_slots <= 64 (BYA_ERR_SHAPE), the table 4-byte aligned (BYA_ERR_ALIGN), both checked before
 * anything is launched.  `index` is what the two-launch path's bya_qknorm_rope writes: with n_split == width (dense)
 * z * (width / 64) + head  of batch entry z; with n_split < width (the column blocks of the head-parallel sharded step:
 * width % n_split == 0, n_split % 64 == 0, desc->batch == 1) the global head (column - tensor * width) / 64.  Column blocks
 * with desc->batch > 1, or any other n_split: BYA_ERR_UNSUPPORTED.  The maximum over the slots equals bya_qknorm_rope's BIT FOR
 * BIT (the squares of bf16 values are exact in fp32, their sum runs in the order of csrc/qknorm_math.h, a maximum does not depend
 * on order); which slot holds it differs.  Rows past M, columns past N and v contribute nothing.  C is the plain entry point's,
 * bit for bit.  A kernel path that does not record statistics answers BYA_ERR_UNSUPPORTED to a non-NULL table and launches
 * nothing (the caller then issues the two launches): bya_gemm_qkv_norm_rope_stats records them on every plan path (the STATS
 * instances of csrc/gemm_v4.hip and gemm_v5.hip); the fp8 and MX forms on path P256 alone.  Every other answer is the plain
 * entry point's. */
int bya_gemm_qkv_norm_rope_stats(const void* A, const void* W, const void* bias, void* C, const bya_gemm_desc* desc,
                                 const bya_qknorm_desc* norm, float* stats, int32_t stats_slots, hipStream_t stream);

/* The same product for SKINNY launches -- at most 64 rows, N <= 8192, N % 16 == 0, K % 32 == 0, K >= 256, no gates, no
 * bias_rowscale, no n_split (anything else: BYA_ERR_UNSUPPORTED) -- on a weight-streaming kernel: one workgroup per 16
 * output columns (batch elements stacked as rows while they fit 64 together), 16 waves split K, partial sums added in a
 * fixed order.  For Linears whose few rows meet a wide weight (the step-invariant conditioning: nn.Linear call sites of
 * models/router.py:216-262 (Perceiver to_kv / LocalFacialExtractor) and models/audio_model.py:78-114 (AudioProjModel)): the
 * tiled kernels give such a launch N / 128 workgroups.  It is a separate entry point because its fp32 summation order
 * differs from bya_gemm_bf16's: which kernel runs is the caller's decision, never a function of the row count. */
int bya_gemm_skinny_bf16(const void* A, const void* W, const void* bias, void* C, const void* res,
                         const bya_gemm_desc* desc, hipStream_t stream);

/* Optional split-K workspace of the persistent GEMM kernel (device memory owned by the caller, 256-byte aligned, at
 * least the size bya_gemm_workspace_bytes reports, ZERO-FILLED once): with it, the last partial round of 256 x 256 output tiles
 * of a bya_gemm_bf16 launch is cut along K over the idle CUs (partial sums and completion counters live here).  One
 * workspace per DEVICE (registered for, and used by launches enqueued under, the current device); launches that use it
 * must be ordered on one stream.  NULL unregisters.  Results do not depend on it beyond fp32 summation order.  (No
 * reference counterpart: scheduling detail of the Linear layers.) */
int bya_set_gemm_workspace(void* ws, int64_t bytes);
int bya_gemm_workspace_bytes(int64_t* bytes);
/* Health of the current device's workspace: *timeouts = number of split tiles whose finisher gave up waiting (~1 s) for a
 * partial sum and finished without it -- 0 on a healthy run; anything else means outputs of that launch were wrong.
 * Completion counters carry the launch epoch, so a late writer of such a launch cannot corrupt later launches.  The ONE
 * entry point that synchronises (it copies a word back over `stream`): call it at step or run end, not per launch. */
int bya_gemm_workspace_status(int32_t* timeouts, hipStream_t stream);

/* Which kernels a GEMM launch runs (host-side queries like bya_attn_variant: they launch nothing and need no GPU).  The GEMM
 * entry points choose their kernels by shape, pointer alignment, the current device's split-K workspace and the options
 * table; each query takes the arguments of its entry point (stream replaced by the plan) and reports what a launch with
 * the same arguments, enqueued now, runs -- the launch calls the same plan functions.  Return value: what the entry point
 * would return before launching (0, or the BYA_ERR_* that rejects the arguments; the plan is then untouched).
 * Path codes (the 256 x 256 and 128 x 256 "persistent" kernels run one wave per SIMD): */
#define BYA_GEMM_PATH_T128X64 0   /* 128 x 64 tiles, 4 waves (option gemm_tile = 0; N <= 64) */
#define BYA_GEMM_PATH_T128X128 1  /* 128 x 128 tiles, 4 waves (gemm_tile = 1); bya_gemm_fp8 / bya_gemm_mx: their 128 x 128 kernel */
#define BYA_GEMM_PATH_T256X128 2  /* 256 x 128 tiles, 8 waves (gemm_tile = 2) */
#define BYA_GEMM_PATH_T256X256 3  /* 256 x 256 tiles, 8 waves (gemm_tile = 3); bya_gemm_mx: the 256 x 256 kernel of e2m3 activations */
#define BYA_GEMM_PATH_P256 4      /* persistent 256 x 256 (csrc/gemm_v4.hip); bya_gemm_fp8: csrc/gemm_fp8_v4.hip; bya_gemm_mx /
                                     bya_gemm_mx_mixed / bya_gemm_mx_quant (out e4m3) under option mx_kernel, e4m3 x e4m3 only:
                                     csrc/gemm_mx_v4.hip.  bya_gemm_mx_qkv_norm_rope never takes it;
                                     bya_gemm_mx_qkv_norm_rope_on takes it by its `kernel` argument, and so does
                                     bya_gemm_mx_call -- for e4m3 x e2m1 launches too, and with BYA_MX_KERNEL_FP6 in its
                                     `kernel` for e2m3 activations (weights e2m3 or e2m1) and e2m3 output as well */
#define BYA_GEMM_PATH_P128 5      /* persistent 128 x 256 (csrc/gemm_v5.hip) */
#define BYA_GEMM_PATH_P128S 6     /* persistent 128 x 256 with loader waves (csrc/gemm_v6.hip) */
#define BYA_GEMM_PATH_W8_256 7    /* the 8-wave 256 x 256 kernel P256 falls back to (fewer than 3 K-tiles, a C / res / bias /
                                     gate pointer or stride that is not 16-byte aligned) and that option gemm_variant = 1 takes */
#define BYA_GEMM_PATH_COUNT 8
typedef struct bya_gemm_plan {
    int32_t path;             /* BYA_GEMM_PATH_*; with a row split: the kernel of rows [0, m0) */
    int32_t m0;               /* > 0: row split -- rows [m0, M) run as a second launch on `tail`; 0: no split */
    int32_t tail;             /* BYA_GEMM_PATH_* of the rows behind m0; -1 without a row split */
    int32_t split_k;          /* P256 cuts the tiles of its last, partial round along K (option gemm_splitk: 1 or 2); 0: no */
    int32_t row_chunks;       /* launches the 2 GiB reach of the epilogues cuts the product into (1: one; the fields above
                                 describe the first) */
} bya_gemm_plan;
/* bya_gemm_bf16 */
int bya_gemm_bf16_plan(const void* A, const void* W, const void* bias, const void* C, const void* res,
                       const void* gate0, const void* gate1, const bya_gemm_desc* desc, bya_gemm_plan* plan);
/* bya_gemm_qkv_norm_rope: path P256 (its plan 0), P128 (plan 1: 128-row tiles) or P256 with m0 and tail P128 (plan 2);
 * BYA_ERR_UNSUPPORTED where the entry point declines the shape */
int bya_gemm_qkv_norm_rope_plan(const void* A, const void* W, const void* bias, const void* C, const bya_gemm_desc* desc,
                                const bya_qknorm_desc* norm, bya_gemm_plan* plan);
/* bya_gemm_qkv_norm_rope_stats: the same paths */
int bya_gemm_qkv_norm_rope_stats_plan(const void* A, const void* W, const void* bias, const void* C, const bya_gemm_desc* desc,
                                      const bya_qknorm_desc* norm, const float* stats, int32_t stats_slots, bya_gemm_plan* plan);

/* ---------------------------------------------------------------------------------------------
 * fp8 weights (BASELINE configs[4]; no reference counterpart: the reference runs bf16/fp16 only).
 * OCP e4m3fn bytes, symmetric per-row scales:  x[m,k] ~= scale[m] * fp8(q[m,k]).
 *
 * bya_quantize_rows_fp8:  scale[m] = max_k |x[m,k]| / 448 (1 for an all-zero row),
 *                         q[m,k]  = e4m3( x[m,k] * inv ),  inv = fp32(448 / max_k |x[m,k]|) correctly rounded, the product
 *                         in fp32, one round-to-nearest-even to e4m3 (torch.float8_e4m3fn's converter, byte for byte).
 *   Used once per weight at load time (rows = output channels) and on the fly for the activations of each fp8 GEMM.
 *   x bf16 [M, K] (row stride ldx), q uint8 [M, K] (row stride ldq), scale fp32 [M].  K % 8 == 0, K <= 12288.
 *
 * bya_gemm_fp8:  C[z][m,n] = res + gate * alpha * act( a_scale[z*M+m] * w_scale[n] * sum_k A8[z][m,k] * W8[n,k] + rowscale*bias[n] )
 *   on v_mfma_scale_f32_16x16x128_f8f6f4 (fp32 accumulation); same descriptor and epilogue as bya_gemm_bf16, with lda / ldw /
 *   a_batch_stride counted in fp8 elements (bytes).  Replaces attn1.to_q|k|v, attn1.to_out, ff.net.0.proj and ff.net.2 of a
 *   CogVideoXBlock (models/transformer.py:241-260) when the engine is built with fp8 weights.
 *   Requirements: K % 128 == 0, N % 4 == 0, lda/ldw % 16 == 0, A8/W8/w_scale 16-byte aligned; act in {NONE, GELU_TANH(_IEEE)}.
 *   What it refuses, launch and plan query alike, before anything runs (tests/test_fp8_exact_gpu.py asserts each): any other
 *   activation (GELU_ERF, RELU, SILU, LEAKY_RELU: BYA_ERR_UNSUPPORTED -- the kernels instantiate the epilogue of the DiT Linears
 *   only); n_split together with a residual (BYA_ERR_SHAPE, as for bya_gemm_bf16: the residual has no column map); ldc / ldres
 *   % 4 or a C / res / bias / gate pointer that is not 8-byte aligned (BYA_ERR_ALIGN).
 *   Which kernel: the persistent 256 x 256 one takes a launch of at least 200 of its tiles (batch included; option
 *   BYA_OPT_FP8_KERNEL set to 1 keeps every launch off it, no option puts a smaller launch on it) that has at least 4 K-tiles (K >=
 *   512), N % 8 == 0, n_split / c_split_stride / ldc / ldres / the batch strides of C, res and the gates % 8 == 0 and C, res,
 *   bias and both gates 16-byte aligned; every other launch -- N = 260, a C view 8 but not 16 bytes aligned, K = 384, a single
 *   output tile -- runs on the 128 x 128 kernel, which has none of these conditions.  On data whose sums are exact in fp32 the
 *   two return the same bits.  A launch whose C or residual rows span 2 GiB runs as row chunks of whole 256-row blocks per
 *   batch entry (bya_gemm_plan::row_chunks), each on the kernel the whole launch's tile count and its own alignment select.
 * --------------------------------------------------------------------------------------------- */
int bya_quantize_rows_fp8(const void* x, void* q, float* scale, int32_t M, int32_t K, int64_t ldx, int64_t ldq,
                          hipStream_t stream);
int bya_gemm_fp8(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias, void* C,
                 const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* desc, hipStream_t stream);
/* its kernel (bya_gemm_bf16_plan): path T128X128 (the 128 x 128 kernel) or P256 (the persistent 256 x 256 one) */
int bya_gemm_fp8_plan(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias,
                      const void* C, const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* desc,
                      bya_gemm_plan* plan);
/* bya_gemm_fp8_qkv_norm_rope:  bya_gemm_fp8 of the packed q|k|v projection WITH the per-head q/k LayerNorm(64) + RoPE of
 *   bya_qknorm_rope in its epilogue (bya_gemm_qkv_norm_rope's counterpart on e4m3 operands): bit for bit bya_gemm_fp8(...,
 *   n_split) followed by bya_qknorm_rope -- per element a_scale[m] * w_scale[n] is formed first and multiplies the accumulator,
 *   the bias is added to that fp32 product (no fused multiply-add across the two), the sum is rounded to bf16 ONCE (the value
 *   the two-launch path stored and read back), and q and k are normalised from it with the arithmetic of csrc/qknorm_math.h and
 *   written once; v columns take the plain bias epilogue.  The two descriptors mean what they mean for bya_gemm_qkv_norm_rope:
 *   N = 3 width (q | k | v) or 2 width (q | k alone), n_split > 0 with c_split_stride (n_split = width, or a column block
 *   n_split < width), text_rows, cos / sin [M - text_rows, 64] fp32, k_scale (0 is read as 1), batch (the rotary row index
 *   restarts per batch entry).  q, k or v is decided per 64-column head, so width % 64 == 0 is enough (a tile may straddle
 *   q | k).  Always ONE launch, on the kernel bya_gemm_fp8 would choose for the same descriptor (option BYA_OPT_FP8_KERNEL, at
 *   least 200 tiles of 256 x 256, eligibility: bya_gemm_fp8_plan's rule) -- the two fp8 kernels differ in last bits, so the
 *   path is never swapped.  bya_gemm_fp8_qkv_norm_rope_stats (bya_gemm_qkv_norm_rope_stats above) records the norm statistics on
 *   path P256 (gemm256p_fp8_qkn_stats_kernel); where the launch would take T128X128 a non-NULL table is answered
 *   BYA_ERR_UNSUPPORTED.  BYA_ERR_UNSUPPORTED, nothing launched (the
 *   caller keeps the two launches): an activation, bias_rowscale, alpha other than 0 / 1, n_split == 0, width % 64, N neither
 *   2 nor 3 widths, a descriptor that describes a residual (ldres or res_batch_stride != 0: there are no residual / gate
 *   arguments), rows or rotary rows beyond the 2 GiB reach of one launch's buffer descriptors.  n_split, c_split_stride, ldc,
 *   c_batch_stride % 8 == 0 and C, the four norm vectors, cos and sin 16-byte aligned (BYA_ERR_ALIGN); otherwise the checks of
 *   bya_gemm_fp8 and of bya_gemm_qkv_norm_rope's norm descriptor (BYA_ERR_SHAPE; cos / sin may be null when every row is
 *   text).  Every check runs before any launch (and without a GPU); a refused plan query leaves *plan untouched. */
int bya_gemm_fp8_qkv_norm_rope(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias,
                               void* C, const bya_gemm_desc* desc, const bya_qknorm_desc* norm, hipStream_t stream);
/* its kernel: path T128X128 or P256 (bya_gemm_fp8_plan's answer for the same descriptor), row_chunks 1, no split;
 * BYA_ERR_UNSUPPORTED where the entry point declines the shape */
int bya_gemm_fp8_qkv_norm_rope_plan(const void* A8, const float* a_scale, const void* W8, const float* w_scale,
                                    const void* bias, const void* C, const bya_gemm_desc* desc, const bya_qknorm_desc* norm,
                                    bya_gemm_plan* plan);
int bya_gemm_fp8_qkv_norm_rope_stats(const void* A8, const float* a_scale, const void* W8, const float* w_scale, const void* bias,
                                     void* C, const bya_gemm_desc* desc, const bya_qknorm_desc* norm, float* stats,
                                     int32_t stats_slots, hipStream_t stream);
int bya_gemm_fp8_qkv_norm_rope_stats_plan(const void* A8, const float* a_scale, const void* W8, const float* w_scale,
                                          const void* bias, const void* C, const bya_gemm_desc* desc, const bya_qknorm_desc* norm,
                                          const float* stats, int32_t stats_slots, bya_gemm_plan* plan);
/* bya_layernorm_fp8: bya_layernorm (same arguments, same arithmetic) followed by bya_quantize_rows_fp8 of each output row,
 * in one pass: the normalised + modulated row is rounded to bf16 exactly as bya_layernorm would store it, then quantised --
 * byte for byte what the two launches produce, without the bf16 round trip.  q uint8 [batch][rows][D] (row stride ldq,
 * batch stride q_batch_stride, bytes), q_scale fp32 [batch * rows_per_batch].  D = 3072 only (the AdaLN LayerNorms of
 * CogVideoXBlock, models/transformer.py:233,251, in front of the q|k|v and MLP Linears). */
int bya_layernorm_fp8(const void* x, void* q, float* q_scale, const void* w, const void* b, const void* shift0,
                      const void* scale0, const void* shift1, const void* scale1, int64_t rows_per_batch, int32_t batch,
                      int32_t D, int64_t ldx, int64_t ldq, int64_t x_batch_stride, int64_t q_batch_stride,
                      int64_t mod_batch_stride, int64_t split, float eps, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MX weights (OCP Microscaling; no reference counterpart: the reference runs bf16/fp16 only).  Elements in blocks of 32
 * consecutive values along K, each block with one e8m0 scale byte:  x[m, 32 b + i] ~= 2^(scale[m,b] - 127) * elem(code).
 * Element formats, numbered as the matrix instruction's cbsz / blgp fields:
 *   BYA_MX_E4M3 = 0: OCP e4m3fn, emax_elem = 8, largest finite 448, 32 bytes per block (element i = byte i);
 *   BYA_MX_E2M3 = 2: OCP e2m3 (1 sign, 2 exponent bits of bias 1, 3 mantissa bits, no inf / NaN), emax_elem = 2,
 *                    largest finite 7.5, 24 bytes per block: element i at bits 6i .. 6i+5 of the block's 192-bit
 *                    little-endian string (least significant bit first: the order v_mfma_scale_f32_16x16x128_f8f6f4
 *                    reads from its six operand VGPRs, checked on exact data).
 *   BYA_MX_E2M1 = 4: OCP e2m1 (1 sign, 2 exponent bits of bias 1, 1 mantissa bit, no inf / NaN; magnitudes 0, 0.5, 1, 1.5,
 *                    2, 3, 4, 6), emax_elem = 2, largest finite 6, 16 bytes per block: element i in bits 4 (i % 2) .. +3 of
 *                    byte i / 2, low nibble first (the order the instruction reads from its four operand VGPRs, measured
 *                    on exact data: tests/test_mxfp4_gpu.py).  WEIGHTS only: bya_quantize_mx writes it, bya_gemm_mx_mixed
 *                    multiplies it with e4m3 or e2m3 activations; e2m1 activations are not offered.
 *   Storage is the plain row-major order in every format; the GEMM kernel arranges the operand VGPRs per format
 *   (csrc/gemm_mx.hip: for e4m3 the instruction's 32-k block spans two 16-byte pieces of different lanes).
 *
 * Scale of block b of row m (amax = max |x| over the block, taken on the bf16 values):
 *   E = floor(log2 amax) - emax_elem, clamped to [-127, 127]; stored byte E + 127.
 *   An all-zero block (+0 or -0 values only) stores the byte 127 and all-zero codes.
 * Element code:  q = RNE(x * 2^-E) (one round-to-nearest-even from the exact product), saturated to +-largest finite;
 *   the sign of x is kept (a negative value that rounds to zero gives -0).
 * Storage: codes uint8 [rows, K * bits / 8] row-major (row stride K * bits / 8, no padding), scales uint8 [rows, K / 32].
 *   Weights use the same layout with rows = output channels.  K % 128 == 0.
 *
 * bya_quantize_mx:  bf16 x [M, K] (row stride ldx, elements) -> codes, scales.  ldx % 8 == 0, x 16-byte aligned.
 * bya_layernorm_mx: bya_layernorm (same arguments, same arithmetic as bya_layernorm_fp8) followed by bya_quantize_mx of each
 *   bf16-rounded output row, in one pass -- byte for byte the two launches.  codes [batch][rows][D * bits / 8] (row stride
 *   ldq, batch stride q_batch_stride, bytes; both % 8 == 0), scales [batch * rows_per_batch, D / 32].  D = 3072 only.
 * bya_gemm_mx:  C[z][m,n] = res + gate * alpha * act( sum_k A[z][m,k] * W[n,k] + rowscale*bias[n] ) with A and W in MX form
 *   on v_mfma_scale_f32_16x16x128_f8f6f4, the block scales applied by the instruction (fp32 accumulation).  Same
 *   descriptor and epilogue as bya_gemm_bf16; lda / ldw / a_batch_stride count BYTES of codes; a_scales is
 *   [batch * M, K / 32], w_scales [N, K / 32] (dense).  Both operands use the same element format.
 *   Requirements: K % 128 == 0, N % 4 == 0, lda / ldw % 16 == 0, A / W 16-byte aligned, a_scales / w_scales 4-byte aligned,
 *   batch * M * K / 32 < 2^31; act in {NONE, GELU_TANH(_IEEE)}.  fmt = BYA_MX_E2M1: BYA_ERR_SHAPE.
 * bya_gemm_mx_mixed:  bya_gemm_mx with a format per operand (the instruction's cbsz / blgp): a_fmt in {E4M3, E2M3};
 *   w_fmt == a_fmt is exactly bya_gemm_mx, w_fmt == BYA_MX_E2M1 multiplies 4-bit weights (codes [N, K / 2]) with the same
 *   activations; every other pair: BYA_ERR_UNSUPPORTED.  lda / ldw are checked against each operand's own row bytes.  The
 *   kernel (tile, ring) follows the activation format.
 * bya_gemm_mx_quant:  bya_gemm_mx_mixed whose epilogue writes MX codes instead of bf16 -- the A operand of the next MX GEMM:
 *     v[z][m,n] = bf16( alpha * act( sum_k A[z][m,k] * W[n,k] + rowscale*bias[n] ) ),   (q_codes, q_scales) = MX(out_fmt) of v
 *   byte for byte bya_gemm_mx_mixed followed by bya_quantize_mx(out_fmt), in one launch and without the bf16 tensor (a block
 *   of 32 output columns of a row sits in one wave of the kernel).  out_fmt in {E4M3, E2M3}, whatever the operand formats;
 *   BYA_MX_E2M1 (never an activation format) and every operand pair bya_gemm_mx_mixed refuses: BYA_ERR_UNSUPPORTED.
 *   q_codes uint8 [batch][M][N * bits / 8]: ldc = row stride and c_batch_stride = batch stride, both in BYTES of codes
 *   (ldc >= N * bits / 8; bytes of a row behind that are not written); q_scales uint8 [batch * M, N / 32], dense.
 *   N % 128 == 0 (a legal K); ldc % 16 == 0, c_batch_stride % 16 == 0, q_codes 16-byte and q_scales 4-byte aligned
 *   (BYA_ERR_ALIGN); the operand side as bya_gemm_mx_mixed.  act in {NONE, GELU_TANH(_IEEE)}; alpha and bias_rowscale as in
 *   bya_gemm_mx.  Codes cannot carry a residual, gates or a column split: there are no such arguments, ldres / gate fields
 *   are ignored and n_split != 0 is BYA_ERR_UNSUPPORTED.  Every check runs before any launch (and without a GPU).
 * bya_gemm_mx_qkv_norm_rope:  bya_gemm_mx_mixed of the packed q|k|v projection WITH the per-head q/k LayerNorm(64) + RoPE of
 *   bya_qknorm_rope in its epilogue (bya_gemm_qkv_norm_rope's counterpart on MX operands): bit for bit bya_gemm_mx_mixed(...,
 *   n_split) followed by bya_qknorm_rope -- q and k are normalised from the bf16-ROUNDED projection with the arithmetic of
 *   csrc/qknorm_math.h and written once; v columns take the plain bias epilogue.  The two descriptors mean what they mean for
 *   bya_gemm_qkv_norm_rope: N = 3 width (q | k | v) or 2 width (q | k alone), n_split > 0 with c_split_stride (n_split = width,
 *   or a column block n_split < width), text_rows, cos / sin [M - text_rows, 64] fp32, k_scale (0 is read as 1), batch.
 *   q, k or v is decided per 64-column head, so width % 64 == 0 is enough (a tile may straddle q | k); the tile follows the
 *   activation format as for every MX GEMM (bya_gemm_mx_mixed_plan's rule).  The norm statistics of bya_qknorm_rope are not
 *   offered.  BYA_ERR_UNSUPPORTED, nothing launched (the caller keeps the two launches): an activation, bias_rowscale, alpha
 *   other than 0 / 1, n_split == 0, width % 64, N neither 2 nor 3 widths, e2m1 activations (every operand pair
 *   bya_gemm_mx_mixed refuses), rows or rotary rows beyond the 2 GiB reach of one launch's buffer descriptors.  There are no
 *   residual / gate arguments; those descriptor fields are ignored.  n_split, c_split_stride, ldc, c_batch_stride % 8 == 0 and
 *   C, the four norm vectors, cos and sin 16-byte aligned (BYA_ERR_ALIGN); otherwise the checks of bya_gemm_mx_mixed and of
 *   bya_gemm_qkv_norm_rope's norm descriptor (BYA_ERR_SHAPE).  Every check runs before any launch (and without a GPU).
 *
 * Domain of the GEMMs (what the definitions above promise, and what tests/test_gemm_cond_gpu.py holds every kernel instance to,
 * element by element against fp64 on the very bytes; the bytes need not come from bya_quantize_mx):
 *   codes        every finite code of the format -- e4m3 subnormals (0x01 .. 0x07) and +-448, all 64 e2m3 and all 16 e2m1 codes,
 *                +-0 included.  The e4m3 NaN codes 0x7F / 0xFF are outside the domain (NaN / Inf propagation is not specified).
 *   scale bytes  0 .. 254 (2^-127 .. 2^127).  The e8m0 NaN byte 255 is outside the domain.
 *   along K      for every A block and the W block it meets, |E_a + E_w| <= 64 (E = byte - 127), so that every scaled product
 *                is a normal fp32: the bytes may be individually extreme (A at 27, W at 227), their products may not.
 *   result       res + gate * alpha * act(sum + rowscale * bias) with the sum within 2 K 2^-24 sum_k |a_k w_k| of the exact one
 *                (fp32 accumulation in any order), then ONE rounding to bf16; where every partial sum is exact in fp32 the
 *                result is the exact one rounded once, bit for bit.  e4m3 activations add the instruction's own block sum to
 *                that bound: inside a 32-block it aligns the non-zero products by their exponent fields (a subnormal code
 *                counts as 2^-6, a zero code takes no part) and drops, toward zero, the bits below 2^-13 of the largest
 *                exponent sum (tests/test_gemm_cond_gpu.py asserts it on probes) -- at most
 *                min(|p_k|, q) per product that has such bits.  e2m3 activations never have any.
 *   bya_gemm_fp8 every finite e4m3 code; row scales any finite positive fp32, not only powers of two (the product of the two
 *                scales is rounded to fp32 before it multiplies the sum).
 * --------------------------------------------------------------------------------------------- */
enum { BYA_MX_E4M3 = 0, BYA_MX_E2M3 = 2, BYA_MX_E2M1 = 4 };
int bya_quantize_mx(const void* x, void* codes, void* scales, int32_t M, int32_t K, int64_t ldx, int32_t fmt,
                    hipStream_t stream);
int bya_layernorm_mx(const void* x, void* q, void* q_scales, const void* w, const void* b, const void* shift0,
                     const void* scale0, const void* shift1, const void* scale1, int64_t rows_per_batch, int32_t batch,
                     int32_t D, int64_t ldx, int64_t ldq, int64_t x_batch_stride, int64_t q_batch_stride,
                     int64_t mod_batch_stride, int64_t split, float eps, int32_t fmt, hipStream_t stream);
int bya_gemm_mx(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, void* C,
                const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* desc, int32_t fmt,
                hipStream_t stream);
/* its kernel (bya_gemm_bf16_plan): path T128X128 (both formats) or T256X256 (e2m3 only); with option BYA_OPT_MX_KERNEL at 1 a
 * launch with e4m3 activations AND weights takes path P256 (csrc/gemm_mx_v4.hip, the same bits) when it has at least 200 tiles of
 * 256 x 256, batch included, and is eligible -- K % 128 == 0, K >= 512, N % 8 == 0, C / res / bias / gates 16-byte aligned,
 * checked per row chunk; at 2 (tests): without the tile count */
int bya_gemm_mx_plan(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                     const void* C, const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* desc,
                     int32_t fmt, bya_gemm_plan* plan);
int bya_gemm_mx_mixed(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias, void* C,
                      const void* res, const void* gate0, const void* gate1, const bya_gemm_desc* desc, int32_t a_fmt,
                      int32_t w_fmt, hipStream_t stream);
/* its kernel: path T128X128, or T256X256 for e2m3 activations (bya_gemm_mx_plan's rule, whatever w_fmt); P256 under option
 * BYA_OPT_MX_KERNEL only with a_fmt == w_fmt == e4m3 */
int bya_gemm_mx_mixed_plan(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                           const void* C, const void* res, const void* gate0, const void* gate1,
                           const bya_gemm_desc* desc, int32_t a_fmt, int32_t w_fmt, bya_gemm_plan* plan);
int bya_gemm_mx_quant(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                      void* q_codes, void* q_scales, const bya_gemm_desc* desc, int32_t a_fmt, int32_t w_fmt,
                      int32_t out_fmt, hipStream_t stream);
/* its kernel: bya_gemm_mx_mixed_plan's rule (path T128X128, or T256X256 for e2m3 activations; P256 under option
 * BYA_OPT_MX_KERNEL when out_fmt is e4m3 as well -- out_fmt e2m3 stays on the 128 x 128 kernel); never cut into row chunks */
int bya_gemm_mx_quant_plan(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                           const void* q_codes, const void* q_scales, const bya_gemm_desc* desc, int32_t a_fmt,
                           int32_t w_fmt, int32_t out_fmt, bya_gemm_plan* plan);
int bya_gemm_mx_qkv_norm_rope(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                              void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* desc, const bya_qknorm_desc* norm,
                              hipStream_t stream);
/* its kernel: path T128X128, or T256X256 for e2m3 activations, whatever option BYA_OPT_MX_KERNEL says; always one launch;
 * BYA_ERR_UNSUPPORTED where the entry point declines the shape */
int bya_gemm_mx_qkv_norm_rope_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                   const void* bias, const void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* desc,
                                   const bya_qknorm_desc* norm, bya_gemm_plan* plan);
/* bya_gemm_mx_qkv_norm_rope with its kernel named by an ARGUMENT (no option is read; BYA_OPT_MX_KERNEL has no say):
 *   kernel = 0: exactly bya_gemm_mx_qkv_norm_rope -- same checks, same launch;
 *   kernel = 1: path P256 -- the persistent 256 x 256 kernel of csrc/gemm_mx_v4.hip with the same epilogue, the same bits --
 *     when fmt == w_fmt == e4m3, the launch has at least 200 tiles of 256 x 256 (batch included) and is eligible as for
 *     bya_gemm_mx_plan (K % 128 == 0, K >= 512, bias 16-byte aligned, on top of this entry point's own checks); otherwise
 *     the tiled kernel of bya_gemm_mx_qkv_norm_rope;
 *   kernel = 2 (tests): as 1 without the tile count;
 *   any other value: BYA_ERR_SHAPE.
 * Always one launch; every other error is bya_gemm_mx_qkv_norm_rope's. */
int bya_gemm_mx_qkv_norm_rope_on(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                                 void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* desc, const bya_qknorm_desc* norm,
                                 int32_t kernel, hipStream_t stream);
/* its kernel: path T128X128, T256X256 (e2m3 activations) or P256 */
int bya_gemm_mx_qkv_norm_rope_on_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                      const void* bias, const void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* desc,
                                      const bya_qknorm_desc* norm, int32_t kernel, bya_gemm_plan* plan);
/* bya_gemm_mx_qkv_norm_rope_on that also records the norm statistics (bya_gemm_qkv_norm_rope_stats above).  `kernel` is
 * bya_gemm_mx_call's (0, 1, 2, or BYA_MX_KERNEL_FP6 + one of them; anything else BYA_ERR_SHAPE): e2m1 weights and, under the flag,
 * e2m3 activations are admitted to path P256 as there.  The statistics are recorded on path P256 (every operand pair); where
 * the launch would take a tiled kernel a non-NULL table is answered BYA_ERR_UNSUPPORTED. */
int bya_gemm_mx_qkv_norm_rope_stats(const void* A, const void* a_scales, const void* W, const void* w_scales, const void* bias,
                                    void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* desc, const bya_qknorm_desc* norm,
                                    int32_t kernel, float* stats, int32_t stats_slots, hipStream_t stream);
int bya_gemm_mx_qkv_norm_rope_stats_plan(const void* A, const void* a_scales, const void* W, const void* w_scales,
                                         const void* bias, const void* C, int32_t fmt, int32_t w_fmt, const bya_gemm_desc* desc,
                                         const bya_qknorm_desc* norm, int32_t kernel, const float* stats, int32_t stats_slots,
                                         bya_gemm_plan* plan);
/* Any of the MX GEMMs above as ONE call whose kernel is named by an ARGUMENT (no option is read; BYA_OPT_MX_KERNEL has no say),
 * and the one way e2m1 weights reach the persistent kernel.  The epilogue follows from the fields: `norm` set = the q/k-norm +
 * RoPE epilogue (bya_gemm_mx_qkv_norm_rope); `q_scales` set = the quantising epilogue (bya_gemm_mx_quant: C = the output codes,
 * ldc / c_batch_stride in bytes, out_fmt); neither = the bf16 epilogue (bya_gemm_mx_mixed: res, gate0, gate1).
 *   kernel = 0: exactly the old entry point of that epilogue as it runs with option BYA_OPT_MX_KERNEL at 0 -- same checks, same row
 *     chunks, same launch;
 *   kernel = 1: path P256 -- the persistent 256 x 256 kernel of csrc/gemm_mx_v4.hip with the same epilogue, the same bits --
 *     when a_fmt is e4m3, w_fmt is e4m3 OR e2m1, out_fmt (quantising epilogue) is e4m3, the launch has at least 200 tiles of
 *     256 x 256 (batch included) and is eligible as for bya_gemm_mx_plan, ldw counting the bytes of the weights' own rows
 *     (K % 128 == 0, K >= 512, N % 8 == 0, ldw % 16 == 0, N * ldw < 2^32, the epilogue's 16-byte alignments); otherwise what
 *     the old entry point runs: T128X128, or T256X256 for e2m3 activations;
 *   kernel = 2 (tests): as 1 without the tile count.
 *   kernel = BYA_MX_KERNEL_FP6 + 1 / + 2 (17, 18): as 1 / 2, and launches whose a_fmt is e2m3 (w_fmt e2m3 or e2m1) and / or whose
 *     out_fmt (quantising epilogue) is e2m3 take path P256 by the same rule, lda / ldw counting the bytes of a code row -- the
 *     e2m3-operand and e2m3-output instances of that kernel, the same bits.  Without the flag such launches stay on the tiled
 *     kernel under every kernel value.  BYA_MX_KERNEL_FP6 alone (16) is 0.
 * Errors: whatever the old entry point of the epilogue refuses, with its code, before any launch, under every kernel value;
 * BYA_ERR_SHAPE for a null call / desc / plan, kernel not one of 0, 1, 2, 16, 17, 18, norm and q_scales both set, and res /
 * gate0 / gate1 set together with norm or q_scales.  A refused query leaves *plan untouched. */
#define BYA_MX_KERNEL_FP6 16        /* flag bit of bya_mx_gemm_call::kernel: e2m3 operands / output may take path P256 */
typedef struct bya_mx_gemm_call {
    const void *A, *a_scales, *W, *w_scales, *bias;
    void* C;                        /* bf16 output; with q_scales set: the output codes (ldc / c_batch_stride in bytes) */
    const void *res, *gate0, *gate1;/* bf16 epilogue only */
    void* q_scales;                 /* non-null: the quantising epilogue (bya_gemm_mx_quant), out_fmt */
    const bya_qknorm_desc* norm;    /* non-null: the q/k-norm + RoPE epilogue (bya_gemm_mx_qkv_norm_rope) */
    int32_t a_fmt, w_fmt, out_fmt, kernel;      /* kernel: 0, 1, 2, or BYA_MX_KERNEL_FP6 + one of them (above) */
} bya_mx_gemm_call;
int bya_gemm_mx_call(const bya_mx_gemm_call* call, const bya_gemm_desc* desc, hipStream_t stream);
/* its kernel: path T128X128, T256X256 (e2m3 activations) or P256; row_chunks as bya_gemm_mx_mixed_plan's (bf16 epilogue) */
int bya_gemm_mx_call_plan(const bya_mx_gemm_call* call, const bya_gemm_desc* desc, bya_gemm_plan* plan);

/* ---------------------------------------------------------------------------------------------
 * Small-M linear (M <= 8 rows):  out[m,n] = sum_k f(x[m,k]) * W[n,k] + bias[n],  f = identity or SiLU.
 * HBM-bound weight stream.  Replaces TimestepEmbedding.linear_1/2, CogVideoXLayerNormZero.linear
 * (models/transformer.py:198,212 -- all 2*num_layers of them in ONE launch over packed weights) and
 * AdaLayerNorm.linear (models/transformer.py:420-426).  act_out applied after bias.
 * --------------------------------------------------------------------------------------------- */
int bya_linear_small_m(const void* x, const void* W, const void* bias, void* out, int32_t M, int32_t N,
                       int32_t K, int32_t silu_in, int32_t act_out, hipStream_t stream);

/* What a launch of one of the small step kernels would do (host-side queries: they launch nothing and run without a GPU).  Each
 * query takes the arguments of its entry point that the decision depends on, validates them like the entry point and returns 0
 * with the plan filled, or the BYA_ERR_* that rejects the arguments with the plan untouched (plan == NULL: BYA_ERR_SHAPE).  The
 * launchers take their decision from the same functions.
 *   bya_linear_small_m_plan:     kernel = rows of the instantiation (2 for M <= 2, else 8); grid = ceil(N / 4) workgroups of
 *                                four waves, one wave per output column; items = N; items_per_round = the 512 elements of K the
 *                                64 lanes take per trip; rounds = ceil(K / 512) trips of lane 0
 *   bya_router_scores_plan:      kernel = BYA_ROUTER_SCORES_*; items = ceil(N / 16) 16-token tiles per identity;
 *                                WAVE: grid = ceil(items n_id / 4), one wave per tile (items_per_round = items, rounds = 1);
 *                                LDS (N >= 4096, n_id <= 256, BYA_REF_ROUTER_SCORES_WAVE not set): grid = 256 / n_id * n_id
 *                                workgroups of eight waves, grid / n_id per identity; items_per_round = 8 grid / n_id tiles of one
 *                                identity per round of the waves' walk; rounds = ceil(items / items_per_round)
 *   bya_act_add_plan:            items = n / 8 16-byte pieces; grid = min(4096, ceil(items / 256)); items_per_round = 256 grid;
 *                                rounds = ceil(items / items_per_round) trips of the grid-stride loop
 *   bya_cfg_scheduler_step_plan: items = n elements; grid = min(8192, ceil(n / 256)); items_per_round = 256 grid; rounds as above
 */
#define BYA_ROUTER_SCORES_WAVE 0
#define BYA_ROUTER_SCORES_LDS 1
typedef struct bya_step_plan_info {
    int32_t kernel;
    int32_t grid;             /* workgroups */
    int32_t rounds;
    int32_t reserved;
    int64_t items;
    int64_t items_per_round;
} bya_step_plan_info;
int bya_linear_small_m_plan(const void* x, const void* W, const void* out, int32_t M, int32_t N, int32_t K, int32_t act_out,
                            bya_step_plan_info* plan);

/* Sinusoidal timestep features (diffusers Timesteps, flip_sin_to_cos, shift 0) in fp32 then rounded
 * to bf16: out[b, 0:dim/2] = cos(t*w_k), out[b, dim/2:] = sin(t*w_k)  (models/transformer.py:679-685). */
int bya_timestep_features(const int64_t* timesteps, void* out, int32_t batch, int32_t dim,
                          int32_t flip_sin_to_cos, float freq_shift, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LayerNorm over the last dim D (fp32 statistics), optional affine (w,b), optional AdaLN modulation
 *   y = (LN(x)*w + b) * (1 + scale[z][type(row)]) + shift[z][type(row)]
 * rows r < split use (shift0,scale0) else (shift1,scale1); mod pointers NULL = plain LayerNorm.
 * Replaces CogVideoXLayerNormZero / AdaLayerNorm / nn.LayerNorm call sites
 * (models/transformer.py:233,251,944,948; models/router.py:247-248,380-393,475-491;
 * models/audio_model.py:249).  D in {512, 768, 1024, 2048, 3072}; rows_per_batch rows per z.
 * Affine + modulation are evaluated as ONE fma, y = fma(LN(x), w (1 + scale), b (1 + scale) + shift), in every kernel
 * behind this entry point (at D = 3072 with w and b a wave keeps those two vectors in registers and walks several rows),
 * so a result does not depend on how the rows are cut into launches.
 * ---------------------------------------------------------------------------------------------
 * Statistics: centred second pass in fp32 on the row held in registers (mean = sum / D by a true division); within half a bf16
 * ulp of F.layer_norm in fp32 on every row distribution of tests/cond_norm.py, offset (|mean| / spread up to 256), near-constant
 * and constant rows included.
 */
int bya_layernorm(const void* x, void* y, const void* w, const void* b, const void* shift0, const void* scale0,
                  const void* shift1, const void* scale1, int64_t rows_per_batch, int32_t batch, int32_t D,
                  int64_t ldx, int64_t ldy, int64_t x_batch_stride, int64_t y_batch_stride,
                  int64_t mod_batch_stride, int64_t split, float eps, hipStream_t stream);
/* What a bya_layernorm / bya_layernorm_fp8 / bya_layernorm_mx launch runs (host-side query like bya_gemm_bf16_plan: validates
 * like the entry point, launches nothing, needs no GPU; the launchers take every decision from the same function).  The
 * arguments are bya_layernorm's, with y the output of the kind asked for: the bf16 matrix, or the fp8 / MX code matrix (ldy
 * and y_batch_stride then in bytes; the scale arrays play no part in the plan).
 *   kernel GENERIC: layernorm_kernel<vec, nv> (D = 64 * vec * nv), one row per wave, parameters re-read for every row; the
 *                   fp8 / MX outputs are instances of it;
 *   kernel ROWS:    layernorm_adaln_rows_kernel<nv, modulated> (D = 3072 with w and b, bf16 output, unless the reference form
 *                   BYA_REF_LN_GENERIC is set): a wave owns rows_per_wave = max(2, ceil(rows / 4096)) consecutive rows of the
 *                   batch-major row enumeration and keeps the parameter vectors in registers.
 * waves = ceil(rows / rows_per_wave) waves have work, four to a workgroup. */
#define BYA_LN_OUT_BF16 0
#define BYA_LN_OUT_FP8 1
#define BYA_LN_OUT_MX_E4M3 2
#define BYA_LN_OUT_MX_E2M3 3
#define BYA_LN_KERNEL_GENERIC 0
#define BYA_LN_KERNEL_ROWS 1
typedef struct bya_layernorm_plan_info {
    int32_t kernel;         /* BYA_LN_KERNEL_* */
    int32_t vec, nv;        /* bf16 elements per lane access, accesses per lane and row */
    int32_t modulated;      /* shift / scale are applied (ROWS: the MOD template instance) */
    int32_t rows_per_wave;  /* 1 for the generic kernel */
    int32_t grid;           /* workgroups of 4 waves */
    int64_t waves;
} bya_layernorm_plan_info;
int bya_layernorm_plan(const void* x, const void* y, const void* w, const void* b, const void* shift0, const void* scale0,
                       const void* shift1, const void* scale1, int64_t rows_per_batch, int32_t batch, int32_t D, int64_t ldx,
                       int64_t ldy, int64_t x_batch_stride, int64_t y_batch_stride, int64_t mod_batch_stride, int64_t split,
                       int32_t out_kind, bya_layernorm_plan_info* plan);

/* Per-head LayerNorm(64, eps, affine) on q and k followed by interleaved-pair RoPE on rows >= text_rows
 * (diffusers CogVideoXAttnProcessor2_0 + apply_rotary_emb; models/transformer.py:204-208).  In place.
 * q,k: [batch, S, heads*64] with row stride ld; cos,sin: fp32 [S - text_rows, 64].
 * k_scale (0 or 1 = off): the finished k is multiplied by it in fp32 before its single rounding to bf16 -- the engine
 * folds softmax_scale*log2(e) into k here so that bya_attn_fwd can run with scores_prescaled = 1.
 * q or k (not both) may be NULL: only the other tensor is processed (the sharded step norms q, starts q's exchange on
 * the RCCL stream and norms k underneath it).
 * stats (may be NULL): fp32 [stats_slots][2][batch * heads], zero-filled by the caller before the launch.  The kernel
 * raises (atomic maximum on the bit pattern) entry [blockIdx % stats_slots][0 = q, 1 = k][z * heads + head] to the squared
 * Euclidean norm of every finished, bf16-rounded head row it writes: max over the slots = max ||q||^2 / max ||k||^2 per
 * (batch, head) -- the data-dependent score bound  |q . k| <= max||q|| max||k||  that bya_attn_fwd reads from device
 * memory (bya_attn_desc.bound_dev) when the worst case over the LayerNorm's parameters is too large to be useful.
 * Statistics: centred second pass in fp32 over the 64 values of a head (qknorm_math.h, shared with the fused q|k|v epilogues);
 * within half a bf16 ulp of the fp32 definition on offset, near-constant and constant head rows (tests/test_norm_cond_gpu.py).
 */
int bya_qknorm_rope(void* q, void* k, const void* qw, const void* qb, const void* kw, const void* kb,
                    const float* cos, const float* sin, int32_t batch, int32_t S, int32_t heads, int64_t ld,
                    int64_t batch_stride, int32_t text_rows, float eps, float k_scale, float* stats, int32_t stats_slots,
                    hipStream_t stream);
/* What a bya_qknorm_rope launch runs (host-side query): the STATS or the plain instance, `only` (0: q and k, 1: q alone,
 * 2: k alone), the (row, head) pairs -- enumerated row-major over all batches, all of q's before k's -- the waves of eight
 * pairs (one 8-lane group each) and the workgroups of four waves. */
typedef struct bya_qknorm_rope_plan_info {
    int32_t stats;          /* 1: qknorm_rope_kernel<true> */
    int32_t only;
    int32_t grid;
    int32_t slots;          /* copies of the statistics table (0 without stats) */
    int64_t pairs;
    int64_t waves;
} bya_qknorm_rope_plan_info;
int bya_qknorm_rope_plan(const void* q, const void* k, const void* qw, const void* qb, const void* kw, const void* kb,
                         const float* cos, const float* sin, int32_t batch, int32_t S, int32_t heads, int64_t ld,
                         int64_t batch_stride, int32_t text_rows, const float* stats, int32_t stats_slots,
                         bya_qknorm_rope_plan_info* plan);

/* ---------------------------------------------------------------------------------------------
 * Flash attention forward, head_dim 64 or 128, no mask, fp32 online softmax, bf16 P.V on MFMA.
 *   O[b1,b2,i,h,:] = softmax_j( scale * Q[b1,b2,i,h,:].K[b1,b2,j,h,:] ) V[b1,b2,j,h,:]
 * Two-level batch (b1 < nb1, b2 < nb2) with independent element strides so one kernel serves: the joint
 * text+video self-attention (F.scaled_dot_product_attention inside CogVideoXAttnProcessor2_0,
 * models/transformer.py:208), the router's spatial attention (models/router.py:476), the perceiver
 * face cross-attention (models/router.py:264-270; q shared by both ids) and the per-frame audio
 * cross-attention (models/audio_model.py:253-256).
 * --------------------------------------------------------------------------------------------- */
typedef struct bya_attn_desc {
    int32_t head_dim;       /* 64 or 128 */
    int32_t heads;
    int32_t nb1, nb2;
    int32_t Sq, Skv;
    int64_t q_s1, q_s2, q_row;   /* element strides: batch level 1, level 2, sequence row */
    int64_t k_s1, k_s2, k_row;
    int64_t v_s1, v_s2, v_row;
    int64_t o_s1, o_s2, o_row;
    float scale;
    int32_t scores_prescaled;   /* 1: q.k is already scale*log2(e)*(q.k) (folded into k upstream); scale is ignored;
                                   head_dim 64 only.  Saves one multiply per score in the VALU-bound softmax. */
    float score_bound;          /* > 0 (with scores_prescaled): the caller GUARANTEES |score| <= score_bound in exp2
                                   units for every (q, k) pair, e.g. because q and k come out of a LayerNorm with known
                                   weights (||q|| <= 8 max|gamma| + ||beta|| at head_dim 64; RoPE is a rotation).  The
                                   softmax then uses no running maximum at all (P = exp2(s): mathematically identical,
                                   shift invariance; every P and every row sum stays a normal fp32 / bf16 number while
                                   |s| <= 90) -- bounds above BYA_ATTN_BOUND_LIMIT are ignored.  0 = unknown. */
    /* Data-dependent bound (head_dim 64, scores_prescaled; NULL = off): squared norms written by bya_qknorm_rope's `stats`,
       fp32 [bound_slots][2][bound_heads]; this launch's (batch, head) index bh reads column bound_bh0 + bh.  Per (batch,
       head) the kernel takes B = sqrt(max_slots q2 * max_slots k2); where B <= BYA_ATTN_BOUND_LIMIT the static kernel runs,
       elsewhere it leaves the head alone, sets fallback_flags[bh] (int32 [nb1 * nb2 * heads], written for EVERY bh, no reset
       needed) and the running-maximum kernel, launched right behind it, computes exactly the flagged heads. */
    const float* bound_dev;
    int32_t bound_slots, bound_heads, bound_bh0;
    int32_t* fallback_flags;
} bya_attn_desc;
#define BYA_ATTN_BOUND_LIMIT 90.0f

int bya_attn_fwd(const void* q, const void* k, const void* v, void* o, const bya_attn_desc* desc,
                 hipStream_t stream);

/* Which softmax variant bya_attn_fwd runs for a descriptor (host-side query, launches nothing): the joint attention
 * silently falls back from the static-bound kernel to the running-maximum kernel when score_bound is above the limit, and callers
 * (tests, bench.py) need to say which one they measured.  Negative = the descriptor is rejected. */
#define BYA_ATTN_D64_RUNNING_MAX 0   /* online softmax, scores scaled in the kernel */
#define BYA_ATTN_D64_PRESCALED 1     /* online softmax, scores already in exp2 units */
#define BYA_ATTN_D64_STATIC_BOUND 2  /* (retired in round 5: the two-block static-bound kernel; never returned) */
#define BYA_ATTN_D128 3
#define BYA_ATTN_D64_STATIC_BOUND_W4 4  /* P = exp2(s), |s| <= score_bound <= 90, on the one-wave-per-SIMD hand-placed kernel (csrc/attn_w4.hip) */
#define BYA_ATTN_D64_DEVICE_BOUND_W4 5  /* the same kernel under the data-dependent bound (bound_dev), per-head running-maximum fallback */
int bya_attn_variant(const bya_attn_desc* desc);

/* What a bya_attn_fwd launch runs (host-side query like bya_gemm_bf16_plan: launches nothing, needs no GPU; the launcher
 * calls the same decision functions).  `o` is the output address of the launch (it decides the store width).
 * workspace_assumed: 1 / 0 = answer as if a stream-K workspace were / were not registered, -1 = as the current device's
 * registration stands.  Returns what bya_attn_fwd would return before launching; the plan is untouched on rejection. */
typedef struct bya_attn_plan_info {
    int32_t variant;        /* BYA_ATTN_*, equal to bya_attn_variant(desc) */
    int32_t grid;           /* workgroups of the (first) launch */
    int32_t q_tile;         /* query rows per workgroup: 128, or 512 on the hand-placed kernel */
    int32_t stream_k;       /* 1: 256 persistent workgroups with the leftover items cut along the keys */
    int32_t sk_rem;         /* stream_k: leftover items of XCD 0 after its whole rounds (mains) */
    int32_t sk_cut;         /* stream_k: the mains take key tiles [0, sk_cut) of a leftover item, helpers the rest */
    int32_t o_wide;         /* 1: the epilogue stores 16 bytes per lane, 0: 8 bytes */
    int32_t second_launch;  /* 1: the running-maximum kernel follows for the flagged heads (device bound) */
} bya_attn_plan_info;
int bya_attn_plan(const bya_attn_desc* desc, const void* o, int32_t workspace_assumed, bya_attn_plan_info* plan);

/* bya_attn_fwd followed by bya_quantize_mx(out_fmt) on its [rows, heads * 64] output, without the bf16 matrix: the
 * epilogue of every head_dim-64 kernel (running maximum plain / prescaled, static bound with and without stream-K, device
 * bound incl. its second launch for the flagged heads) rounds acc / l to bf16 as bya_attn_fwd stores it, takes the |max| of
 * each 32-column half of a head over the lane pair that holds it, and writes the MX codes and one e8m0 scale byte per
 * (row, head, half) -- byte for byte what the two launches write (see "MX weights" for the formats).
 *   codes:  byte (head * 64 + 32 h) * bits / 8 of a row holds half h of the head (32 bytes as e4m3, 24 as e2m3);
 *   scales: byte 2 * head + h of a row.
 * Row r of batch (b1, b2) starts at  codes + b1 * c_s1 + b2 * c_s2 + r * c_row  and  scales + b1 * sc_s1 + b2 * sc_s2 +
 * r * sc_row -- all strides in BYTES.  Rows >= Sq and bytes outside the heads' code / scale bytes are never written.
 * desc is bya_attn_fwd's descriptor with o_s1 = o_s2 = o_row = 0 (there is no bf16 output; anything else: BYA_ERR_SHAPE).
 * The kernel / stream-K / second-launch decisions are bya_attn_fwd's; bya_attn_mx_plan answers them (o_wide is 0).
 * Refused before any launch: head_dim != 64, out_fmt other than e4m3 (0) / e2m3 (2) -> BYA_ERR_UNSUPPORTED; codes or a
 * code stride not a multiple of 4 bytes (a lane stores 16 or 12 bytes as dwords; scale bytes are stored one by one and
 * need no alignment) -> BYA_ERR_ALIGN; c_row < heads * 64 * bits / 8, sc_row < 2 * heads, a negative batch stride or
 * anything bya_attn_fwd refuses as a shape -> BYA_ERR_SHAPE. */
int bya_attn_fwd_mx(const void* q, const void* k, const void* v, void* codes, void* scales, const bya_attn_desc* desc,
                    int32_t out_fmt, int64_t c_s1, int64_t c_s2, int64_t c_row, int64_t sc_s1, int64_t sc_s2, int64_t sc_row,
                    hipStream_t stream);
int bya_attn_mx_plan(const bya_attn_desc* desc, const void* codes, const void* scales, int32_t out_fmt, int64_t c_s1,
                     int64_t c_s2, int64_t c_row, int64_t sc_s1, int64_t sc_s2, int64_t sc_row, int32_t workspace_assumed,
                     bya_attn_plan_info* plan);

/* Optional stream-K workspace of the static-bound joint-attention kernel (BYA_ATTN_D64_STATIC_BOUND_W4): device memory
 * owned by the caller, 256-byte aligned, at least bya_attn_workspace_bytes (69 MB), ZERO-FILLED once; one per DEVICE, used
 * by launches enqueued under the current device, which must be ordered on one stream.  NULL unregisters.  With it, a
 * bya_attn_fwd launch whose (batch x head, 512-row q-tile) items do not fill whole rounds of 256 CUs (49 x 480 x 720:
 * 1680 items = 6.56 rounds that cost 7; a rank's 6 heads of an 8-GPU step: 210 items on 256 CUs) runs as 256 persistent
 * workgroups: whole rounds item by item, then the leftover items cut at ONE key tile -- "mains" take the key prefix of an
 * item each, the remaining workgroups share the key suffixes -- and an item is completed by adding the fp32 partial (O, l)
 * of its suffix pieces, exchanged through this workspace, to the prefix (partials of the static-bound softmax are
 * additive).  Results equal the one-workgroup-per-item form up to fp32 summation order at the cut items.
 * bya_attn_workspace_status: number of hand-offs that timed out (~1 s; 0 on a healthy run), synchronises `stream`.  (No
 * reference counterpart: scheduling detail of F.scaled_dot_product_attention, models/transformer.py:200-209 via diffusers
 * CogVideoXAttnProcessor2_0.) */
int bya_set_attn_workspace(void* ws, int64_t bytes);
int bya_attn_workspace_bytes(int64_t* bytes);
int bya_attn_workspace_status(int32_t* timeouts, hipStream_t stream);

/* Cross-attention onto at most 64 keys per identity with the router's masked combine in its epilogue:
 *   z[g, n, :] = sum_id w[g n, id] * softmax(q[g, n] . K[id, g]^T * scale) V[id, g]      (fp32 mix, one rounding to bf16)
 * The audio cross-attention (models/audio_model.py:247-258: 32 audio tokens per latent frame g and identity) and the face
 * Perceiver cross-attention (models/router.py:255-270: 32 face tokens per identity), each followed in the reference by the
 * masked combine of models/transformer.py:821-832 / 895-936 AFTER the (linear) output projection: the engine mixes first
 * and projects once.  r: routing logits bf16 [n_grp * Sq, n_id]; af: NULL = face weights (w = r), else the audio-to-face
 * matrix bf16 [n_id, n_id] (w as in bya_masked_combine mode 1).  wsum (optional, fp32 [n_grp * Sq]) = sum_id w, the row scale
 * of the projection's bias.  q rows are shared by all identities.  Element strides; head h of a row starts at h * head_dim.
 * Up to 32 keys (both callers) with z 16-byte aligned: the K / V of every identity stay in LDS for a (group, head) and z is
 * stored as whole head segments; otherwise one 128-row tile per workgroup on 64-key tiles -- the same bits either way. */
typedef struct bya_attn_mix_desc {
    int32_t head_dim, heads, n_id, n_grp, Sq, Skv;
    int64_t q_grp, q_row, k_id, k_grp, k_row, v_id, v_grp, v_row, z_grp, z_row;
    float scale;
} bya_attn_mix_desc;
int bya_attn_kv_mix(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                    const bya_attn_mix_desc* desc, hipStream_t stream);
/* Which form a bya_attn_kv_mix launch with this z, af (NULL or not) and descriptor runs (host-side query). */
#define BYA_KV_MIX_MIX32 0      /* <= 32 keys: K / V of every identity resident in LDS, one workgroup per (group, head, row chunk) */
#define BYA_KV_MIX_ONE_TILE 1   /* one 128-row query tile per workgroup on a 64-key tile */
typedef struct bya_attn_kv_mix_plan_info {
    int32_t form;           /* BYA_KV_MIX_* */
    int32_t head_dim;
    int32_t grid;
    int32_t row_chunks;     /* workgroups per (group, head) */
    int32_t lds_bytes;
    int32_t big_lds;        /* 1: more than 64 KiB of LDS, the launch opts in (four identities at head_dim 128) */
} bya_attn_kv_mix_plan_info;
int bya_attn_kv_mix_plan(const void* z, const void* af, const bya_attn_mix_desc* desc, bya_attn_kv_mix_plan_info* plan);

/* bya_attn_kv_mix followed by bya_quantize_mx(out_fmt) on its [n_grp * Sq, heads * head_dim] output, without the bf16 matrix:
 * the operand of the cross-attention's output projection as MX codes, written by the <= 32-key form's epilogue.  There the
 * mixed z passes through the wave's LDS patch and is re-read row-major, 8 consecutive bf16 columns per lane, so a 32-column
 * MX block of a row is one aligned lane quad: |max| over the quad by cross-lane moves, then the standalone quantiser's
 * arithmetic on the bf16 value of the patch -- byte for byte what the two launches write (see "MX weights" for the formats).
 *   codes:  byte (head * head_dim + 32 j) * bits / 8 of a row holds block j of the head (32 bytes as e4m3, 24 as e2m3);
 *   scales: byte head * head_dim / 32 + j of a row.
 * Row n of group g starts at  codes + g * c_grp + n * c_row  and  scales + g * sc_grp + n * sc_row  -- strides in BYTES.
 * Rows >= Sq and bytes outside the heads' code / scale bytes are never written; wsum is written as by bya_attn_kv_mix.
 * desc is bya_attn_kv_mix's descriptor with z_grp = z_row = 0 (there is no bf16 output; anything else: BYA_ERR_SHAPE).
 * Refused before any launch: out_fmt other than e4m3 (0) / e2m3 (2), Skv > 32 or reference form BYA_REF_KV_MIX_GENERIC set
 * (the MX epilogue exists on the BYA_KV_MIX_MIX32 form alone: the caller then issues the two launches) -> BYA_ERR_UNSUPPORTED;
 * codes or a code stride not a multiple of 4 bytes -> BYA_ERR_ALIGN; c_row < heads * head_dim * bits / 8, sc_row < heads *
 * head_dim / 32, a negative group stride or anything bya_attn_kv_mix refuses -> BYA_ERR_SHAPE.  bya_attn_kv_mix_mx_plan
 * answers with bya_attn_kv_mix_plan's struct: the same grid, row chunks and LDS rule as the bf16 launch (form = MIX32). */
int bya_attn_kv_mix_mx(const void* q, const void* k, const void* v, const void* r, const void* af, void* codes, void* scales,
                       float* wsum, const bya_attn_mix_desc* desc, int32_t out_fmt, int64_t c_grp, int64_t c_row,
                       int64_t sc_grp, int64_t sc_row, hipStream_t stream);
int bya_attn_kv_mix_mx_plan(const void* codes, const void* scales, const void* af, const bya_attn_mix_desc* desc,
                            int32_t out_fmt, int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row,
                            bya_attn_kv_mix_plan_info* plan);

/* bya_attn_kv_mix / bya_attn_kv_mix_mx over a SEGMENT TABLE: one launch for groups of unequal length that start anywhere, e.g. the
 * partial latent frames a sequence-parallel rank holds (one bya_attn_kv_mix launch each otherwise).  The table is read on the
 * host and travels BY VALUE in the kernel's arguments: no device memory, so a captured graph carries it.
 *   desc is bya_attn_kv_mix's descriptor, read as follows: n_grp = the K / V groups that can be addressed (0 <= grp[i] < n_grp);
 *   Sq = the TOTAL row count of q, r, z and wsum (start[i] + len[i] <= Sq); q_grp = z_grp = 0, and c_grp = sc_grp = 0 for the MX
 *   entry.  Row n is addressed directly: q + n * q_row, r[n, :], z + n * z_row, wsum[n], codes + n * c_row, scales + n * sc_row.
 *   Segment i computes rows [start[i], start[i] + len[i]) against K[id, grp[i]] and V[id, grp[i]].
 *   Rows outside every segment are never read as queries and nothing is written for them: not z, not wsum, not codes, not
 *   scales.  Segments are in ascending order and do not overlap (start[i] + len[i] <= start[i + 1]); gaps are allowed.
 * Every row gets the arithmetic of bya_attn_kv_mix (the kernel body is the same code): the output is byte for byte that of one
 * bya_attn_kv_mix / bya_attn_kv_mix_mx launch per segment (n_grp = 1, Sq = len[i], pointers advanced by start[i] rows).
 * Refused before any launch.  BYA_ERR_SHAPE: seg NULL, n outside 1 .. BYA_MIX_MAX_SEGMENTS, a len <= 0, a grp outside
 * [0, n_grp), rows past Sq, overlapping or descending segments, a non-zero group stride on q, z, codes or scales, anything
 * bya_attn_kv_mix / bya_attn_kv_mix_mx refuses.  BYA_ERR_UNSUPPORTED -- the segment form exists on the BYA_KV_MIX_MIX32 form with
 * head_dim 64 alone, the caller then issues the launches per segment --: Skv > 32, reference form BYA_REF_KV_MIX_GENERIC set, z
 * not 16-byte aligned or z_row not a multiple of 8, head_dim 128.
 * The plan queries answer with bya_attn_kv_mix_plan's struct: form = BYA_KV_MIX_MIX32, row_chunks = the existing rule
 * ceil(ceil(L / 32) / 12) for the LONGEST segment's L, grid = row_chunks * heads * n (one workgroup per (segment, head, row
 * chunk); one whose share of a shorter segment's 32-row tiles is empty leaves at once), lds_bytes as for bya_attn_kv_mix; the
 * plan is untouched on rejection. */
#define BYA_MIX_MAX_SEGMENTS 16
typedef struct bya_attn_mix_segments {
    int32_t n;                                   /* 1 .. BYA_MIX_MAX_SEGMENTS */
    int32_t grp[BYA_MIX_MAX_SEGMENTS];           /* K / V group (frame) the segment's rows attend to */
    int32_t start[BYA_MIX_MAX_SEGMENTS];         /* first row of the segment in q / r / z / wsum */
    int32_t len[BYA_MIX_MAX_SEGMENTS];           /* rows, > 0 */
} bya_attn_mix_segments;
int bya_attn_kv_mix_seg(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                        const bya_attn_mix_desc* desc, const bya_attn_mix_segments* seg, hipStream_t stream);
int bya_attn_kv_mix_seg_plan(const void* z, const void* af, const bya_attn_mix_desc* desc, const bya_attn_mix_segments* seg,
                             bya_attn_kv_mix_plan_info* plan);
int bya_attn_kv_mix_mx_seg(const void* q, const void* k, const void* v, const void* r, const void* af, void* codes, void* scales,
                           float* wsum, const bya_attn_mix_desc* desc, const bya_attn_mix_segments* seg, int32_t out_fmt,
                           int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row, hipStream_t stream);
int bya_attn_kv_mix_mx_seg_plan(const void* codes, const void* scales, const void* af, const bya_attn_mix_desc* desc,
                                const bya_attn_mix_segments* seg, int32_t out_fmt, int64_t c_grp, int64_t c_row, int64_t sc_grp,
                                int64_t sc_row, bya_attn_kv_mix_plan_info* plan);

/* bya_attn_kv_mix / bya_attn_kv_mix_mx over a BATCH of samples: one launch where the caller issued one per sample (the
 * [uncond, cond] pair of a guided step).  The arguments are the single-sample entry's, for sample 0; `batch` (by value: no device
 * memory, a captured graph carries it) holds the sample count n and, per pointer that differs between samples, the distance from
 * one sample to the next: in ELEMENTS of the pointer's type for q, k, v, r, af, z (bf16) and wsum (fp32), in BYTES for codes and
 * scales.  A stride of 0 shares the operand (one forcing tensor r for the whole batch); the af stride is ignored where af is
 * NULL.  The wsum stride is checked (not negative, no overlap) whenever wsum is given OR the stride is not 0 -- the plan queries
 * see no wsum pointer, and the entries follow the same rule; pass 0 without wsum.  The descriptor is common to the samples.
 * The sample is a second grid dimension of the single-sample kernel body: a workgroup's (group, head, row chunk) within its sample
 * is the single-sample launch's, so every row's arithmetic -- and with it wsum and the MX scale bytes -- does not depend on n.
 * The output is byte for byte that of n single-sample launches with the pointers advanced by the strides; bytes those never write
 * (rows >= Sq, bytes outside a head's code / scale bytes, anything between the samples) are never written.
 * Refused before any launch: anything the single-sample entry refuses, with its code; n < 1 (or > 65535), a negative stride, an
 * output (z, codes, scales, wsum by the rule above) stride smaller than what one sample covers of it when n > 1 -- samples would
 * overlap --, a negative output row / group stride -> BYA_ERR_SHAPE; a q / k / v stride that is no multiple of 8 elements, a z
 * stride that is no multiple of 4, a codes stride that is no multiple of 4 bytes -> BYA_ERR_ALIGN; the generic form (Skv > 32,
 * BYA_REF_KV_MIX_GENERIC, a z that is not 16-byte aligned in every sample: z, z_grp, z_row or the z stride no multiple of 8) ->
 * BYA_ERR_UNSUPPORTED, as the segment form: the caller then issues the launches per sample.
 * The plan queries answer with bya_attn_kv_mix_plan's struct: the single-sample launch's form (BYA_KV_MIX_MIX32), row_chunks,
 * lds_bytes and big_lds, and grid = the single-sample grid * n; untouched on rejection. */
typedef struct bya_attn_mix_samples {
    int32_t n;                                   /* samples, >= 1 */
    int32_t reserved;
    int64_t q, k, v, r, af, z, wsum;             /* elements from one sample to the next */
} bya_attn_mix_samples;
typedef struct bya_attn_mix_mx_samples {
    int32_t n;
    int32_t reserved;
    int64_t q, k, v, r, af, codes, scales, wsum; /* codes, scales: bytes */
} bya_attn_mix_mx_samples;
int bya_attn_kv_mix_batch(const void* q, const void* k, const void* v, const void* r, const void* af, void* z, float* wsum,
                          const bya_attn_mix_desc* desc, bya_attn_mix_samples batch, hipStream_t stream);
int bya_attn_kv_mix_batch_plan(const void* z, const void* af, const bya_attn_mix_desc* desc, bya_attn_mix_samples batch,
                               bya_attn_kv_mix_plan_info* plan);
int bya_attn_kv_mix_mx_batch(const void* q, const void* k, const void* v, const void* r, const void* af, void* codes, void* scales,
                             float* wsum, const bya_attn_mix_desc* desc, int32_t out_fmt, int64_t c_grp, int64_t c_row,
                             int64_t sc_grp, int64_t sc_row, bya_attn_mix_mx_samples batch, hipStream_t stream);
int bya_attn_kv_mix_mx_batch_plan(const void* codes, const void* scales, const void* af, const bya_attn_mix_desc* desc,
                                  int32_t out_fmt, int64_t c_grp, int64_t c_row, int64_t sc_grp, int64_t sc_row,
                                  bya_attn_mix_mx_samples batch, bya_attn_kv_mix_plan_info* plan);

/* Tiny-sequence self-attention (sequence length L <= 16, head_dim 64) used by the router's temporal
 * (L = frames) and multi-ID (L = ids) attentions (models/router.py:482,488).  Element e of sequence
 * `g` lives at row  g_outer(g)*outer_stride + e*seq_stride + g_inner(g)  of the [rows, ld] matrices,
 * with g = g_outer * n_inner + g_inner. */
int bya_attn_tiny(const void* q, const void* k, const void* v, void* o, int32_t L, int32_t heads,
                  int64_t n_outer, int64_t n_inner, int64_t outer_stride, int64_t seq_stride, int64_t ld_qkv,
                  int64_t ld_o, float scale, hipStream_t stream);
/* Which of the eight kernel instances a bya_attn_tiny launch runs (host-side query): 8 heads per wave with the sequence in
 * registers for L in {2, 3, 13, 25} when heads % 8 == 0 and pointers and row strides are 16-byte aligned, else one wave per
 * (sequence, head) with L rounded up to 2 / 4 / 16 / 32. */
#define BYA_TINY8_2 0
#define BYA_TINY8_3 1
#define BYA_TINY8_13 2
#define BYA_TINY8_25 3
#define BYA_TINY_GENERIC_2 4
#define BYA_TINY_GENERIC_4 5
#define BYA_TINY_GENERIC_16 6
#define BYA_TINY_GENERIC_32 7
typedef struct bya_attn_tiny_plan_info {
    int32_t instance;       /* BYA_TINY* */
    int32_t grid;           /* workgroups of 4 waves */
    int64_t waves;          /* waves with work (the last workgroup may be partly idle) */
} bya_attn_tiny_plan_info;
int bya_attn_tiny_plan(const void* q, const void* k, const void* v, const void* o, int32_t L, int32_t heads, int64_t n_outer,
                       int64_t n_inner, int64_t ld_qkv, int64_t ld_o, bya_attn_tiny_plan_info* plan);

/* ---------------------------------------------------------------------------------------------
 * Embedding-Router specific kernels (models/router.py:364-411).
 * router_scores: s[id,n,tok*heads+h] = sum_d qr[n,h*128+d] * kr[id,tok,h*128+d]; LayerNorm(512, w,b);
 *                + pos_emb[n]  ->  out[id,n,512]
 * router_head:   r[n,id] = sigmoid(x[id,n,:].w + b)  ->  [N, n_id]  (the [1,N,n_id] routing logits)
 * (router_scores keeps an identity's 32 keys in LDS from 4096 tokens on; same bits as the per-wave form below that.)
 * ---------------------------------------------------------------------------------------------
 * Statistics of the LayerNorm(512): centred second pass in fp32 on the accumulators, in both kernels; no restriction on the rows
 * (tests/test_norm_cond_gpu.py).
 */
int bya_router_scores(const void* qr, const void* kr, const void* ln_w, const void* ln_b, const void* pos_emb,
                      void* out, int32_t n_id, int64_t N, int32_t heads, int32_t face_tokens, float eps,
                      hipStream_t stream);
int bya_router_scores_plan(const void* qr, const void* kr, const void* ln_w, const void* ln_b, const void* pos_emb,
                           const void* out, int32_t n_id, int64_t N, int32_t heads, int32_t face_tokens,
                           bya_step_plan_info* plan);           /* see bya_step_plan_info */
int bya_router_head(const void* x, const void* w, const void* b, void* r, int32_t n_id, int64_t N, int32_t D,
                    hipStream_t stream);
/* bya_router_scores / bya_router_head over a BATCH of samples, as bya_attn_kv_mix_batch: the single-sample entry's arguments for
 * sample 0 plus, by value, n and the distance in bf16 ELEMENTS from one sample to the next of each pointer that differs per
 * sample (qr, kr, out; x, r); 0 shares an input.  The sample is a second grid dimension of the same kernels (a single-sample
 * launch is the batch of one): a sample's tiles are walked as there, the output is byte for byte that of n single-sample launches
 * on the advanced pointers and nothing else is written.
 * Refused before any launch: anything the single-sample entry refuses, with its code; n < 1 (or > 65535), a negative stride, an
 * output stride (out: below n_id * N * 512; r: below N * n_id) that makes samples overlap when n > 1 -> BYA_ERR_SHAPE; a qr, kr,
 * out or x stride that is no multiple of 8 elements -> BYA_ERR_ALIGN.
 * Plan queries (bya_step_plan_info; untouched on rejection): bya_router_scores_batch_plan = bya_router_scores_plan's answer for one
 * sample -- kernel, rounds, items, items_per_round -- with grid = its grid * n; bya_router_head_batch_plan: kernel = 0, items =
 * items_per_round = N * n_id (one wave per identity and row), rounds = 1, grid = ceil(items / 4) * n. */
typedef struct bya_router_scores_samples {
    int32_t n;                                   /* samples, >= 1 */
    int32_t reserved;
    int64_t qr, kr, out;
} bya_router_scores_samples;
typedef struct bya_router_head_samples {
    int32_t n;
    int32_t reserved;
    int64_t x, r;
} bya_router_head_samples;
int bya_router_scores_batch(const void* qr, const void* kr, const void* ln_w, const void* ln_b, const void* pos_emb, void* out,
                            int32_t n_id, int64_t N, int32_t heads, int32_t face_tokens, float eps,
                            bya_router_scores_samples batch, hipStream_t stream);
int bya_router_scores_batch_plan(const void* qr, const void* kr, const void* ln_w, const void* ln_b, const void* pos_emb,
                                 const void* out, int32_t n_id, int64_t N, int32_t heads, int32_t face_tokens,
                                 bya_router_scores_samples batch, bya_step_plan_info* plan);
int bya_router_head_batch(const void* x, const void* w, const void* b, void* r, int32_t n_id, int64_t N, int32_t D,
                          bya_router_head_samples batch, hipStream_t stream);
int bya_router_head_batch_plan(const void* x, const void* w, const void* b, const void* r, int32_t n_id, int64_t N, int32_t D,
                               bya_router_head_samples batch, bya_step_plan_info* plan);

/* Forcing override (models/transformer.py:813-819): out[t,r,id] = max_t' forcing[t',r,id]. Bit-exact. */
int bya_forcing_max_over_frames(const void* forcing, void* out, int32_t frames, int64_t per_frame,
                                int32_t n_id, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Masked combines (models/transformer.py:821-822,831-832 and 860-863,895-900,925-926,935-936).
 *  mode 0 (face):  x[b,n,:] += alpha * sum_id r[b][n,id] * feat[b,id,n,:]
 *  mode 1 (audio): av[n,i] = bf16(sum_j af[b,i,j]*r[b][n,j]); w[n,id] = bf16(1 - av[n,1-id]);
 *                  x[b,n,:] += sum_id w[n,id] * feat[b,id,n,:]
 *                  n_id in 3..4 (the reference hard-codes two streams; build-defined): af is [batch, n_id, n_id] and
 *                  w[n,a] = prod_{b != a} bf16(1 - av[n,b]), every product rounded to bf16 (two streams: same bits)
 * r: [batch or 1, N, n_id] (r_batch_stride 0 = shared forcing mask); feat [batch, n_id, N, D]. In place.
 * n_id in 1..4; mode 1 needs at least two streams: mode == 1 with n_id < 2 is BYA_ERR_UNSUPPORTED, here and in
 * bya_routed_mix, before any launch (the weights of one stream alone are not defined; bya_attn_kv_mix refuses it too).
 * --------------------------------------------------------------------------------------------- */
int bya_masked_combine(void* x, const void* feat, const void* r, const void* af, int32_t mode, float alpha,
                       int32_t batch, int32_t n_id, int64_t N, int32_t D, int64_t x_row, int64_t x_batch_stride,
                       int64_t r_batch_stride, hipStream_t stream);

/* Routed mix BEFORE the output projection (to_out is linear, so sum_id w*(o_id W^T + b) = (sum_id w*o_id) W^T +
 * (sum_id w) b): z[b,n,:] = sum_id w[b,n,id] * feat[b,id,n,:], wsum[b,n] = sum_id w (fp32, may be NULL); w derived from
 * the routing logits exactly as in bya_masked_combine (mode 0 face, mode 1 audio).  The half-size GEMM that follows
 * takes wsum as bias_rowscale and the hidden stream as residual. */
int bya_routed_mix(const void* feat, const void* r, const void* af, void* z, float* wsum, int32_t mode, int32_t batch,
                   int32_t n_id, int64_t N, int32_t D, int64_t r_batch_stride, hipStream_t stream);

/* Patchify (im2col of the 2x2/stride-2 Conv2d of CogVideoXPatchEmbed, models/transformer.py:690):
 *   cols[b, (t*Ht+h)*Wt+w, c*4+ph*2+pw] = x[b,t,c,2h+ph,2w+pw]
 * and unpatchify (models/transformer.py:955-957):
 *   out[b,t,c,2h+ph,2w+pw] = y[b,(t*Ht+h)*Wt+w, c*4+ph*2+pw].  Index-only, bit-exact. */
int bya_patchify(const void* x, void* cols, int32_t batch, int32_t frames, int32_t channels, int32_t H, int32_t W,
                 hipStream_t stream);
int bya_unpatchify(const void* y, void* out, int32_t batch, int32_t frames, int32_t channels, int32_t H, int32_t W,
                   hipStream_t stream);

/* Elementwise helpers: y = act(x) (+ r) over n bf16 elements (n % 8 == 0). */
int bya_act_add(const void* x, const void* r, void* y, int64_t n, int32_t act, hipStream_t stream);
int bya_act_add_plan(const void* x, const void* r, const void* y, int64_t n, int32_t act,
                     bya_step_plan_info* plan);                  /* see bya_step_plan_info */

/* ---------------------------------------------------------------------------------------------
 * First-block step cache (an opt-in mode of this engine; the reference has none.  DESIGN.md section 19).
 * Consecutive denoise steps change the token stream little: a step whose first block moved the stream by nearly what it moved
 * it in the last fully computed step re-uses that step's residual of the WHOLE block stack instead of running blocks 1..L-1.
 *
 * x is the resident joint stream [B, S, D] bf16 (text rows first), n = B S D.  "Block 0" is iteration 0 of the step's block
 * loop, its face routing and audio injection included.  Buffers of n bf16 each: the snapshot E, the first-block residuals
 * r_ref (of the last FULLY COMPUTED step) and r_new (of this step), and the block-stack residual R.  Every step:
 *   1. after the patch embed                E <- x                                  (a device copy)
 *   2. block 0 runs
 *   3. PROBE, one pass (bya_step_cache_probe):
 *        r_new = bf16_rne(float(x) - float(E));   E <- x   (E now holds x after block 0)
 *        (bf16_rne: round to nearest even; every NaN becomes the quiet NaN 0x7fc0, so that the written bits are a function of
 *        the values alone -- converters disagree on a NaN's bits, torch's own scalar and vectorised ones among them)
 *        num = sum |float(r_new) - float(r_ref)|,  den = sum |float(r_ref)|   over all n elements; r_new enters as stored
 *        (rounded).  Terms in fp32, accumulation in fp64 in an order fixed by n alone: a lane adds its terms in pass order,
 *        a workgroup its lanes in a fixed tree, the workgroups' partials land in fixed slots (partials[2 g], [2 g + 1]) and a
 *        one-workgroup finish launch adds them in index order into sums[0] = num, sums[1] = den.  No floating-point atomics:
 *        the same inputs give the same 16 bytes on every run.  r_ref == NULL (no reference yet): r_new and E are written,
 *        both sums are 0.
 *   4. the host reads the two doubles (one synchronisation), d = num / den (den == 0: inf), and RE-USES the residual if and
 *      only if a reference exists, d < threshold and hits < max_consecutive_hits (none: unbounded).  NaN compares false: a
 *      full step.  threshold = 0 never re-uses.
 *   5. FULL step:    blocks 1..L-1 run; CAPTURE R = bf16_rne(float(x) - float(E)) (bya_step_cache_capture); r_ref and r_new
 *                    swap; hits = 0.
 *      RE-USED step: APPLY x = bf16_rne(float(x) + float(R)) in place (bya_step_cache_apply; x holds block 0's output);
 *                    hits += 1; r_ref and R stay.
 *   6. the head runs as always.
 * The whole batch decides jointly (both halves of a guided step's [uncond, cond] pair skip together).
 *
 * The three entry points are HBM-bound streaming passes: 16-byte loads and stores, eight bf16 per lane, a grid-stride walk of
 * grid = min(2048, ceil(n / 2048)) workgroups of 256 lanes -- a function of n alone.  Tensors are contiguous and 16-byte
 * aligned (partials, sums: 8 bytes), n % 8 == 0: else BYA_ERR_SHAPE (a missing pointer, n <= 0, n % 8) or BYA_ERR_ALIGN with
 * nothing launched.  They never allocate and never synchronise.  partials is the caller's: partials_bytes of the plan query
 * (2 doubles per workgroup).  bya_step_cache_probe_plan answers for all three (they share the grid); the plan is untouched on
 * rejection (plan == NULL: BYA_ERR_SHAPE).
 * --------------------------------------------------------------------------------------------- */
typedef struct bya_step_cache_plan_info {
    int32_t grid;             /* workgroups of the probe, the capture and the apply */
    int32_t vec;              /* bf16 per lane and pass: 8 (one 16-byte vector) */
    int32_t wg_pass_elems;    /* elements a workgroup takes per pass of its walk: 2048 */
    int32_t passes;           /* passes of workgroup 0: ceil(n / (grid wg_pass_elems)) */
    int64_t partials_bytes;   /* what the probe needs behind `partials`: 16 grid */
} bya_step_cache_plan_info;
int bya_step_cache_probe(const void* x, void* E, const void* r_ref, void* r_new, double* partials, double* sums, int64_t n,
                         hipStream_t stream);
int bya_step_cache_probe_plan(const void* x, const void* E, const void* r_ref, const void* r_new, int64_t n,
                              bya_step_cache_plan_info* plan);
int bya_step_cache_capture(const void* x, const void* E, void* R, int64_t n, hipStream_t stream);
int bya_step_cache_apply(void* x, const void* R, int64_t n, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row-stationary GEMM for K = 512 with optional fused LayerNorm, GELU(erf) and residual:
 *     C[M,N] = res + act( LN?(X)[M,512] . W[N,512]^T + bias )
 * Replaces, inside every SpatialTemporalAttentionBlock of the Embedding Router (models/router.py:468-493), the
 * pairs  nn.LayerNorm -> to_q|to_k|to_v  and  nn.LayerNorm -> mlp[0] -> GELU  (ln = 1) and the to_out / mlp[2]
 * projections with their residual adds (ln = 0, res = X of the block).
 * ln = 1: W must be the gamma-folded weight  Wg[n,k] = W[n,k] * gamma[k]  (bf16),  colsum[n] = sum_k Wg[n,k]  (fp32),
 *         cvec[n] = sum_k W[n,k] * beta[k] + bias[n]  (fp32);  the kernel computes the row mean / rstd itself and
 *         applies  rstd * (x . Wg^T - mean * colsum) + cvec.
 * ln = 0: W as is, cvec = bias (fp32), colsum ignored.
 * Statistics (ln = 1): ONE PASS.  sum x and sum x^2 come from the matrix core in fp32, var = max(E[x^2] - mean^2, 0), and the mean
 * is folded into the product (acc - mean * colsum): two cancellations.  Supported domain: bf16 rows with |mean| / spread <= 8 (and
 * colsum of a few units; with colsum = 25.6 only rows without an offset).  There the result is within half a bf16 ulp of what an
 * fp32 centred LayerNorm followed by the Linear gives (tests/test_norm_cond_gpu.py).  Beyond it the result drifts, measured on an
 * MI355X in bf16 ulps of the fp64 result: |mean| / spread = 8 with colsum = 25.6: up to 1.14;  64: 3.6 .. 11.5;  256: 32 .. 131;
 * near-constant rows (8 channels a few bf16 steps off a constant): 98 .. 526;  constant rows: finite, but up to 0.1 off cvec.
 * X: bf16 rows of 512 with row stride ldx; C / res: bf16 with row strides ldc / ldres (C may alias res).
 * N % (64 * nsplit) == 0; nsplit <= 0 lets the library choose how many column groups share a row block.
 * act: BYA_ACT_NONE or BYA_ACT_GELU_ERF.
 * --------------------------------------------------------------------------------------------- */
int bya_rowgemm512(const void* X, const void* W, const float* colsum, const float* cvec, const void* res, void* C,
                   int32_t M, int32_t N, int32_t ldx, int32_t ldc, int32_t ldres, int32_t ln, float eps, int32_t act,
                   int32_t nsplit, hipStream_t stream);
/* What a bya_rowgemm512 launch runs (host-side query like bya_gemm_bf16_plan: validates like the entry point, launches nothing,
 * needs no GPU; the launcher takes every decision from the same function).  form: the chunk-balanced kernel (every (256-row
 * block, 64-column chunk) pair, cut into `grid` equal contiguous ranges) or, for N = 512 without LayerNorm at
 * 2048 <= M <= 65536, the W-stationary one (64 row groups x 4 W quarters; its work items are the 16-row tiles). */
#define BYA_ROWGEMM_CHUNK_BALANCED 0
#define BYA_ROWGEMM_W_STATIONARY 1
typedef struct bya_rowgemm512_plan_info {
    int32_t form;               /* BYA_ROWGEMM_* */
    int32_t ln, res, act;       /* the template instance <LN, RES, ACT> */
    int32_t grid;               /* workgroups of 8 waves */
    int32_t crosses_row_block;  /* chunk-balanced: some workgroup's range holds chunks of two row blocks */
    int64_t work_items;         /* chunk-balanced: row blocks x chunks; W-stationary: 16-row tiles */
} bya_rowgemm512_plan_info;
int bya_rowgemm512_plan(const void* X, const void* W, const float* colsum, const float* cvec, const void* res, const void* C,
                        int32_t M, int32_t N, int32_t ldx, int32_t ldc, int32_t ldres, int32_t ln, int32_t act,
                        bya_rowgemm512_plan_info* plan);

/* ---------------------------------------------------------------------------------------------
 * Fused  LayerNorm(512) -> to_q | to_k | to_v (8 heads x 64) -> softmax(q k^T / 8) v  over SMALL groups of rows: the
 * temporal attention (the 13 frames of one (identity, location)) and the multi-ID attention (the identities of one
 * token) of SpatialTemporalAttentionBlock.  Replaces models/router.py:476-478 / :482-484 up to (not including) the
 * to_out projection: diffusers Attention + the default SDPA processor on [B', L, 512] with L = 13 / n_id, i.e. the
 * sequence  bya_rowgemm512(ln = 1, N = 1536)  ->  bya_attn_tiny  without the [M, 1536] q|k|v tensor in between.
 * X [M, 512] bf16 rows (stride ldx), O [M, 512] bf16 attention output in the SAME row order (stride ldo; may not alias X).
 * Wqkv [1536, 512] bf16: rows 0..511 = gamma-folded to_q, 512..1023 = to_k, 1024..1535 = to_v; colsum / cvec [1536] fp32
 * exactly as for bya_rowgemm512 with ln = 1.  Groups as for bya_attn_tiny: group (o, i), o < n_outer, i < n_inner,
 * consists of the L rows  o * outer_stride + i + e * seq_stride,  e < L;  1 <= L <= 32: groups of up to 16 rows share a
 * 16-row MFMA tile in power-of-two cells, groups of 17 .. 32 rows (25 latent frames of a 97-frame clip) take the two
 * tiles of one wave; longer sequences return BYA_ERR_UNSUPPORTED (the unfused pair handles them).
 * scale = 1 / sqrt(64).  q, k, v are rounded to bf16 where the unfused path stored them, P to bf16 before P.V.
 * Statistics: one pass, as bya_rowgemm512 with ln = 1 -- the same domain (|mean| / spread <= 8) and, measured through a one-key
 * group (L = 1: O = v), the same drift beyond it: 0.78 bf16 ulp at 8 with colsum = 25.6, 5.9 at 64, 58 at 256, 429 on
 * near-constant rows.
 * Score domain: the softmax subtracts each query's largest score over the keys of its group before exp2, so there is NO
 * static bound on q . k * scale (unlike the static-bound attention kernels above).  The suite holds every output element to
 * the fp64 softmax of the bf16 q, k, v on scores of up to +-162 exp2 units (q . k * scale * log2 e) within one group, a
 * constant of +-60 under a row, one key 40 above the rest, and all-equal scores (tests/cond_rowattn.py: |error| <=
 * (1 + eps) 2^-8 (sum_j p_j |v_j| / l + |O|), eps = 0.19 there).  The keys of the tile's other groups, its empty slots (which
 * read as rows of zeros: k = cvec_k, v = cvec_v) and rows of no group have no weight in the result, whatever they hold.
 * bya_router_group_attn_out inherits all of it.
 * --------------------------------------------------------------------------------------------- */
int bya_router_group_attn(const void* X, const void* Wqkv, const float* colsum, const float* cvec, void* O,
                          int32_t M, int32_t ldx, int32_t ldo, int32_t L, int64_t n_outer, int64_t n_inner,
                          int64_t outer_stride, int64_t seq_stride, float eps, float scale, hipStream_t stream);
/* What a bya_router_group_attn launch runs (host-side query): P slots per group (the power of two >= L; 16 when wide), G = 16 / P
 * groups per 16-row tile, wide (16 < L <= 32: a group takes the two tiles of one wave), the tiles and the workgroups. */
typedef struct bya_router_group_attn_plan_info {
    int32_t P, G, wide;
    int32_t blocks;             /* workgroups of 8 waves x 2 tiles */
    int64_t tiles;
} bya_router_group_attn_plan_info;
int bya_router_group_attn_plan(const void* X, const void* Wqkv, const float* colsum, const float* cvec, const void* O,
                               int32_t M, int32_t ldx, int32_t ldo, int32_t L, int64_t n_outer, int64_t n_inner,
                               int64_t outer_stride, int64_t seq_stride, bya_router_group_attn_plan_info* plan);

/* ---------------------------------------------------------------------------------------------
 * Router chains (round 6; csrc/rowchain.hip): two Linears of a SpatialTemporalAttentionBlock sub-block in ONE launch, the
 * [M, 512] activation between them in registers, updating the router rows in place.
 *
 * bya_router_mlp_fused:  C = X + mlp[2]( GELU_erf( mlp[0]( LayerNorm(X) ) ) )  -- models/router.py:491 with norm4 -- i.e.
 *   bya_rowgemm512(ln = 1, act = GELU_ERF) -> bya_rowgemm512(res = X)  without the hidden tensor.  W1 [512, 512] gamma-
 *   folded with colsum1 / cvec1 as for bya_rowgemm512 ln = 1; W2 [512, 512] with cvec2 = its bias.  C may be X (every row
 *   is read and written by one wave); the router's hidden width must equal 512 (mlp_ratio 1, models/router.py:318).
 * bya_router_group_attn_out:  C = X + to_out( attention over row groups( LayerNorm(X) ) )  -- models/router.py:482-483 /
 *   :486-487 -- i.e.  bya_router_group_attn -> bya_rowgemm512(res = X)  without the attention-output tensor.  Wqkv, colsum,
 *   cvec, the group geometry (L, n_outer, n_inner, outer_stride, seq_stride) and scale exactly as for
 *   bya_router_group_attn; Wo [512, 512] with cvec_o = its bias.  1 <= L <= 16 (a group is held by ONE 16-row MFMA tile;
 *   longer groups: BYA_ERR_UNSUPPORTED, the caller keeps the two launches).  C may be X.  Rows outside every group are
 *   neither read nor written.
 * Both give, BIT FOR BIT, what their two launches give (same MFMA order over K, same epilogue expressions on the same
 * rounded values).  tiles_pass0: 16-row tiles per workgroup in the first pass over the rows (1..8; 0 = 8); the remainder
 * is dealt over all workgroups in a short second pass.  A tuning hint: results do not depend on it.
 * Statistics of both chains: one pass (rowgemm_common.h tile_row_stats), the domain and the drift of bya_rowgemm512 with ln = 1:
 * measured on the value kept in registers, bya_router_mlp_fused is 1.0 bf16 ulp off at |mean| / spread = 8 (as its two-launch
 * definition in fp32), 4.0 at 64, 34 .. 49 at 256; bya_router_group_attn_out 1.0, 11.5 and 40.
 * --------------------------------------------------------------------------------------------- */
int bya_router_mlp_fused(const void* X, const void* W1, const float* colsum1, const float* cvec1, const void* W2,
                         const float* cvec2, void* C, int32_t M, int32_t ldx, int32_t ldc, float eps, int32_t tiles_pass0,
                         hipStream_t stream);
int bya_router_group_attn_out(const void* X, const void* Wqkv, const float* colsum, const float* cvec, const void* Wo,
                              const float* cvec_o, void* C, int32_t M, int32_t ldx, int32_t ldc, int32_t L, int64_t n_outer,
                              int64_t n_inner, int64_t outer_stride, int64_t seq_stride, float eps, float scale,
                              int32_t tiles_pass0, hipStream_t stream);
/* What a chain launch runs (host-side queries): the 16-row tiles, the first pass's tiles per workgroup (tiles_pass0, or the
 * library's choice for 0), the grid, the number of passes over the rows, and the last pass: tiles per workgroup there and how
 * many workgroups have one (the others only keep staging W). */
typedef struct bya_router_chain_plan_info {
    int32_t tiles, tp0, grid, passes, tiles_last, wgs_last;
} bya_router_chain_plan_info;
int bya_router_mlp_fused_plan(const void* X, const void* W1, const float* colsum1, const float* cvec1, const void* W2,
                              const float* cvec2, const void* C, int32_t M, int32_t ldx, int32_t ldc, int32_t tiles_pass0,
                              bya_router_chain_plan_info* plan);
int bya_router_group_attn_out_plan(const void* X, const void* Wqkv, const float* colsum, const float* cvec, const void* Wo,
                                   const float* cvec_o, const void* C, int32_t M, int32_t ldx, int32_t ldc, int32_t L,
                                   int64_t n_outer, int64_t n_inner, int64_t outer_stride, int64_t seq_stride,
                                   int32_t tiles_pass0, bya_router_chain_plan_info* plan);

/* ---------------------------------------------------------------------------------------------
 * Classifier-free-guidance combine + scheduler step in one pass over the latents.
 * Replaces models/pipeline_bindyouravatar.py:924-948: noise = u + g*(c - u) in fp32 on the bf16 prediction
 * (n_pred = 2: [uncond, cond], second sample at pred + pred_stride; n_pred = 1: no guidance), then the
 * v-prediction step of diffusers' CogVideoXDDIMScheduler / CogVideoXDPMScheduler:
 *   x0   = bf16(sqrt_alpha * x) - sqrt_beta * noise_pred
 *   d    = old_x0 ? k_cur * x0 - k_old * old_x0 : x0                (DPM second-order correction)
 *   prev = bf16( (bf16(k_sample * x) - k_denoised * d) [+ bf16(k_noise * noise)] )
 * DDIM: k_sample = a_t, k_denoised = -b_t, old_x0 = noise = NULL.  x0_out (fp32, optional) feeds the next DPM step.
 * The bf16() roundings are where torch's type promotion rounds (0-dim coefficient x bf16 tensor).
 * --------------------------------------------------------------------------------------------- */
typedef struct bya_sched_coef {
    float guidance, sqrt_alpha, sqrt_beta, k_sample, k_denoised, k_noise, k_cur, k_old;
} bya_sched_coef;

int bya_cfg_scheduler_step(const void* pred, int32_t n_pred, int64_t pred_stride, const void* sample,
                           const float* old_x0, const void* noise, void* prev_sample, float* x0_out,
                           int64_t n, const bya_sched_coef* coef, hipStream_t stream);
int bya_cfg_scheduler_step_plan(const void* pred, int32_t n_pred, int64_t pred_stride, const void* sample,
                                const void* prev_sample, int64_t n, const bya_sched_coef* coef,
                                bya_step_plan_info* plan);       /* see bya_step_plan_info */

/* Tracking masks -> routing_logits_forcing (stage 2 of the reference inference; util/utils.py:481-514 resize_mask,
 * :871-936 process_masks_to_routing_logits parts 2-3).  masks: uint8 [n_id, in_frames, in_h, in_w], > 0 = foreground;
 * logits: bf16 [frames*h*w, n_id], one-hot per token (zero row = background), the LAST identity whose trilinearly
 * resized (align_corners = false) mask exceeds 0.5 wins.  Index / threshold work: bit-exact against the reference. */
int bya_masks_to_routing_logits(const void* masks, void* logits, int32_t n_id, int32_t in_frames, int32_t in_h,
                                int32_t in_w, int32_t frames, int32_t h, int32_t w, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Video VAE either side of the denoise loop: AutoencoderKLCogVideoX (diffusers; un-vendored
 * third-party layer) as called by models/pipeline_bindyouravatar.py:406-424 (encode of the conditioning frame) and :461-466
 * (decode of the finished latents).  Activations are channels-last bf16 [T, H, W, C]; every convolution is
 * bya_vae_patches + bya_gemm_bf16 (bias / residual in its epilogue), 1x1x1 convolutions are bya_gemm_bf16 alone.
 * --------------------------------------------------------------------------------------------- */
/* Patch matrix of a causal KT x 3 x 3 convolution (KT = 3: CogVideoXCausalConv3d; KT = 1: the per-frame 3 x 3 convolutions of
 * CogVideoXUpsample3D / CogVideoXDownsample3D) for output frames [t0, t0 + nt) of a chunk: out [nt * Ho * Wo, Kpad] bf16, column
 * (kt, kh, kw, c), zero beyond KT * 9 * C.  x: the chunk [Ts, Hs, Ws, C]; cache: the previous chunk's last KT - 1 frames
 * [KT - 1, Hs, Ws, C] or NULL (first chunk: frame 0 is repeated -- diffusers pad_mode "first").  Space: tap (kh, kw) of output
 * (h, w) reads (h * stride + kh - pad, w * stride + kw - pad), zero outside.  up = 1: the convolution runs on the
 * nearest-neighbour x2 up-sampling of x in space (never materialised) and in time by tmode: 0 = frames as stored, 1 = every
 * frame doubled, 2 = first frame single, the rest doubled (CogVideoXUpsample3D.compress_time with an odd frame count). */
int bya_vae_patches(const void* x, const void* cache, void* out, int32_t Ts, int32_t Hs, int32_t Ws, int32_t C, int32_t KT,
                    int32_t stride, int32_t pad, int32_t up, int32_t tmode, int32_t Ho, int32_t Wo, int32_t t0, int32_t nt,
                    int32_t Kpad, hipStream_t stream);
/* GroupNorm statistics of one chunk: sums [groups][2] fp32 = (sum, sum of squares) over x [rows, C], summed in a FIXED order
 * (no atomics: the same chunk gives the same bits every run).  partial: caller's scratch, ceil(rows / 512) * groups * 2 floats.
 * C <= 512 with C / 8 a power of two.  Every sum is carried in fp64 and rounded to fp32 once per partial and once per result:
 * the pair is as good as its fp32 slots can hold, whatever the depth of the hierarchy.  Nothing in the package calls this form or
 * bya_vae_norm_act any more (vae.py runs the two _moments entry points below); they stay for callers that hold such sums. */
int bya_vae_groupnorm_stats(const void* x, float* sums, float* partial, int64_t rows, int32_t C, int32_t groups,
                            hipStream_t stream);
/* The same statistics as CENTRED moments: moments [groups][2] fp32 = (mean, var) with var = max(sum x^2 / n - mean^2, 0) formed in
 * fp64 from fp64 sums (one read of x, like bya_vae_groupnorm_stats) and rounded to fp32 once: the cancellation costs 2^-53 R^2
 * of the variance of a group with R = |mean| / spread, where the fp32 pair above holds it to 3 * 2^-24 * R^2 at best.  partial:
 * caller's scratch, ceil(rows / 512) * groups * 2 DOUBLES.  Same shapes, same fixed order.  Read by bya_vae_norm_act_moments. */
int bya_vae_groupnorm_moments(const void* x, float* moments, double* partial, int64_t rows, int32_t C, int32_t groups,
                              hipStream_t stream);
/* y = act( GroupNorm(x; sums, gamma, beta, eps) [ * zy[z(row)] + zb[z(row)] ] ), act 0 = none, 1 = SiLU.  zy / zb (both or
 * neither): conv_y / conv_b of CogVideoXSpatialNorm3D evaluated at LATENT resolution [Tz * hz * wz rows, row stride ldz]; row
 * (t, h, w) of x [T, H, W, C] reads latent position (frame by tmode, h >> log2(H / hz), w >> log2(W / wz)): tmode 0 = same
 * frame, 1 = floor(t Tz / T), 2 = first frame apart (0 -> 0, t -> 1 + floor((t - 1)(Tz - 1) / (T - 1))): torch's nearest
 * F.interpolate, first frame and the rest resized separately when T is odd and > 1.
 * Statistics of bya_vae_norm_act: ONE PASS, mean = sum / n and var = max(sum of squares / n - mean^2, 0) in fp32 from the fp32 pair
 * ``sums``, which holds the variance of a group with R = |mean| / spread to about 3 * 2^-24 * R^2.  Supported domain: R <= 8.
 * Beyond it the result drifts, measured on an MI355X in bf16 ulps of the fp64 result: R = 64: 0.8 .. 3.9 (the worst where gamma,
 * beta and the modulation cancel);  256: 0.7 .. 18.6;  near-constant groups: 4 .. 179;  constant groups: beta exactly.
 * bya_vae_norm_act_moments is the same operation on ``moments`` = (mean, var) of bya_vae_groupnorm_moments -- what the VAE runs --
 * and has no such restriction: within half a bf16 ulp of F.group_norm in fp32 on every distribution of tests/cond_norm.py, R = 256,
 * near-constant and constant groups included (tests/test_norm_cond_gpu.py). */
/* out_pad = 1: y is the zero-padded input of bya_vae_conv3d, [T + 2, H + 2, W + 2, C] (the caller zero-fills it once and
 * writes the two context frames; this call writes pixel (t, h, w) at (t + 2, h + 1, w + 1)); rows must be T H W. */
int bya_vae_norm_act(const void* x, void* y, const float* sums, const void* gamma, const void* beta, const void* zy,
                     const void* zb, int64_t rows, int32_t C, int32_t groups, int32_t act, float eps, int32_t T, int32_t H,
                     int32_t W, int32_t Tz, int32_t hz, int32_t wz, int32_t tmode, int64_t ldz, int32_t out_pad,
                     hipStream_t stream);
int bya_vae_norm_act_moments(const void* x, void* y, const float* moments, const void* gamma, const void* beta, const void* zy,
                             const void* zb, int64_t rows, int32_t C, int32_t groups, int32_t act, float eps, int32_t T, int32_t H,
                             int32_t W, int32_t Tz, int32_t hz, int32_t wz, int32_t tmode, int64_t ldz, int32_t out_pad,
                             hipStream_t stream);

/* Causal KT x 3 x 3 convolution, stride 1 (KT = 3: diffusers CogVideoXCausalConv3d inside CogVideoXResnetBlock3D and conv_out;
 * KT = 1: the per-frame 3 x 3 convolution of CogVideoXUpsample3D; reached from models/pipeline_bindyouravatar.py:461-466 /
 * :406-424), as an IMPLICIT GEMM on the persistent MFMA kernel: no patch matrix.
 * xpad: bf16 [To + KT - 1, H + 2, W + 2, C], channels-last, zero border of one pixel around every frame; for KT = 3 frames 0
 * and 1 are the causal context (last two input frames of the previous chunk, or the first frame twice); w: [Cout, ldw] bf16
 * with column ((dt 3 + dh) 3 + dw) C + c; bias [Cout] or NULL; res [To, H, W, ldres] or NULL; out [To, H, W, ldc] (may alias
 * res).  C in {128, 256, 512}; Cout, ldc, ldres multiples of 8.  out = res + bias + conv(x). */
int bya_vae_conv3d(const void* xpad, const void* w, const void* bias, const void* res, void* out, int32_t To, int32_t H,
                   int32_t W, int32_t C, int32_t Cout, int32_t KT, int64_t ldw, int64_t ldc, int64_t ldres,
                   hipStream_t stream);

/* Nearest-neighbour up-sampling of x [T, H, W, C] (space x 2; time by tmode as in bya_vae_patches: 0 = frames as they are,
 * 1 = every frame doubled, 2 = first frame single and the rest doubled) into the interior of ypad [To, 2 H + 2, 2 W + 2, C],
 * the zero-padded input of the up-sampler's convolution (bya_vae_conv3d, KT = 1); the caller zero-fills ypad once. */
int bya_vae_upsample_pad(const void* x, void* ypad, int32_t T, int32_t H, int32_t W, int32_t C, int32_t tmode,
                         hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU exchanges of the sharded step over RCCL.  ``comm`` is the caller's ncclComm_t (one
 * process per GPU); both calls only ENQUEUE on ``stream`` -- give them a stream of their own to overlap with compute.
 * The reference has no inference parallelism; these have no counterpart there.  (The Python module of this package
 * issues the same exchanges through torch.distributed's nccl backend = RCCL, because torch does not expose its
 * communicator.)  BYA_ERR_UNSUPPORTED: no RCCL in the process.
 * --------------------------------------------------------------------------------------------- */
/* Exchange A, K/V form: k_local / v_local [rows_local, row_elems] bf16 of this rank -> k_full / v_full
 * [world * rows_local, row_elems] on every rank (rank-major = global row order), one grouped call. */
int bya_allgather_kv(const void* k_local, const void* v_local, void* k_full, void* v_full, int64_t rows_local,
                     int64_t row_elems, void* comm, hipStream_t stream);
/* Exchange A head-parallel form and exchange B (router repartition frame-major <-> location-major): uneven all-to-all
 * of bf16 elements.  send_counts[p] elements go to rank p from send + sum(send_counts[:p]); recv_counts[p] elements
 * arrive from rank p at recv + sum(recv_counts[:p]).  Grouped point-to-point: every element crosses one xGMI link once. */
int bya_alltoall_router(const void* send, void* recv, const int64_t* send_counts, const int64_t* recv_counts,
                        int32_t world, void* comm, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * P2P exchange engine (csrc/comm.hip): the exchanges of the sharded step as ordinary kernels that store
 * straight into the peers' HBM over xGMI -- one launch per exchange whatever its scatter/gather list, capturable in a
 * hipGraph (RCCL collectives are neither).  No reference counterpart (the reference has no inference parallelism).
 * Set-up is the host's (bind_your_avatar_implementation_amd/p2p.py): every rank allocates its receive buffers and one
 * control block of 64 uint32 words per channel (zero-filled), trades hipIpc handles once, and builds per channel, in DEVICE
 * memory, (a) the copy table (bya_p2p_copy below): `src` local, `dst` an address inside a peer's (or its own) receive buffer
 * mapped into this process; 16-byte aligned pieces and pitches take the fast path; (b) `peer_ctrl[p]` = the
 * channel's control block ON PEER p (mapped), p < world, own rank included.
 * bya_p2p_push: copy every table entry, then publish the channel's next sequence number to word `rank` of every peer's
 * control block.  bya_p2p_wait (receiver, same channel, once per push of the peers): returns to the stream when all
 * `world` source ranks have published the receiver's next expected number; kernels enqueued behind it see the data (the
 * wait runs as 16 small workgroups, dealt over the XCDs, each ending in a system-scope acquire).  bya_p2p_exchange = push
 * and wait in ONE launch, for the exchanges nothing is overlapped with.
 * Sequence numbers live in the control block (words 32 / 33): a hipGraph replay advances them by itself.  A wait is bounded
 * by wall time: `wait_limit_ms` of the launch (<= 0: 30 s; a captured launch keeps the limit it was captured with).  One
 * that gives up counts itself in word 35 of its channel and in word 37 of `group_ctrl` -- the FIRST control block of the
 * group the channel belongs to (may be NULL: then only the channel's own word is used) -- both sticky.  A wait that finds
 * the group's word set returns at once, counted as timed out: after the first time-out of a group the rest of the step runs
 * through without polling.  bya_p2p_poison(ctrl_base, n_channels, out, n) -- enqueue it behind the last consumer of a step --
 * overwrites the bf16 tensor `out` with NaN when any of the n_channels control blocks (64 words apart) carries a time-out or a
 * non-zero word 38 (written by the host: "this step's exchange checksum differed between the ranks") or word 39 (written by
 * bya_p2p_verify, below: "a piece of an exchange did not arrive as it was sent"), so that a result made
 * from a buffer that never arrived, or arrived stale, cannot be consumed.  The caller guarantees that a receive buffer is not
 * pushed into again before its owner has consumed it (the step's data dependencies do).
 * --------------------------------------------------------------------------------------------- */
typedef struct bya_p2p_copy {      /* a 2-D piece: `rows` rows of `row_bytes` bytes (a contiguous piece is ONE row) */
    const void* src;
    void* dst;
    int64_t row_bytes;             /* % 2 == 0 */
    int64_t rows;
    int64_t src_pitch, dst_pitch;  /* bytes from one row to the next on either side (% 2 == 0; ignored when rows == 1) */
    int64_t chunk0;                /* chunks of the entries before this one; an entry has rows * ceil(row_bytes / 64 KiB) chunks
                                      when row_bytes > 64 KiB, else ceil(rows / floor(64 KiB / row_bytes)) */
} bya_p2p_copy;

/* Exchange verification (opt-in: BYA_SP_VERIFY=all in the host module; csrc/comm.hip).  The CHECKSUM of a piece: its bytes in
 * logical order (row-major over rows x row_bytes, pitches removed) as 16-bit little-endian words w_i, i = 0, 1, ...:
 *     A = sum w_i                        mod 2^64
 *     B = sum w_i * ((i mod 65521) + 1)  mod 2^64
 * Integer sums: exact, and independent of the order in which workgroups and chunks add to them (the chunk walk, the grid size
 * and a graph replay cannot change them).  B catches rows that landed at another pitch or offset; A alone would not.
 * bya_p2p_push_verified / bya_p2p_exchange_verified = bya_p2p_push / bya_p2p_exchange whose copy loop also sums what it has
 * in registers, per entry of the copy table, into `acc_dev` [n_copies][2] uint64 (zero-filled by the host; zeroed again by
 * the launch), and whose last workgroup writes, BEFORE it publishes the sequence number, one RECORD per destination rank p
 * to `peer_rec_dev[p]` + rank * BYA_P2P_VERIFY_REC_WORDS int64 words -- peer_rec_dev[p] = the channel's [32 senders][REC_WORDS]
 * block of rank p's record buffer (mapped; fine-grained memory where the platform hands it out).  A record has two halves of
 * 64 words, taken by the parity of the sequence number (a sender can be ONE exchange ahead of a receiver that has not
 * verified yet, never two): [0] sequence number, [1] n_pieces (<= BYA_P2P_VERIFY_PIECES), then per piece 7 words
 * {buf_id, dst_byte_offset, row_bytes, rows, dst_pitch, A, B}.  `pieces_dev` [n_copies][4] int64 = {destination rank (< 0:
 * the place-holder entry), index of the piece in that rank's record, buf_id, dst_byte_offset}; `counts_dev` [world] int64 =
 * pieces per destination rank.  buf_id = index of the destination buffer in an order every rank agrees on (the host module:
 * order of allocation); dst_byte_offset is relative to that buffer's base ON THE RECEIVER.
 * bya_p2p_verify (receiver, behind the wait of the same exchange; no host synchronisation, capturable): for every sender's
 * record of the sequence number the channel has just waited for, recompute A, B of every piece from the receiver's own
 * buffer -- `buf_bases_dev` [BYA_P2P_VERIFY_BUFS][2] int64 = {local base address, bytes; 0, 0 = no such buffer} -- with
 * ordinary cached loads (what a consumer kernel reads) and compare.  On a difference: re-read the piece ONCE with
 * system-scope loads and note whether that sum matches; append an entry to `log_dev` (int64: [0] entries wanted so far, [16 +
 * 16 * e ...] entry e < BYA_P2P_VERIFY_LOG_ENTRIES = {channel, sender, sequence, piece, want A, want B, got A, got B,
 * reread_matches, buf_id, receiver rank, kind: 0 sums differ / 1 no record of that sequence number / 2 record names memory
 * outside the buffer table (nothing is read)}; behind the entries BYA_P2P_VERIFY_PIECES * 32 * 4 words of scratch; all
 * BYA_P2P_VERIFY_LOG_WORDS zero-filled by the host); bump word 39 of `ctrl` and word 40 of `group_ctrl` (sticky; bya_p2p_poison
 * treats word 39 like a time-out).  A channel or group that carries a time-out is not verified (its data is known bad).
 * `ctrl` must be one of the control blocks that start at `group_ctrl` (its index there is the log's channel). */
#define BYA_P2P_VERIFY_PIECES 8
#define BYA_P2P_VERIFY_REC_WORDS 128
#define BYA_P2P_VERIFY_BUFS 1024
#define BYA_P2P_VERIFY_LOG_ENTRIES 64
#define BYA_P2P_VERIFY_LOG_WORDS (16 + 16 * BYA_P2P_VERIFY_LOG_ENTRIES + BYA_P2P_VERIFY_PIECES * 32 * 4)
int bya_p2p_push_verified(const bya_p2p_copy* copies_dev, int32_t n_copies, int64_t total_chunks, void* const* peer_ctrl_dev,
                          int32_t world, int32_t rank, void* ctrl, const int64_t* pieces_dev, const int64_t* counts_dev,
                          void* acc_dev, void* const* peer_rec_dev, hipStream_t stream);
int bya_p2p_exchange_verified(const bya_p2p_copy* copies_dev, int32_t n_copies, int64_t total_chunks, void* const* peer_ctrl_dev,
                              int32_t world, int32_t rank, void* ctrl, void* group_ctrl, int64_t wait_limit_ms,
                              const int64_t* pieces_dev, const int64_t* counts_dev, void* acc_dev, void* const* peer_rec_dev,
                              hipStream_t stream);
int bya_p2p_verify(void* ctrl, const void* rec, const int64_t* buf_bases_dev, int32_t world, int32_t rank, void* group_ctrl,
                   void* log_dev, hipStream_t stream);

int bya_p2p_push(const bya_p2p_copy* copies_dev, int32_t n_copies, int64_t total_chunks, void* const* peer_ctrl_dev,
                 int32_t world, int32_t rank, void* ctrl, hipStream_t stream);
int bya_p2p_wait(void* ctrl, int32_t world, void* group_ctrl, int64_t wait_limit_ms, hipStream_t stream);
int bya_p2p_exchange(const bya_p2p_copy* copies_dev, int32_t n_copies, int64_t total_chunks, void* const* peer_ctrl_dev,
                     int32_t world, int32_t rank, void* ctrl, void* group_ctrl, int64_t wait_limit_ms, hipStream_t stream);
int bya_p2p_poison(const void* ctrl_base, int32_t n_channels, void* out, int64_t n_elems, hipStream_t stream);
/* Set-up only (the ONLY entry points of this library that allocate; never called inside a step): device memory a peer may
 * store into or a running kernel polls, by kind -- 0 coarse-grained (hipMalloc), 1 fine-grained, 2 uncached
 * (hipExtMallocWithFlags) -- zero-filled, and its hipIpc handle (64 bytes) for the peers.  BYA_ERR_UNSUPPORTED: the
 * platform refused (the host module then falls back, p2p.py). */
int bya_p2p_alloc(int64_t bytes, int32_t kind, void** out);
int bya_p2p_free(void* ptr);
int bya_p2p_ipc_export(void* ptr, void* handle64);
int bya_p2p_ipc_import(const void* handle64, void** out);
int bya_p2p_ipc_release(void* ptr);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BYA_H */
