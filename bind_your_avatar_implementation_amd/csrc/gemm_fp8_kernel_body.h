// The body of the tiled e4m3 GEMM kernel (gemm_fp8_kernel.h includes this file once per kernel, between the braces of a
// __global__ template <BM, BN, WAVES_M, WAVES_N> with parameters (GemmArgs p, sa, sw, GM)): the K-loop, the row x channel
// scales and the epilogue -- GEMM_FP8_BODY_QKN 0: the common one (epilogue_block), 1: the q/k-norm + RoPE one
// (bya_gemm_fp8_qkv_norm_rope; p.qkn_*).  Text, not a function: the plain kernel keeps the instruction stream it had as one
// function (as a __forceinline__ body taking the arguments by reference hipcc laid its blocks out differently).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NWAVES = WAVES_M * WAVES_N;
    constexpr int TILE_A = BM * BK8, TILE_W = BN * BK8, STAGE = TILE_A + TILE_W;
    constexpr int WM = BM / WAVES_M, WN = BN / WAVES_N, MI = WM / 16, NI = WN / 16;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    const int id = xcd_remap(blockIdx.x, nwg);
    // group-M order: GM row-tiles sweep one column-tile before moving on (W panels are re-read once per group of rows)
    const int per_group = GM * tiles_n;
    const int group = id / per_group, first_m = group * GM;
    const int gsz = (tiles_m - first_m) < GM ? (tiles_m - first_m) : GM;
    const int in_g = id - group * per_group;
    const int tm = first_m + in_g % gsz, tn = in_g / gsz;
    const int m0 = tm * BM, n0 = tn * BN;
    const int z = blockIdx.z;

    const uint8_t* A = reinterpret_cast<const uint8_t*>(p.A) + (long long)z * p.a_bs;
    const uint8_t* W = reinterpret_cast<const uint8_t*>(p.W);
    const int nk = p.K / BK8;

    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * STAGE;
        stage_tile8<BM, NWAVES>(A, p.lda, m0, p.M - 1, kt * BK8, base, wave, lane);
        stage_tile8<BN, NWAVES>(W, p.ldw, n0, p.N - 1, kt * BK8, base + TILE_A, wave, lane);
    };

    f32x4 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int fr = lane & 15, fq = lane >> 4;
    const int unit = 0x7f7f7f7f;                            // E8M0 block scales: 2^(127 - 127) in every byte

    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
        const char* ta = smem + (kt & 1) * STAGE;
        const char* tw = ta + TILE_A;
        i32x8 fa[MI], fw[NI];
#pragma unroll
        for (int j = 0; j < MI; ++j) fa[j] = lds_frag8(ta, wm * WM + j * 16 + fr, fq);
#pragma unroll
        for (int i = 0; i < NI; ++i) fw[i] = lds_frag8(tw, wn * WN + i * 16 + fr, fq);
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < MI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fa[j], acc[i][j], 0, 0, 0, unit, 0, unit);
    }

    // ---- row and channel scales, then the common epilogue.  Lane holds C[m][n4 .. n4+3], m = m_base + 16 j,
    // n4 = n_base + 16 i  (W fragment = A operand: the 16 x 16 result is transposed, as in every GEMM kernel here)
    const int m_base = m0 + wm * WM + fr, n_base = n0 + wn * WN + fq * 4;
    float ra[MI];
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const int m = m_base + 16 * j;
        ra[j] = sa[(long long)z * p.M + (m < p.M ? m : p.M - 1)];
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int n4 = n_base + 16 * i;
        const f32x4 rw = n4 < p.N ? *reinterpret_cast<const f32x4*>(sw + n4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < MI; ++j)
#pragma unroll
#if !GEMM_FP8_BODY_QKN
            for (int e = 0; e < 4; ++e) acc[i][j][e] *= ra[j] * rw[e];
    }
    auto run = [&](auto act_tag) {
        epilogue_block<decltype(act_tag)::value, NI, MI, (NI * MI > 16 ? 1 : NI)>(p, z, m_base, n_base, acc);
    };
    dispatch_act_big(p.act, run);
#else
            for (int e = 0; e < 4; ++e) {
                acc[i][j][e] *= ra[j] * rw[e];
                // The scaled value is rounded to fp32 HERE, as in the two-launch path, whose epilogue adds the bias with an fmaf
                // of its own.  epilogue_mx_qkn adds it with a plain +, which hipcc's default -ffp-contract would merge with this
                // multiply into fma(acc, scale, bias) -- one rounding less, other bits.  An empty asm that owns the register
                // hides the multiply from the addition.
                asm("" : "+v"(acc[i][j][e]));
            }
    }
    // bit for bit the epilogue of the other branch (alpha = 1, no activation, no row scale of the bias) followed by
    // bya_qknorm_rope: epilogue_mx_qkn on the scaled accumulators, q / k / v per 64-column head
    epilogue_mx_qkn<NI, MI, BYA_MX_QKN_STORE16 != 0>(p, z, m_base, n0 + wn * WN, fq, acc);
#endif
