// gemm_fp8_v4_qkn.hip's kernel with the score-bound statistics in its epilogue (the *_stats entry points): gemm_fp8_v4.hip
// compiled under BYA_F8_QKN = 2 -- gemm256p_fp8_qkn_stats_kernel and bya_launch_gemm256p_fp8_qkn_stats.  A translation unit
// of its own for the same reason (build.AGPR_SOURCES).
#define BYA_F8_QKN 2
#include "gemm_fp8_v4.hip"
