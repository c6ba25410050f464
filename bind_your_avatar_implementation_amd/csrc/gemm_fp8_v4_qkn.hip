// The persistent 256 x 256 e4m3 GEMM with the q/k-norm + RoPE epilogue (bya_gemm_fp8_qkv_norm_rope): gemm_fp8_v4.hip compiled
// under BYA_F8_QKN -- gemm256p_fp8_qkn_kernel and bya_launch_gemm256p_fp8_qkn.  A translation unit of its own: each holds ONE
// instance of the hand-placed kernel (its 512 registers and its packed-fp32 count are accounted per unit), built with the same
// flags (build.AGPR_SOURCES).
#define BYA_F8_QKN 1
#include "gemm_fp8_v4.hip"
