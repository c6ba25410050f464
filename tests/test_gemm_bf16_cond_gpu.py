"""Every bf16 GEMM path -- bya_gemm_bf16 on its eight plan paths, split-K and the row split, bya_gemm_skinny_bf16, and
bya_rowgemm512 without LayerNorm on both of its kernels -- on full-range bf16 bit patterns and off-grid epilogue operands, every
element against fp64: tests/cond_gemm_bf16.py has the data, the case tables and the glue, tests/cond_gemm.py the measure and the
derivation of the bars; tests/test_gemm_bf16_cond_cpu.py holds the restatement inside them, plants the faults they must catch
and plans the same tables on meta tensors.  The plan is asserted before every launch, under the case's options, and every case
prints, per family, the worst e with its eps, the differing share, the signed mean and (K >= 1024) the rms beside the
restatement's."""
import pytest

import cond_gemm_bf16 as B

pytestmark = pytest.mark.gpu


def _ops(dev):
    from bind_your_avatar_implementation_amd import ops
    ops.ensure_gemm_workspace(dev)            # (split-K plans depend on it: registered before the first query)
    return ops


def ids(cases):
    return [c["id"] for c in cases]


@pytest.mark.parametrize("c", B.plain_cases(), ids=ids(B.plain_cases()))
def test_bf16_gemm_every_element_against_fp64(dev, c):
    """near / spread / cancel / subnormal / extreme rows in one plain launch: subnormal and extreme bit for bit."""
    B.run_gemm(_ops(dev), dev, c)


@pytest.mark.parametrize("c", B.one_hot_cases(), ids=ids(B.one_hot_cases()))
def test_bf16_gemm_one_hot_returns_every_finite_bf16_value(dev, c):
    """The output is A[m, n mod K] bit for bit, all 65280 finite patterns, subnormals and the largest values included; the
    second launch -0.5 times it, rounded once."""
    B.run_gemm(_ops(dev), dev, c)


@pytest.mark.parametrize("c", B.epilogue_cases(), ids=ids(B.epilogue_cases()))
def test_bf16_gemm_epilogues_against_fp64(dev, c):
    """The seven epilogues of cond_gemm.EPILOGUES off every grid (n_split 3 through the guarded split outputs, batch 2 with the
    residual aliasing the output) and res-cancel, whose result is a few bf16 steps of the value before the residual."""
    B.run_gemm(_ops(dev), dev, c)


@pytest.mark.parametrize("c", B.activation_cases(), ids=ids(B.activation_cases()))
def test_bf16_gemm_activations_over_their_whole_range(dev, c):
    """Pre-activations spread evenly over [-30, 30]: GELU(tanh) on every path that instantiates it, the others on T128X128."""
    B.run_gemm(_ops(dev), dev, c)


@pytest.mark.parametrize("c", B.splitk_cases() + B.row_split_cases(), ids=ids(B.splitk_cases() + B.row_split_cases()))
def test_bf16_gemm_split_k_and_row_split(dev, c):
    """Tiles cut along K over the workspace (its status 0 afterwards) and rows cut at m0 into two launches: bias, two gates and a
    residual; bar (e) on every family."""
    B.run_gemm(_ops(dev), dev, c)


@pytest.mark.parametrize("c", B.skinny_cases(), ids=ids(B.skinny_cases()))
def test_skinny_gemm_against_fp64(dev, c):
    """bya_gemm_skinny_bf16: the restatement of bar (c) sums the kernel's 16 K ranges and adds them in wave order."""
    B.run_skinny(_ops(dev), dev, c)


@pytest.mark.parametrize("mode", B.ROWGEMM_MODES)
@pytest.mark.parametrize("M,N,form", B.ROWGEMM)
def test_rowgemm512_without_layernorm_against_fp64(dev, M, N, form, mode):
    B.run_rowgemm(_ops(dev), dev, M, N, form, mode)
