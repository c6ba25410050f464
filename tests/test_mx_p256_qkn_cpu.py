"""CPU: the MX q|k|v projection with the q/k-norm + RoPE epilogue on the persistent 256 x 256 kernel (include/bya.h,
bya_gemm_mx_qkv_norm_rope_on / bya_gemm_mx_qkv_norm_rope_on_plan; ops.gemm_mx_qkv_norm_rope(..., kernel=)) -- declared,
exported, bound; which kernel the `kernel` ARGUMENT takes, asked through the plan query on meta tensors (every check runs
before any launch, so without a GPU).  Option mx_kernel has no say.  tests/test_mx_p256_qkn_gpu.py checks the bits."""
import ctypes
import os
import re

import pytest

from test_mx_qkn_cpu import BASE, E2M3, E4M3, ERR_SHAPE, ERR_UNSUPPORTED, OK, lib_and_hip, meta_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan(*a, kernel=0, **kw):
    from bind_your_avatar_implementation_amd import ops
    return ops.gemm_mx_qkv_norm_rope_plan(**meta_args(*a, **kw), kernel=kernel)


def test_symbols_are_declared_exported_and_bound():
    lib, _hip = lib_and_hip()
    header = open(os.path.join(ROOT, "include", "bya.h")).read()
    want = "A, a_scales, W, w_scales, bias, C, fmt, w_fmt, desc, norm, kernel".split(", ")
    for name, last in (("bya_gemm_mx_qkv_norm_rope_on", "stream"), ("bya_gemm_mx_qkv_norm_rope_on_plan", "plan")):
        m = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/bya.h"
        args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert args == want + [last], args
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name]) == 12
        fn = getattr(lib, name)                                          # exported (AttributeError otherwise)
        assert fn.argtypes is not None and len(fn.argtypes) == 12
        # the arguments of the existing pair plus `kernel` in front of the last one
        old = _hip.SIGNATURES[name.replace("_on", "")]
        assert _hip.SIGNATURES[name] == old[:-1] + [ctypes.c_int32] + old[-1:]


def test_the_kernel_argument_picks_the_persistent_kernel():
    lib_and_hip()
    whole = {"m0": 0, "tail": None, "split_k": 0, "row_chunks": 1}
    big = (17776, 3072, 3072)
    for kernel, want in ((0, "t128x128"), (1, "p256"), (2, "p256")):
        assert plan(*big, "mxfp8", text=226, kernel=kernel) == {"path": want, **whole}
    # q | k alone, the column-block form and a batch ride along
    assert plan(*big, "mxfp8", tensors=2, kernel=1)["path"] == "p256"
    assert plan(2222, 3072, 3072, "mxfp8", split=(768, 2222 * 768), kernel=1)["path"] == "p256"     # 9 x 36 tiles
    assert plan(300, 192, 512, "mxfp8", batch=2, text=300, kernel=2)["path"] == "p256"
    # width % 64 == 0 is enough here too
    assert plan(300, 192, 512, "mxfp8", kernel=2)["path"] == "p256" and plan(300, 1216, 512, "mxfp8", kernel=2)["path"] == "p256"


def test_other_formats_stay_on_the_tiled_kernel():
    lib_and_hip()
    for kernel in (0, 1, 2):
        assert plan(17776, 3072, 3072, "mxfp6", text=226, kernel=kernel)["path"] == "t256x256"
        assert plan(300, 3072, 3072, "mxfp6", text=226, kernel=kernel)["path"] == "t128x128"
        assert plan(17776, 3072, 3072, "mxfp6", "mxfp4", kernel=kernel)["path"] == "t256x256"
        assert plan(17776, 3072, 3072, "mxfp8", "mxfp4", text=226, kernel=kernel)["path"] == "t128x128"


def test_tile_count_and_k_tile_count():
    lib_and_hip()
    # 2 x 36 = 72 tiles of 256 x 256: fewer than 200
    assert plan(300, 3072, 3072, "mxfp8", text=226, kernel=1)["path"] == "t128x128"
    assert plan(300, 3072, 3072, "mxfp8", text=226, kernel=2)["path"] == "p256"
    # fewer than four K-tiles: the persistent kernel's ring does not take it
    assert plan(17776, 3072, 256, "mxfp8", kernel=2)["path"] == "t128x128"
    assert plan(17776, 3072, 384, "mxfp8", kernel=1)["path"] == "t128x128"
    assert plan(17776, 3072, 512, "mxfp8", kernel=1)["path"] == "p256"


def test_kernel_values_outside_0_1_2_are_refused():
    lib, _hip = lib_and_hip()
    for bad in (3, -1, 7):
        with pytest.raises(Exception):
            plan(17776, 3072, 3072, "mxfp8", kernel=bad)
    # ... with BYA_ERR_SHAPE, by the plan query and by the entry point alike, before anything else is looked at
    d, n, p = _hip.GemmDesc(), _hip.QkNormDesc(), _hip.GemmPlan(-9, -9, -9, -9, -9)
    args = (BASE, BASE, BASE, BASE, None, BASE, E4M3, E4M3, ctypes.byref(d), ctypes.byref(n))
    assert lib.bya_gemm_mx_qkv_norm_rope_on_plan(*args, 3, ctypes.byref(p)) == ERR_SHAPE and p.path == -9
    assert lib.bya_gemm_mx_qkv_norm_rope_on(*args, 3, None) == ERR_SHAPE
    assert lib.bya_gemm_mx_qkv_norm_rope_on_plan(*args, 1, None) == ERR_SHAPE


def test_option_mx_kernel_has_no_say():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    with ops.options(mx_kernel=2):
        assert plan(17776, 3072, 3072, "mxfp8", text=226, kernel=0)["path"] == "t128x128"
        assert plan(17776, 3072, 3072, "mxfp8", text=226)["path"] == "t128x128"
        assert plan(300, 3072, 3072, "mxfp8", text=226, kernel=1)["path"] == "t128x128"     # the tile count still holds
    with ops.options(mx_kernel=0):
        assert plan(17776, 3072, 3072, "mxfp8", text=226, kernel=1)["path"] == "p256"


def test_errors_are_those_of_the_existing_entry_point():
    """What bya_gemm_mx_qkv_norm_rope refuses, the new pair refuses with the same code under every kernel value."""
    lib, _hip = lib_and_hip()

    def both(kernel, fmt=E4M3, w_fmt=E4M3, M=300, width=128, K=512, **over):
        d, n = _hip.GemmDesc(), _hip.QkNormDesc()
        d.M, d.N, d.K, d.batch = M, 3 * width, K, 1
        d.lda, d.ldw, d.ldc = K, K, width
        d.n_split, d.c_split_stride, d.alpha = width, M * width, 1.0
        n.qw = n.qb = n.kw = n.kb = n.cos = n.sin = BASE
        n.text_rows, n.width, n.eps, n.k_scale = 40, width, 1e-6, 0.18
        ptr = dict(A=BASE, a_scales=BASE, W=BASE, w_scales=BASE, bias=BASE, C=BASE)
        for k, v in over.items():
            if k in ptr:
                ptr[k] = v
            elif hasattr(n, k):
                setattr(n, k, v)
            else:
                setattr(d, k, v)
        common = (*ptr.values(), fmt, w_fmt, ctypes.byref(d), ctypes.byref(n))
        p0, p1 = _hip.GemmPlan(-9, -9, -9, -9, -9), _hip.GemmPlan(-9, -9, -9, -9, -9)
        rc_old = lib.bya_gemm_mx_qkv_norm_rope_plan(*common, ctypes.byref(p0))
        rc_new = lib.bya_gemm_mx_qkv_norm_rope_on_plan(*common, kernel, ctypes.byref(p1))
        assert rc_new == rc_old, (over, kernel)
        if rc_new != OK:
            assert lib.bya_gemm_mx_qkv_norm_rope_on(*common, kernel, None) == rc_new            # refused before any launch
            assert p1.path == -9
        return rc_new, p1.path

    for kernel in (0, 1, 2):
        assert both(kernel)[0] == OK
        assert both(kernel, act=1)[0] == ERR_UNSUPPORTED and both(kernel, n_split=0)[0] == ERR_UNSUPPORTED
        assert both(kernel, fmt=E4M3, w_fmt=E2M3)[0] == ERR_UNSUPPORTED
        assert both(kernel, A=None)[0] == ERR_SHAPE and both(kernel, cos=None)[0] == ERR_SHAPE and both(kernel, K=192)[0] == ERR_SHAPE
        assert both(kernel, C=BASE + 8)[0] == -2 and both(kernel, ldc=132)[0] == -2
    assert both(2)[1] == 4 and both(1)[1] == 1 and both(0)[1] == 1
    # a bias the persistent kernel's 16-byte loads cannot take (8-byte aligned is legal for the tiled kernel): tiled, not refused
    assert both(2, bias=BASE + 8) == (OK, 1)
    assert both(2, fmt=E2M3, w_fmt=E2M3, lda=512 * 6 // 8, ldw=512 * 6 // 8) == (OK, 1)
