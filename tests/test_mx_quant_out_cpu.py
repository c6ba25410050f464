"""CPU: the C ABI of the MX GEMM with the quantising epilogue (include/bya.h, bya_gemm_mx_quant / bya_gemm_mx_quant_plan) --
declared, exported, bound; every argument check runs before any launch, so it runs here, without a GPU; the plan query
reports the tile by bya_gemm_mx_mixed_plan's rule.  tests/test_mx_quant_out_gpu.py checks the bytes."""
import ctypes
import os
import re
import types

import pytest
import torch

E4M3, E2M3, E2M1 = 0, 2, 4
T128X128, T256X256 = 1, 3
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_and_hip():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    return _hip.load(), _hip


def test_error_codes_are_the_librarys():
    text = open(os.path.join(ROOT, "bind_your_avatar_implementation_amd", "csrc", "bya_common.h")).read()
    for name, val in (("BYA_ERR_SHAPE", ERR_SHAPE), ("BYA_ERR_ALIGN", ERR_ALIGN), ("BYA_ERR_UNSUPPORTED", ERR_UNSUPPORTED)):
        m = re.search(rf"#define {name} \((-?\d+)\)", text)
        assert m and int(m.group(1)) == val, name


def test_symbols_are_declared_exported_and_bound():
    lib, _hip = lib_and_hip()
    header = open(os.path.join(ROOT, "include", "bya.h")).read()
    for name, nargs in (("bya_gemm_mx_quant", 12), ("bya_gemm_mx_quant_plan", 12)):
        m = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/bya.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name]) == nargs
        fn = getattr(lib, name)                                          # exported (AttributeError otherwise)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    # no res / gate arguments: seven pointers, the descriptor, three formats, the stream or the plan
    decl = re.search(r"\bint bya_gemm_mx_quant\(([^;]*)\);", header).group(1)
    assert "res" not in decl and "gate" not in decl and "q_codes" in decl and "q_scales" in decl and "out_fmt" in decl


def desc(_hip, M=300, N=256, K=256, a_fmt=E2M3, w_fmt=None, out_fmt=E2M3, batch=1):
    w_fmt = a_fmt if w_fmt is None else w_fmt
    bits = {E4M3: 8, E2M3: 6, E2M1: 4}
    d = _hip.GemmDesc()
    d.M, d.N, d.K, d.batch = M, N, K, batch
    d.lda, d.ldw, d.ldc = K * bits[a_fmt] // 8, K * bits[w_fmt] // 8, N * bits.get(out_fmt, 8) // 8
    d.a_batch_stride, d.c_batch_stride = M * d.lda, M * d.ldc
    return d


def test_validation_table_runs_before_any_launch():
    lib, _hip = lib_and_hip()
    base = 1 << 40                                                        # never dereferenced: every call below is refused

    def call(d, a_fmt=E2M3, w_fmt=None, out_fmt=E2M3, A=base, sa=base, W=base, sw=base, qc=base, qs=base):
        return lib.bya_gemm_mx_quant(A, sa, W, sw, None, qc, qs, ctypes.byref(d) if d is not None else None, a_fmt,
                                     a_fmt if w_fmt is None else w_fmt, out_fmt, None)

    d = desc(_hip)
    # NULL pointers: BYA_ERR_SHAPE
    for kw in ({"A": None}, {"sa": None}, {"W": None}, {"sw": None}, {"qc": None}, {"qs": None}):
        assert call(d, **kw) == ERR_SHAPE, kw
    assert call(None) == ERR_SHAPE
    # N % 128 != 0: BYA_ERR_SHAPE (the result must be a legal K)
    for n in (64, 96, 192, 3700):
        assert call(desc(_hip, N=n)) == ERR_SHAPE, n
    # a code row stride below the row, K % 128, non-positive sizes: BYA_ERR_SHAPE
    short = desc(_hip)
    short.ldc = 176
    assert call(short) == ERR_SHAPE
    assert call(desc(_hip, K=192)) == ERR_SHAPE
    assert call(desc(_hip, M=0)) == ERR_SHAPE
    # misaligned codes or scales, code strides that are no multiple of 16: BYA_ERR_ALIGN
    assert call(d, qc=base + 8) == ERR_ALIGN and call(d, qc=base + 1) == ERR_ALIGN
    assert call(d, qs=base + 2) == ERR_ALIGN and call(d, qs=base + 1) == ERR_ALIGN
    odd = desc(_hip)
    odd.ldc = 192 + 8
    assert call(odd) == ERR_ALIGN
    odd = desc(_hip, batch=2)
    odd.c_batch_stride += 8
    assert call(odd) == ERR_ALIGN
    # e2m1 output, unknown output formats, operand pairs bya_gemm_mx_mixed refuses, n_split: BYA_ERR_UNSUPPORTED
    assert call(d, out_fmt=E2M1) == ERR_UNSUPPORTED
    assert call(d, out_fmt=1) == ERR_UNSUPPORTED and call(d, out_fmt=3) == ERR_UNSUPPORTED
    assert call(desc(_hip, a_fmt=E2M1, w_fmt=E2M1), a_fmt=E2M1, w_fmt=E2M1) == ERR_UNSUPPORTED
    assert call(desc(_hip, a_fmt=E4M3, w_fmt=E2M3), a_fmt=E4M3, w_fmt=E2M3) == ERR_UNSUPPORTED
    assert call(desc(_hip, a_fmt=E2M3, w_fmt=E4M3), a_fmt=E2M3, w_fmt=E4M3) == ERR_UNSUPPORTED
    split = desc(_hip)
    split.n_split, split.c_split_stride = 128, 4096
    assert call(split) == ERR_UNSUPPORTED
    act = desc(_hip)
    act.act = 4                                                           # SiLU: not an activation of the DiT Linears
    assert call(act) == ERR_UNSUPPORTED
    # the same table through the plan query
    pl = _hip.GemmPlan(-9, -9, -9, -9, -9)
    assert lib.bya_gemm_mx_quant_plan(base, base, base, base, None, base, base, ctypes.byref(desc(_hip, N=192)), E2M3, E2M3,
                                      E2M3, ctypes.byref(pl)) == ERR_SHAPE
    assert lib.bya_gemm_mx_quant_plan(base, base, base, base, None, base + 8, base, ctypes.byref(d), E2M3, E2M3, E2M3,
                                      ctypes.byref(pl)) == ERR_ALIGN
    assert lib.bya_gemm_mx_quant_plan(base, base, base, base, None, base, base, ctypes.byref(d), E2M3, E2M3, E2M1,
                                      ctypes.byref(pl)) == ERR_UNSUPPORTED
    assert (pl.path, pl.m0, pl.tail, pl.split_k, pl.row_chunks) == (-9, -9, -9, -9, -9)        # untouched on rejection


def test_plan_query_follows_the_mixed_gemm_rule():
    lib, _hip = lib_and_hip()
    base = 1 << 40
    pl, pm = _hip.GemmPlan(-9, -9, -9, -9, -9), _hip.GemmPlan(-9, -9, -9, -9, -9)

    def plans(a_fmt, w_fmt, out_fmt, M, N, K=256, batch=1):
        d = desc(_hip, M, N, K, a_fmt, w_fmt, out_fmt, batch)
        rc = lib.bya_gemm_mx_quant_plan(base, base, base, base, None, base, base, ctypes.byref(d), a_fmt, w_fmt, out_fmt,
                                        ctypes.byref(pl))
        d.ldc, d.c_batch_stride = N, M * N                                # the bf16 launch: ldc in elements
        rm = lib.bya_gemm_mx_mixed_plan(base, base, base, base, None, base, None, None, None, ctypes.byref(d), a_fmt, w_fmt,
                                        ctypes.byref(pm))
        assert rc == OK and rm == OK
        assert pl.path == pm.path
        return pl.path

    for out_fmt in (E4M3, E2M3):
        assert plans(E2M3, E2M3, out_fmt, 3500, 3712) == T256X256         # 14 x 15 = 210 tiles of 256 x 256
        assert plans(E2M3, E2M1, out_fmt, 3500, 3712) == T256X256
        assert plans(E2M3, E2M3, out_fmt, 3500, 3584) == T128X128         # 14 x 14 = 196 < 200
        assert plans(E2M3, E2M1, out_fmt, 300, 256) == T128X128
        assert plans(E2M3, E2M3, out_fmt, 2600, 2560) == T128X128         # 11 x 10 = 110 ...
        assert plans(E2M3, E2M3, out_fmt, 2600, 2560, batch=2) == T256X256   # ... and 220 with the batch
        assert plans(E4M3, E4M3, out_fmt, 3500, 3712) == T128X128         # e4m3 activations: always the 128 x 128 tile
        assert plans(E4M3, E2M1, out_fmt, 17, 128) == T128X128
    assert plans(E2M3, E2M3, E2M3, 17776, 12288, K=3072) == T256X256      # ff.net.0 at one GPU
    assert (pl.m0, pl.tail, pl.split_k, pl.row_chunks) == (0, -1, 0, 1)
    d = desc(_hip)
    assert lib.bya_gemm_mx_quant_plan(base, base, base, base, None, base, base, ctypes.byref(d), E2M3, E2M3, E2M3, None) \
        == ERR_SHAPE


def test_python_front_end_and_the_model_switch():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel, ops
    meta = lambda *s: torch.empty(*s, dtype=torch.uint8, device="meta")
    for fmt, w_fmt, expect in (("mxfp6", None, "t256x256"), ("mxfp6", "mxfp4", "t256x256"), ("mxfp8", None, "t128x128")):
        for out_fmt in ("mxfp6", "mxfp8"):
            args = (meta(3500, ops.mx_code_bytes(256, fmt)), meta(3500, 8), meta(3712, ops.mx_code_bytes(256, w_fmt or fmt)),
                    meta(3712, 8), meta(3500, ops.mx_code_bytes(3712, out_fmt)), meta(3500, 116), fmt)
            assert ops.gemm_mx_quant_plan(*args, w_fmt=w_fmt, out_fmt=out_fmt, act="gelu_tanh")["path"] == expect
    with pytest.raises(ValueError):                                       # e2m1 is never an output format
        ops.gemm_mx_quant_plan(meta(300, 192), meta(300, 8), meta(256, 192), meta(256, 8), meta(300, 128), meta(300, 8),
                               "mxfp6", out_fmt="mxfp4")
    with pytest.raises(ValueError):                                       # an output pair of the wrong size
        ops.gemm_mx_quant_plan(meta(300, 192), meta(300, 8), meta(256, 192), meta(256, 8), meta(300, 256), meta(300, 8),
                               "mxfp6", out_fmt="mxfp6")
    # the switch: keyword only, on by default, invalidates the engine like every other argument
    enable = BindyouravatarTransformer3DModel.enable_mx_weights
    calls = []
    fake = types.SimpleNamespace(invalidate_engine=lambda: calls.append(1))
    enable(fake, "mxfp6")
    assert fake._mx_fuse_activation_quant is True and calls == [1]
    enable(fake, "mxfp6", fuse_activation_quant=False)
    assert fake._mx_fuse_activation_quant is False and calls == [1, 1]
    with pytest.raises(TypeError):
        enable(fake, "mxfp6", True, None, None, False)
    assert calls == [1, 1]
