"""CPU: the C ABI of the MX q|k|v projection whose epilogue norms and rotates q and k (include/bya.h,
bya_gemm_mx_qkv_norm_rope / bya_gemm_mx_qkv_norm_rope_plan) -- declared, exported, bound; the plan query and every argument
check run before any launch, so they run here, without a GPU; the Python front end (ops.gemm_mx_qkv_norm_rope_plan on meta
tensors, enable_mx_weights(fuse_qk_norm=...)).  tests/test_mx_qkn_gpu.py checks the bits."""
import ctypes
import os
import re
import types

import pytest
import torch

E4M3, E2M3, E2M1 = 0, 2, 4
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
BITS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1 << 40                                                            # never dereferenced: nothing below launches


def lib_and_hip():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    return _hip.load(), _hip


def test_symbols_are_declared_exported_and_bound():
    lib, _hip = lib_and_hip()
    header = open(os.path.join(ROOT, "include", "bya.h")).read()
    want = "A, a_scales, W, w_scales, bias, C, fmt, w_fmt, desc, norm".split(", ")
    for name, last in (("bya_gemm_mx_qkv_norm_rope", "stream"), ("bya_gemm_mx_qkv_norm_rope_plan", "plan")):
        m = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/bya.h"
        args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert args == want + [last], args
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name]) == 11
        fn = getattr(lib, name)                                          # exported (AttributeError otherwise)
        assert fn.argtypes is not None and len(fn.argtypes) == 11
    sig = _hip.SIGNATURES["bya_gemm_mx_qkv_norm_rope_plan"]
    assert sig[6:8] == [ctypes.c_int32, ctypes.c_int32]
    assert sig[8:] == [ctypes.POINTER(_hip.GemmDesc), ctypes.POINTER(_hip.QkNormDesc), ctypes.POINTER(_hip.GemmPlan)]
    # the bf16 entry point and the descriptor stand as they were
    assert len(re.search(r"\bint bya_gemm_qkv_norm_rope\(([^;]*)\);", header).group(1).split(",")) == 7


def meta_args(M, width, K, fmt, w_fmt=None, tensors=3, batch=1, text=0, split=None):
    """Meta tensors standing for the operands of one launch: the keyword arguments of ops.gemm_mx_qkv_norm_rope_plan."""
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device="meta")
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device="meta")
    N = tensors * width
    lead = (batch, M) if batch > 1 else (M,)
    out = bf(tensors, *lead, width)
    cos = torch.empty(M - text, 64, dtype=torch.float32, device="meta") if text < M else None
    return dict(a_codes=u8(*lead, K * BITS[fmt] // 8), a_scales=u8(*lead, K // 32),
                w_codes=u8(N, K * BITS[w_fmt or fmt] // 8), w_scales=u8(N, K // 32), out=out[0], bias=bf(N),
                split=(width, batch * M * width) if split is None else split, qw=bf(64), qb=bf(64), kw=bf(64), kb=bf(64),
                cos=cos, sin=cos, text_rows=text, eps=1e-6, k_scale=0.18, tensors=tensors, fmt=fmt, w_fmt=w_fmt)


def test_plan_query_reports_the_tile_of_the_activation_format():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    plan = lambda *a, **kw: ops.gemm_mx_qkv_norm_rope_plan(**meta_args(*a, **kw))
    whole = {"m0": 0, "tail": None, "split_k": 0, "row_chunks": 1}
    assert plan(17776, 3072, 3072, "mxfp8", text=226) == {"path": "t128x128", **whole}
    assert plan(17776, 3072, 3072, "mxfp6", text=226) == {"path": "t256x256", **whole}
    assert plan(300, 3072, 3072, "mxfp6", text=226) == {"path": "t128x128", **whole}
    # ... whatever the weights' format, for q | k alone, for a column block and for a batch
    assert plan(17776, 3072, 3072, "mxfp8", "mxfp4")["path"] == "t128x128"
    assert plan(17776, 3072, 3072, "mxfp6", "mxfp4")["path"] == "t256x256"
    assert plan(17776, 3072, 3072, "mxfp6", tensors=2)["path"] == "t256x256"
    assert plan(2222, 3072, 3072, "mxfp6", split=(768, 2222 * 768))["path"] == "t256x256"       # 9 x 36 tiles of 256 x 256
    assert plan(300, 192, 256, "mxfp8", batch=2, text=300)["path"] == "t128x128"       # all text: no rotary tables
    # width % 64 == 0 is enough (the bf16 entry point asks for % 128)
    assert plan(300, 192, 256, "mxfp6") is not None and plan(300, 1216, 256, "mxfp6") is not None


def test_shapes_the_entry_point_declines():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    plan = ops.gemm_mx_qkv_norm_rope_plan
    assert plan(**meta_args(300, 96, 256, "mxfp6")) is None                              # width 96: no whole heads
    assert plan(**meta_args(300, 128, 256, "mxfp6"), act="gelu_tanh") is None            # an activation
    assert plan(**meta_args(300, 128, 256, "mxfp6"), alpha=0.5) is None
    assert plan(**meta_args(300, 128, 256, "mxfp6", split=(0, 0))) is None               # n_split = 0: one packed tensor
    assert plan(**meta_args(300, 128, 256, "mxfp6")) is not None
    with pytest.raises(ValueError):                                                       # e2m1 activations: the front end refuses
        plan(**meta_args(300, 128, 256, "mxfp4"))


def raw(lib, _hip, M=300, width=128, K=256, fmt=E2M3, w_fmt=E2M3, tensors=3, **over):
    bits = {E4M3: 8, E2M3: 6, E2M1: 4}
    d, n, p = _hip.GemmDesc(), _hip.QkNormDesc(), _hip.GemmPlan(-9, -9, -9, -9, -9)
    d.M, d.N, d.K, d.batch = M, tensors * width, K, 1
    d.lda, d.ldw, d.ldc = K * bits.get(fmt, 8) // 8, K * bits.get(w_fmt, 8) // 8, width
    d.n_split, d.c_split_stride, d.alpha = width, M * width, 1.0
    n.qw = n.qb = n.kw = n.kb = n.cos = n.sin = BASE
    n.text_rows, n.width, n.eps, n.k_scale = 40, width, 1e-6, 0.18
    ptr = dict(A=BASE, a_scales=BASE, W=BASE, w_scales=BASE, bias=BASE, C=BASE)
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v
        elif hasattr(n, k) and k not in ("M", "N", "K"):
            setattr(n, k, v)
        else:
            setattr(d, k, v)
    rc = lib.bya_gemm_mx_qkv_norm_rope_plan(*ptr.values(), fmt, w_fmt, ctypes.byref(d), ctypes.byref(n), ctypes.byref(p))
    # the entry point runs the same checks before it launches: whatever the query refuses, it refuses with the same code
    if rc != OK:
        assert lib.bya_gemm_mx_qkv_norm_rope(*ptr.values(), fmt, w_fmt, ctypes.byref(d), ctypes.byref(n), None) == rc
        assert (p.path, p.m0, p.tail, p.split_k, p.row_chunks) == (-9, -9, -9, -9, -9)   # untouched on rejection
    return rc, p


def test_validation_table_runs_before_any_launch():
    lib, _hip = lib_and_hip()
    rc, p = raw(lib, _hip)
    assert rc == OK and (p.path, p.m0, p.tail, p.split_k, p.row_chunks) == (1, 0, -1, 0, 1)
    assert raw(lib, _hip, fmt=E4M3, w_fmt=E2M1)[0] == OK and raw(lib, _hip, tensors=2)[0] == OK
    assert raw(lib, _hip, k_scale=0.0)[0] == OK                                           # 0 is read as 1
    # declined: the caller keeps the two launches
    for kw in (dict(width=96), dict(act=1), dict(n_split=0), dict(fmt=E2M1, w_fmt=E2M1), dict(fmt=E4M3, w_fmt=E2M3),
               dict(alpha=0.5), dict(bias_rowscale=BASE), dict(N=4 * 128),
               dict(M=1 << 23, text_rows=0)):                                              # rows past one descriptor's reach
        assert raw(lib, _hip, **kw)[0] == ERR_UNSUPPORTED, kw
    big = dict(M=1 << 22, width=3072, c_split_stride=(1 << 22) * 3072)                    # 24 GiB of q: rows out of reach
    assert raw(lib, _hip, **big)[0] == ERR_UNSUPPORTED
    # malformed: the errors of the MX GEMM and of the norm descriptor
    for kw in (dict(A=None), dict(W=None), dict(a_scales=None), dict(w_scales=None), dict(C=None), dict(qw=None), dict(kb=None),
               dict(cos=None), dict(sin=None), dict(text_rows=-1), dict(M=0), dict(K=192), dict(batch=0), dict(lda=16),
               dict(n_split=-4)):
        assert raw(lib, _hip, **kw)[0] == ERR_SHAPE, kw
    assert raw(lib, _hip, cos=None, sin=None, text_rows=300)[0] == OK                     # all text: no tables needed
    for kw in (dict(A=BASE + 8), dict(a_scales=BASE + 2), dict(C=BASE + 8), dict(qw=BASE + 8), dict(cos=BASE + 4), dict(ldc=132),
               dict(c_split_stride=300 * 128 + 4), dict(c_batch_stride=4), dict(bias=BASE + 4)):
        assert raw(lib, _hip, **kw)[0] == ERR_ALIGN, kw
    d, n = _hip.GemmDesc(), _hip.QkNormDesc()
    assert lib.bya_gemm_mx_qkv_norm_rope_plan(BASE, BASE, BASE, BASE, None, BASE, E2M3, E2M3, ctypes.byref(d), ctypes.byref(n),
                                              None) == ERR_SHAPE
    assert lib.bya_gemm_mx_qkv_norm_rope_plan(BASE, BASE, BASE, BASE, None, BASE, E2M3, E2M3, None, None,
                                              ctypes.byref(_hip.GemmPlan())) == ERR_SHAPE


def test_the_model_switch():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    enable = BindyouravatarTransformer3DModel.enable_mx_weights
    calls = []
    fake = types.SimpleNamespace(invalidate_engine=lambda: calls.append(1))
    enable(fake, "mxfp6")
    assert fake._mx_fuse_qk_norm is False and calls == [1]                                # off by default
    assert fake._mx_fuse_attention_quant is False and fake._mx_fuse_activation_quant is True      # ... and the others as before
    enable(fake, "mxfp6", fuse_qk_norm=True)
    assert fake._mx_fuse_qk_norm is True and fake._mx_fuse_attention_quant is False and calls == [1, 1]
    enable(fake, "mxfp8", weight_format="mxfp4", fuse_qk_norm=True, fuse_attention_quant=True)
    assert (fake._mx_weights, fake._mx_weight_format, fake._mx_fuse_qk_norm, fake._mx_fuse_attention_quant) == \
        ("mxfp8", "mxfp4", True, True)
    # keyword only; a non-bool is refused and leaves the model as it was
    before = dict(vars(fake))
    with pytest.raises(TypeError):
        enable(fake, "mxfp6", True, None, None, True, False, True)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError):
            enable(fake, "mxfp6", fuse_qk_norm=bad)
    assert vars(fake) == before and calls == [1, 1, 1]
    assert "fuse_qk_norm" in enable.__doc__
    # the default leaves the engine's semantics untouched: the call without the keyword sets what it set before, plus False
    plain = types.SimpleNamespace(invalidate_engine=lambda: None)
    enable(plain, "mxfp6", linears=("qkv",), weight_format="mxfp4")
    assert vars(plain) == dict(invalidate_engine=plain.invalidate_engine, _mx_weights="mxfp6", _mx_weight_format="mxfp4",
                               _mx_linears=("qkv",), _mx_fuse_activation_quant=True, _mx_fuse_attention_quant=False,
                               _mx_fuse_qk_norm=False)
