"""CPU: the C ABI of the fp8 q|k|v projection whose epilogue norms and rotates q and k (include/bya.h,
bya_gemm_fp8_qkv_norm_rope / bya_gemm_fp8_qkv_norm_rope_plan) -- declared, exported, bound; the plan query and every argument
check run before any launch, so they run here, without a GPU; the Python front end (ops.gemm_fp8_qkv_norm_rope_plan on meta
tensors, enable_fp8_weights(fuse_qk_norm=...)).  tests/test_fp8_qkn_gpu.py checks the bits."""
import ctypes
import os
import re
import types

import pytest
import torch

OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
T128X128, P256 = "t128x128", "p256"
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
    want = "A8, a_scale, W8, w_scale, bias, C, desc, norm".split(", ")
    for name, last in (("bya_gemm_fp8_qkv_norm_rope", "stream"), ("bya_gemm_fp8_qkv_norm_rope_plan", "plan")):
        m = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/bya.h"
        args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert args == want + [last], args
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name]) == 9
        fn = getattr(lib, name)                                          # exported (AttributeError otherwise)
        assert fn.argtypes is not None and len(fn.argtypes) == 9
    sig = _hip.SIGNATURES["bya_gemm_fp8_qkv_norm_rope_plan"]
    assert sig[6:] == [ctypes.POINTER(_hip.GemmDesc), ctypes.POINTER(_hip.QkNormDesc), ctypes.POINTER(_hip.GemmPlan)]
    # the plain fp8 entry point stands as it was
    assert len(re.search(r"\bint bya_gemm_fp8\(([^;]*)\);", header).group(1).split(",")) == 11


def meta_args(M, width, K, tensors=3, batch=1, text=0, split=None):
    """Meta tensors standing for the operands of one launch: the keyword arguments of ops.gemm_fp8_qkv_norm_rope_plan."""
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device="meta")
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device="meta")
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device="meta")
    N = tensors * width
    lead = (batch, M) if batch > 1 else (M,)
    out = bf(tensors, *lead, width)
    cos = f32(M - text, 64) if text < M else None
    return dict(a8=u8(*lead, K), a_scale=f32(*lead), w8=u8(N, K), w_scale=f32(N), out=out[0], bias=bf(N),
                split=(width, batch * M * width) if split is None else split, qw=bf(64), qb=bf(64), kw=bf(64), kb=bf(64),
                cos=cos, sin=cos, text_rows=text, eps=1e-6, k_scale=0.18, tensors=tensors)


def plain_plan(ops, kw):
    """What ops.gemm_fp8 would run for the same operands: the fused launch must follow it."""
    return ops.gemm_fp8_plan(kw["a8"], kw["a_scale"], kw["w8"], kw["w_scale"], kw["out"], bias=kw["bias"], split=kw["split"])


def test_plan_query_follows_the_plain_fp8_gemm():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    whole = {"m0": 0, "tail": None, "split_k": 0, "row_chunks": 1}
    plan = lambda *a, **kw: ops.gemm_fp8_qkv_norm_rope_plan(**meta_args(*a, **kw))
    assert plan(300, 128, 256, text=40) == {"path": T128X128, **whole}
    assert plan(4400, 1216, 512, text=226) == {"path": P256, **whole}                     # 18 x 15 = 270 tiles of 256 x 256
    with ops.options(fp8_kernel=1):
        assert plan(4400, 1216, 512, text=226) == {"path": T128X128, **whole}
    assert plan(4400, 1216, 384, text=226) == {"path": T128X128, **whole}                 # fewer than four K-tiles
    # ... the step's shapes, q | k alone, a column block, a batch, all text
    assert plan(17776, 3072, 3072, text=226) == {"path": P256, **whole}
    assert plan(2222, 3072, 3072, text=226) == {"path": P256, **whole}                    # 9 x 36
    assert plan(2222, 3072, 3072, tensors=2, text=226) == {"path": P256, **whole}         # 9 x 24 = 216
    assert plan(5200, 1216, 512, tensors=2, text=226) == {"path": P256, **whole}          # 21 x 10 = 210
    assert plan(3500, 1280, 512, text=40, split=(320, 3500 * 320)) == {"path": P256, **whole}
    assert plan(1800, 1216, 512, batch=2, text=40) == {"path": P256, **whole}             # 2 x 8 x 15 = 240
    assert plan(300, 192, 256, batch=2, text=300) == {"path": T128X128, **whole}          # all text: no rotary tables
    # the same answer as the plain GEMM's query, in both option states
    for a, kw in (((300, 128, 256), {}), ((4400, 1216, 512), dict(text=226)), ((3700, 1216, 512), dict(text=3700)),
                  ((2222, 3072, 3072), dict(tensors=2))):
        for opt in (0, 1):
            with ops.options(fp8_kernel=opt):
                m = meta_args(*a, **kw)
                assert ops.gemm_fp8_qkv_norm_rope_plan(**m)["path"] == plain_plan(ops, m)["path"], (a, kw, opt)


def test_shapes_the_entry_point_declines():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    plan = ops.gemm_fp8_qkv_norm_rope_plan
    bf = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device="meta")
    assert plan(**meta_args(300, 96, 256)) is None                                        # width 96: no whole heads
    assert plan(**meta_args(300, 128, 256), act="gelu_tanh") is None                      # an activation
    assert plan(**meta_args(300, 128, 256), alpha=0.5) is None
    assert plan(**meta_args(300, 128, 256), res=bf(300, 384)) is None                     # a residual
    assert plan(**meta_args(300, 128, 256, split=(0, 0))) is None                         # n_split = 0: one packed tensor
    assert plan(**meta_args(300, 128, 256)) is not None
    with pytest.raises(ValueError):
        plan(**{**meta_args(300, 128, 256), "tensors": 4})
    with pytest.raises(ValueError):
        plan(**{**meta_args(300, 128, 256), "split": None})


def raw(lib, _hip, M=300, width=128, K=256, tensors=3, **over):
    d, n, p = _hip.GemmDesc(), _hip.QkNormDesc(), _hip.GemmPlan(-9, -9, -9, -9, -9)
    d.M, d.N, d.K, d.batch = M, tensors * width, K, 1
    d.lda, d.ldw, d.ldc = K, K, width
    d.n_split, d.c_split_stride, d.alpha = width, M * width, 1.0
    n.qw = n.qb = n.kw = n.kb = n.cos = n.sin = BASE
    n.text_rows, n.width, n.eps, n.k_scale = 40, width, 1e-6, 0.18
    ptr = dict(A8=BASE, a_scale=BASE, W8=BASE, w_scale=BASE, bias=BASE, C=BASE)
    for k, v in over.items():
        if k in ptr:
            ptr[k] = v
        elif hasattr(n, k) and k not in ("M", "N", "K"):
            setattr(n, k, v)
        else:
            setattr(d, k, v)
    rc = lib.bya_gemm_fp8_qkv_norm_rope_plan(*ptr.values(), ctypes.byref(d), ctypes.byref(n), ctypes.byref(p))
    # the entry point runs the same checks before it launches: whatever the query refuses, it refuses with the same code
    if rc != OK:
        assert lib.bya_gemm_fp8_qkv_norm_rope(*ptr.values(), ctypes.byref(d), ctypes.byref(n), None) == rc
        assert (p.path, p.m0, p.tail, p.split_k, p.row_chunks) == (-9, -9, -9, -9, -9)   # untouched on rejection
    return rc, p


def test_validation_table_runs_before_any_launch():
    lib, _hip = lib_and_hip()
    paths = {v: k for k, v in _hip.GEMM_PATHS.items()}
    rc, p = raw(lib, _hip)
    assert rc == OK and (p.path, p.m0, p.tail, p.split_k, p.row_chunks) == (paths[T128X128], 0, -1, 0, 1)
    rc, p = raw(lib, _hip, M=4400, width=1216, K=512, c_split_stride=4400 * 1216)
    assert rc == OK and (p.path, p.m0, p.tail, p.split_k, p.row_chunks) == (paths[P256], 0, -1, 0, 1)
    assert raw(lib, _hip, tensors=2)[0] == OK
    assert raw(lib, _hip, k_scale=0.0)[0] == OK and raw(lib, _hip, alpha=0.0)[0] == OK    # 0 is read as 1
    assert raw(lib, _hip, bias=None)[0] == OK
    # declined: the caller keeps the two launches
    for kw in (dict(width=96), dict(act=1), dict(n_split=0), dict(alpha=0.5), dict(bias_rowscale=BASE), dict(N=4 * 128),
               dict(N=128), dict(ldres=384), dict(res_batch_stride=8),
               dict(M=1 << 23, text_rows=0)):                                              # rows past one descriptor's reach
        assert raw(lib, _hip, **kw)[0] == ERR_UNSUPPORTED, kw
    assert raw(lib, _hip, act=2)[0] == ERR_UNSUPPORTED                                    # (bya_gemm_fp8's own refusal)
    big = dict(M=1 << 22, width=3072, c_split_stride=(1 << 22) * 3072)                    # 24 GiB of q: rows out of reach
    assert raw(lib, _hip, **big)[0] == ERR_UNSUPPORTED
    # rotary rows: [M - text_rows, 64] fp32 of 2 GiB or more is out of the table descriptors' reach.  (For the rows of C to be
    # in reach at that M the row stride must be 64 and the three tensors 64 elements apart: no check looks at their overlap)
    far = dict(M=(1 << 23) + 256, width=64, ldc=64, n_split=64, c_split_stride=64)
    assert raw(lib, _hip, text_rows=0, **far)[0] == ERR_UNSUPPORTED
    assert raw(lib, _hip, text_rows=512, **far)[0] == OK                                  # 2 GiB less 64 KiB of table
    # malformed: the errors of the fp8 GEMM and of the norm descriptor
    for kw in (dict(A8=None), dict(W8=None), dict(a_scale=None), dict(w_scale=None), dict(C=None), dict(qw=None), dict(qb=None),
               dict(kw=None), dict(kb=None), dict(cos=None), dict(sin=None), dict(text_rows=-1), dict(M=0), dict(K=192),
               dict(batch=0), dict(n_split=-4), dict(N=3 * 128 + 2)):
        assert raw(lib, _hip, **kw)[0] == ERR_SHAPE, kw
    assert raw(lib, _hip, cos=None, sin=None, text_rows=300)[0] == OK                     # all text: no tables needed
    for kw in (dict(A8=BASE + 8), dict(w_scale=BASE + 4), dict(C=BASE + 8), dict(qw=BASE + 8), dict(cos=BASE + 4), dict(ldc=132),
               dict(lda=264), dict(c_split_stride=300 * 128 + 4), dict(c_batch_stride=4), dict(bias=BASE + 4)):
        assert raw(lib, _hip, **kw)[0] == ERR_ALIGN, kw
    d, n = _hip.GemmDesc(), _hip.QkNormDesc()
    assert lib.bya_gemm_fp8_qkv_norm_rope_plan(BASE, BASE, BASE, BASE, None, BASE, ctypes.byref(d), ctypes.byref(n),
                                               None) == ERR_SHAPE
    assert lib.bya_gemm_fp8_qkv_norm_rope_plan(BASE, BASE, BASE, BASE, None, BASE, None, None,
                                               ctypes.byref(_hip.GemmPlan())) == ERR_SHAPE


def test_whatever_the_plain_gemm_refuses_is_refused_with_its_code():
    """The operand side is bya_gemm_fp8's: same descriptor (the residual-free one the fused entry point sees), same code."""
    lib, _hip = lib_and_hip()
    for kw in (dict(K=192), dict(M=0), dict(lda=264), dict(ldw=8), dict(A8=BASE + 8), dict(W8=None), dict(a_scale=None),
               dict(act=3), dict(n_split=-4), dict(n_split=130), dict(N=3 * 128 + 2)):
        d = _hip.GemmDesc()
        d.M, d.N, d.K, d.batch = 300, 384, 256, 1
        d.lda, d.ldw, d.ldc, d.n_split, d.c_split_stride, d.alpha = 256, 256, 128, 128, 300 * 128, 1.0
        ptr = dict(A8=BASE, a_scale=BASE, W8=BASE, w_scale=BASE, bias=BASE, C=BASE)
        for k, v in kw.items():
            if k in ptr:
                ptr[k] = v
            else:
                setattr(d, k, v)
        p = _hip.GemmPlan()
        plain = lib.bya_gemm_fp8_plan(*ptr.values(), None, None, None, ctypes.byref(d), ctypes.byref(p))
        assert plain != OK, kw
        assert raw(lib, _hip, **kw)[0] == plain, kw


def test_the_model_switch():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    enable = BindyouravatarTransformer3DModel.enable_fp8_weights
    calls = []
    fake = types.SimpleNamespace(invalidate_engine=lambda: calls.append(1))
    enable(fake)
    assert not hasattr(fake, "_fp8_fuse_qk_norm") and fake._fp8_weights is True and calls == [1]      # off by default
    enable(fake, fuse_qk_norm=True)
    assert fake._fp8_fuse_qk_norm is True and calls == [1, 1]                             # the switch invalidates the engine
    enable(fake, linears=("qkv", "out"), fuse_qk_norm=True)
    assert fake._fp8_linears == ("qkv", "out") and fake._fp8_fuse_qk_norm is True
    # keyword only; a non-bool is refused and leaves the model as it was
    before = dict(vars(fake))
    with pytest.raises(TypeError):
        enable(fake, True, None, True)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError):
            enable(fake, fuse_qk_norm=bad)
    assert vars(fake) == before and calls == [1, 1, 1]
    assert "fuse_qk_norm" in enable.__doc__
    enable(fake)                                                                          # ... and a plain call switches it off again
    assert not hasattr(fake, "_fp8_fuse_qk_norm")
    enable(fake, fuse_qk_norm=True)
    enable(fake, enabled=False, fuse_qk_norm=True)                                        # nothing to fuse into without fp8 weights
    assert fake._fp8_weights is False and not hasattr(fake, "_fp8_fuse_qk_norm")
    # the default leaves the model's attributes exactly as a call without the keyword always left them
    plain = types.SimpleNamespace(invalidate_engine=lambda: None)
    enable(plain, linears=("qkv",))
    assert vars(plain) == dict(invalidate_engine=plain.invalidate_engine, _fp8_weights=True, _fp8_linears=("qkv",))


def test_the_engine_reads_the_switch_only_with_fp8_weights():
    """DenoiseEngine.fp8_fuse_qk_norm = fp8 weights AND the model's switch (the constructor's own expression)."""
    import inspect
    from bind_your_avatar_implementation_amd import engine
    src = inspect.getsource(engine.DenoiseEngine.__init__)
    assert 'self.fp8_fuse_qk_norm = self.fp8_weights and bool(getattr(model, "_fp8_fuse_qk_norm", False))' in src
    assert "ops.gemm_fp8_qkv_norm_rope(" in inspect.getsource(engine.DenoiseEngine._qkv_norm_rope)
