"""CPU: bya_gemm_mx_call / bya_gemm_mx_call_plan (include/bya.h; ops.gemm_mx_call, ops.gemm_mx_call_plan) -- any MX GEMM as one
call whose kernel is an ARGUMENT, and the one way mxfp4 (e2m1) weights under mxfp8 activations reach the persistent 256 x 256
kernel of csrc/gemm_mx_v4.hip.  Which kernel a call takes is asked through the plan query on meta tensors (every check runs
before any launch, so without a GPU); the errors are those of the old entry point of each epilogue; no option has a say; what
the older entry points answer for mxfp4 weights is as it was.  tests/test_mx_p256_w4_gpu.py checks the bits."""
import ctypes
import os
import subprocess
import sys
import types

import torch

from test_mx_p256_cpu import gemm_args, quant_args
from test_mx_qkn_cpu import BASE, E2M1, E2M3, E4M3, ERR_SHAPE, ERR_UNSUPPORTED, OK, lib_and_hip
from test_mx_qkn_cpu import meta_args as qkn_meta_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ALIGN = -2
KERNELS = (0, 1, 2)


def bf16_path(kernel, M, N, K, fmt="mxfp8", w_fmt="mxfp4", batch=1):
    from bind_your_avatar_implementation_amd import ops
    a = gemm_args(M, N, K, fmt, w_fmt, batch)
    return ops.gemm_mx_call_plan(a.pop("a_codes"), a.pop("a_scales"), a.pop("w_codes"), a.pop("w_scales"), a.pop("out"),
                                 kernel, **a)["path"]


def quant_path(kernel, M, N, K, fmt="mxfp8", w_fmt="mxfp4", out_fmt="mxfp8"):
    from bind_your_avatar_implementation_amd import ops
    a = quant_args(M, N, K, fmt, out_fmt)
    a["w_codes"] = torch.empty(N, K * {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}[w_fmt] // 8, dtype=torch.uint8, device="meta")
    return ops.gemm_mx_call_plan(a["a_codes"], a["a_scales"], a["w_codes"], a["w_scales"], a["out_codes"], kernel, fmt=fmt,
                                 w_fmt=w_fmt, bias=a["bias"], act=a["act"], out_scales=a["out_scales"], out_fmt=out_fmt)["path"]


def qkn_path(kernel, M, width, K, fmt="mxfp8", w_fmt="mxfp4", **kw):
    from bind_your_avatar_implementation_amd import ops
    a = qkn_meta_args(M, width, K, fmt, w_fmt, **kw)
    norm = {k: a[k] for k in ("qw", "qb", "kw", "kb", "cos", "sin", "text_rows", "eps", "k_scale", "tensors")}
    return ops.gemm_mx_call_plan(a["a_codes"], a["a_scales"], a["w_codes"], a["w_scales"], a["out"], kernel, fmt=fmt, w_fmt=w_fmt,
                                 bias=a["bias"], split=a["split"], norm=norm)["path"]


def test_symbols_and_struct_are_declared_exported_and_bound():
    lib, _hip = lib_and_hip()
    import re
    header = open(os.path.join(ROOT, "include", "bya.h")).read()
    body = re.search(r"typedef struct bya_mx_gemm_call \{(.*?)\} bya_mx_gemm_call;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",")]
    assert names == [f[0] for f in _hip.MxGemmCall._fields_], names
    assert ctypes.sizeof(_hip.MxGemmCall) == 11 * 8 + 4 * 4
    for name, last in (("bya_gemm_mx_call", ctypes.c_void_p), ("bya_gemm_mx_call_plan", ctypes.POINTER(_hip.GemmPlan))):
        assert re.search(rf"\bint {name}\(const bya_mx_gemm_call\* call, const bya_gemm_desc\* desc, ", header)
        assert _hip.SIGNATURES[name] == [ctypes.POINTER(_hip.MxGemmCall), ctypes.POINTER(_hip.GemmDesc), last]
        assert len(getattr(lib, name).argtypes) == 3


def test_mxfp4_weights_reach_the_persistent_kernel_under_every_epilogue():
    lib_and_hip()
    assert [bf16_path(k, 17776, 9216, 3072) for k in KERNELS] == ["t128x128", "p256", "p256"]
    assert [quant_path(k, 17776, 9216, 3072) for k in KERNELS] == ["t128x128", "p256", "p256"]
    assert [qkn_path(k, 17776, 3072, 3072, text=226) for k in KERNELS] == ["t128x128", "p256", "p256"]


def test_tile_count_k_tiles_and_alignment():
    lib_and_hip()
    assert [bf16_path(k, 300, 264, 512) for k in KERNELS] == ["t128x128", "t128x128", "p256"]       # 2 x 2 tiles
    assert bf16_path(2, 300, 264, 256) == "t128x128" and bf16_path(2, 300, 264, 384) == "t128x128"  # fewer than four K-tiles
    assert bf16_path(2, 300, 260, 512) == "t128x128"                                                # N % 8 != 0
    assert bf16_path(1, 1811, 3848, 640) == "t128x128"                                              # 8 x 16 = 128 tiles
    assert bf16_path(1, 1811, 3848, 640, batch=2) == "p256"                                         # the batch counts
    assert [quant_path(k, 300, 256, 512) for k in KERNELS] == ["t128x128", "t128x128", "p256"]
    assert [qkn_path(k, 300, 192, 512, text=40) for k in KERNELS] == ["t128x128", "t128x128", "p256"]


def test_other_formats_answer_as_ever():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    for k in KERNELS:
        assert quant_path(k, 17776, 12288, 3072, out_fmt="mxfp6") == "t128x128"                     # out e2m3: tiled
        assert bf16_path(k, 17776, 9216, 3072, "mxfp6", "mxfp6") == "t256x256"
        assert bf16_path(k, 300, 264, 512, "mxfp6", "mxfp6") == "t128x128"
        assert bf16_path(k, 17776, 9216, 3072, "mxfp6", "mxfp4") == "t256x256"
        assert bf16_path(k, 300, 264, 512, "mxfp6", "mxfp4") == "t128x128"
        assert quant_path(k, 17776, 12288, 3072, "mxfp6", "mxfp6", "mxfp6") == "t256x256"
        assert qkn_path(k, 17776, 3072, 3072, "mxfp6", "mxfp4") == "t256x256"
    # same-format mxfp8 through the new pair: what bya_gemm_mx_mixed_plan answers under option mx_kernel = 0 / 1 / 2
    for shape in ((17776, 9216, 3072), (300, 264, 512), (300, 264, 256), (300, 260, 512), (1811, 3848, 640)):
        for k in KERNELS:
            with ops.options(mx_kernel=k):
                want = ops.gemm_mx_plan(**gemm_args(*shape, "mxfp8"))
            a = gemm_args(*shape, "mxfp8")
            got = ops.gemm_mx_call_plan(a.pop("a_codes"), a.pop("a_scales"), a.pop("w_codes"), a.pop("w_scales"), a.pop("out"), k, **a)
            assert got == want, (shape, k)


def test_option_mx_kernel_has_no_say_and_the_old_pins_hold():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    with ops.options(mx_kernel=2):
        assert [bf16_path(k, 17776, 9216, 3072) for k in KERNELS] == ["t128x128", "p256", "p256"]
        assert bf16_path(1, 300, 264, 512) == "t128x128" and bf16_path(0, 300, 264, 512, "mxfp8", "mxfp8") == "t128x128"
        assert quant_path(0, 17776, 9216, 3072, "mxfp8", "mxfp8") == "t128x128"
    # the older entry points for mxfp8 x mxfp4: the tiled kernel, whatever the option says
    for o in KERNELS:
        with ops.options(mx_kernel=o):
            assert ops.gemm_mx_plan(**gemm_args(17776, 9216, 3072, "mxfp8", "mxfp4"))["path"] == "t128x128"
            assert ops.gemm_mx_plan(**gemm_args(300, 264, 512, "mxfp8", "mxfp4"))["path"] == "t128x128"
    assert ops.get_option("mx_kernel") == 0


def raw(lib, _hip, kernel, epi="bf16", a_fmt=E4M3, w_fmt=E2M1, out_fmt=E4M3, M=300, N=384, K=512, call=None, **over):
    """(code of the old entry point's plan query or None, code of the new query, code of the new launch, plan path) for one
    call given through the C ABI; `over`: pointer fields of the call, fields of the norm descriptor or of the GEMM descriptor."""
    d, n, c = _hip.GemmDesc(), _hip.QkNormDesc(), _hip.MxGemmCall()
    bytes_of = {E4M3: K, E2M3: K * 6 // 8, E2M1: K // 2}
    d.M, d.N, d.K, d.batch = M, N, K, 1
    d.lda, d.ldw, d.ldc, d.alpha = bytes_of[a_fmt], bytes_of[w_fmt], N, 1.0
    n.qw = n.qb = n.kw = n.kb = n.cos = n.sin = BASE
    n.text_rows, n.width, n.eps, n.k_scale = 40, N // 3, 1e-6, 0.18
    if epi == "qkn":
        d.ldc, d.n_split, d.c_split_stride = N // 3, N // 3, M * (N // 3)
    c.A = c.a_scales = c.W = c.w_scales = c.bias = c.C = BASE
    c.a_fmt, c.w_fmt, c.out_fmt, c.kernel = a_fmt, w_fmt, out_fmt, kernel
    if epi == "quant":
        c.q_scales = BASE
    if epi == "qkn":
        c.norm = ctypes.pointer(n)
    for k, v in (call or {}).items():
        setattr(c, k, v)
    for k, v in over.items():
        setattr(n if hasattr(n, k) and not hasattr(d, k) else d, k, v)
    p0, p1 = _hip.GemmPlan(-9, -9, -9, -9, -9), _hip.GemmPlan(-9, -9, -9, -9, -9)
    ops_ = (c.A, c.a_scales, c.W, c.w_scales, c.bias, c.C)
    if epi == "bf16":
        old = lib.bya_gemm_mx_mixed_plan(*ops_, c.res, c.gate0, c.gate1, ctypes.byref(d), a_fmt, w_fmt, ctypes.byref(p0))
    elif epi == "quant":
        old = lib.bya_gemm_mx_quant_plan(*ops_, c.q_scales, ctypes.byref(d), a_fmt, w_fmt, out_fmt, ctypes.byref(p0))
    else:
        old = lib.bya_gemm_mx_qkv_norm_rope_plan(*ops_, a_fmt, w_fmt, ctypes.byref(d), ctypes.byref(n), ctypes.byref(p0))
    new = lib.bya_gemm_mx_call_plan(ctypes.byref(c), ctypes.byref(d), ctypes.byref(p1))
    launch = lib.bya_gemm_mx_call(ctypes.byref(c), ctypes.byref(d), None) if new != OK else None
    return old, new, launch, p1.path


def test_errors_of_the_new_pair():
    lib, _hip = lib_and_hip()
    for epi in ("bf16", "quant", "qkn"):
        for bad in (3, -1):
            assert raw(lib, _hip, bad, epi)[1:] == (ERR_SHAPE, ERR_SHAPE, -9)
        assert raw(lib, _hip, 2, epi)[1::2] == (OK, 4) and raw(lib, _hip, 0, epi)[1::2] == (OK, 1)
    for k in KERNELS:
        # both epilogues; gates or a residual together with either
        n = _hip.QkNormDesc()
        assert raw(lib, _hip, k, "quant", call=dict(norm=ctypes.pointer(n)))[1:] == (ERR_SHAPE, ERR_SHAPE, -9)
        for extra in ("gate0", "gate1", "res"):
            assert raw(lib, _hip, k, "qkn", call={extra: BASE})[1:] == (ERR_SHAPE, ERR_SHAPE, -9)
            assert raw(lib, _hip, k, "quant", call={extra: BASE})[1:] == (ERR_SHAPE, ERR_SHAPE, -9)
        for epi in ("bf16", "quant", "qkn"):
            assert raw(lib, _hip, k, epi, w_fmt=E2M3)[:3] == (ERR_UNSUPPORTED,) * 3                   # e4m3 x e2m3
            assert raw(lib, _hip, k, epi, a_fmt=E2M1, w_fmt=E2M1)[:3] == (ERR_UNSUPPORTED,) * 3       # e2m1 activations
    d, c, p = _hip.GemmDesc(), _hip.MxGemmCall(), _hip.GemmPlan(-9, -9, -9, -9, -9)
    assert lib.bya_gemm_mx_call_plan(None, ctypes.byref(d), ctypes.byref(p)) == ERR_SHAPE
    assert lib.bya_gemm_mx_call_plan(ctypes.byref(c), None, ctypes.byref(p)) == ERR_SHAPE
    assert lib.bya_gemm_mx_call_plan(ctypes.byref(c), ctypes.byref(d), None) == ERR_SHAPE
    assert lib.bya_gemm_mx_call(None, ctypes.byref(d), None) == ERR_SHAPE and lib.bya_gemm_mx_call(ctypes.byref(c), None, None) == ERR_SHAPE
    assert p.path == -9


def test_bad_descriptors_get_the_old_entry_points_code_under_every_kernel():
    lib, _hip = lib_and_hip()
    table = [("bf16", dict(K=192), ERR_SHAPE), ("bf16", dict(ldw=128), ERR_SHAPE), ("bf16", dict(lda=520), ERR_ALIGN),
             ("bf16", dict(act=2), ERR_UNSUPPORTED), ("bf16", dict(n_split=6), ERR_SHAPE), ("bf16", dict(M=0), ERR_SHAPE),
             ("quant", dict(n_split=128), ERR_UNSUPPORTED), ("quant", dict(N=264), ERR_SHAPE), ("quant", dict(ldc=200), ERR_SHAPE),
             ("quant", dict(ldc=392), ERR_ALIGN), ("quant", dict(out_fmt=E2M1), ERR_UNSUPPORTED),
             ("qkn", dict(act=1), ERR_UNSUPPORTED), ("qkn", dict(n_split=0), ERR_UNSUPPORTED), ("qkn", dict(width=100), ERR_UNSUPPORTED),
             ("qkn", dict(ldc=132), ERR_ALIGN), ("qkn", dict(text_rows=-1), ERR_SHAPE), ("qkn", dict(cos=None), ERR_SHAPE)]
    for epi, over, want in table:
        for k in KERNELS:
            kw = dict(over)
            out_fmt = kw.pop("out_fmt", E4M3)
            old, new, launch, path = raw(lib, _hip, k, epi, out_fmt=out_fmt, **kw)
            assert old == want and (new, launch, path) == (want, want, -9), (epi, over, k, old, new, launch, path)
    for k in KERNELS:
        for epi in ("bf16", "quant", "qkn"):
            assert raw(lib, _hip, k, epi, call=dict(A=None))[:3] == (ERR_SHAPE,) * 3
            assert raw(lib, _hip, k, epi, call=dict(C=BASE + 4))[:3] == (ERR_ALIGN,) * 3
    # a bias the persistent kernel's 16-byte loads cannot take (legal for the tiled kernel): tiled, not refused
    assert raw(lib, _hip, 2, "bf16", call=dict(bias=BASE + 8))[1::2] == (OK, 1)


def test_model_switch_and_the_engines_kernel_value():
    from bind_your_avatar_implementation_amd import engine
    from bind_your_avatar_implementation_amd.transformer import BindyouravatarTransformer3DModel as Model
    fake = types.SimpleNamespace(invalidate_engine=lambda: None)
    for value in (True, "always"):
        Model.enable_mx_weights(fake, "mxfp8", weight_format="mxfp4", persistent_gemm=value)
        assert fake._mx_persistent_gemm == value and fake._mx_weight_format == "mxfp4"
    Model.enable_mx_weights(fake, "mxfp8", weight_format="mxfp4")
    assert getattr(fake, "_mx_persistent_gemm", False) is False
    pick = engine.mx_call_kernel
    assert [pick("mxfp8", "mxfp4", v) for v in (True, "always", False)] == [1, 2, 0]
    assert [pick("mxfp6", w, v) for w in ("mxfp6", "mxfp4") for v in (True, "always", False)] == [0] * 6
    assert [pick("mxfp8", "mxfp8", v) for v in (True, "always", False)] == [0] * 3       # same format: option mx_kernel, as ever


def test_generated_bodies_are_current_and_the_e2m1_body_has_14_pieces():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_gemm_mx_schedule.py"), "--check"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=os.path.join(ROOT, "tools"))
    assert r.returncode == 0, r.stdout.decode()
    src = open(os.path.join(ROOT, "bind_your_avatar_implementation_amd", "csrc", "gemm_mx_v4.hip")).read()
    body = src.split("// GENERATED-W4-BEGIN")[1].split("// GENERATED-W4-END")[0]
    pieces = [f"PIECE({q}, {w})" for w, n in (("false", 8), ("true", 4)) for q in range(n)] + ["SPIECE(false)", "SPIECE(true)"]
    assert body.count("PIECE(") == 14 and all(body.count(" " + p + ";") == 1 for p in pieces)
    assert body.count("MFX(") == 64 and "PIECE(4, true)" not in body
    # B2 counts the pieces requested in front of it
    head = body.split("B2(")[0]
    assert f"B2({head.count('PIECE(')})" in body
    assert "vmcnt(14)" in src
