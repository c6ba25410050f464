"""CPU: the flag bit BYA_MX_KERNEL_FP6 (16) of bya_mx_gemm_call::kernel (include/bya.h; ops.gemm_mx_call, ops.gemm_mx_call_plan) --
the one way mxfp6 (e2m3) activations, with mxfp6 or mxfp4 weights, and mxfp6 output of the quantising epilogue reach the persistent
256 x 256 kernel of csrc/gemm_mx_v4.hip.  Which kernel a call takes is asked through the plan query on meta tensors (every check
runs before any launch, so without a GPU); without the bit nothing changes (tests/test_mx_p256_w4_cpu.py pins that);
tests/test_mx_p256_fp6_gpu.py checks the bits."""
import ctypes
import os
import subprocess
import sys
import types

import pytest

import test_mx_p256_w4_cpu as w4
from test_mx_p256_w4_cpu import bf16_path, qkn_path, quant_path, raw
from test_mx_qkn_cpu import BASE, E2M1, E2M3, E4M3, ERR_SHAPE, ERR_UNSUPPORTED, OK, lib_and_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP6_KERNELS = (16, 17, 18)
PAIRS = (("mxfp6", "mxfp6"), ("mxfp6", "mxfp4"))
P256, T128, T256 = 4, 1, 3


def test_the_flag_is_declared_and_the_struct_keeps_its_size():
    lib, _hip = lib_and_hip()
    header = open(os.path.join(ROOT, "include", "bya.h")).read()
    assert "#define BYA_MX_KERNEL_FP6 16" in header and _hip.MX_KERNEL_FP6 == 16
    assert ctypes.sizeof(_hip.MxGemmCall) == 11 * 8 + 4 * 4


@pytest.mark.parametrize("fmt,w_fmt", PAIRS)
def test_mxfp6_activations_reach_the_persistent_kernel_under_every_epilogue(fmt, w_fmt):
    lib_and_hip()
    big = (17776, 9216, 3072)
    assert [bf16_path(k, *big, fmt, w_fmt) for k in FP6_KERNELS] == ["t256x256", "p256", "p256"]
    assert [quant_path(k, *big, fmt, w_fmt, "mxfp6") for k in FP6_KERNELS] == ["t256x256", "p256", "p256"]
    assert [quant_path(k, *big, fmt, w_fmt, "mxfp8") for k in FP6_KERNELS] == ["t256x256", "p256", "p256"]
    assert [qkn_path(k, 17776, 3072, 3072, fmt, w_fmt, text=226) for k in FP6_KERNELS] == ["t256x256", "p256", "p256"]


@pytest.mark.parametrize("fmt,w_fmt", PAIRS)
def test_tile_count_k_tiles_and_alignment(fmt, w_fmt):
    lib_and_hip()
    assert [bf16_path(k, 300, 264, 512, fmt, w_fmt) for k in FP6_KERNELS] == ["t128x128", "t128x128", "p256"]    # 2 x 2 tiles
    assert bf16_path(18, 300, 264, 256, fmt, w_fmt) == "t128x128" and bf16_path(18, 300, 264, 384, fmt, w_fmt) == "t128x128"
    assert bf16_path(18, 300, 260, 512, fmt, w_fmt) == "t128x128"                                                # N % 8 != 0
    assert bf16_path(17, 1811, 3848, 640, fmt, w_fmt) == "t128x128"                                              # 128 tiles
    assert bf16_path(17, 1811, 3848, 640, fmt, w_fmt, batch=2) == "p256"                                         # the batch counts
    assert [quant_path(k, 300, 256, 512, fmt, w_fmt, "mxfp6") for k in FP6_KERNELS] == ["t128x128", "t128x128", "p256"]
    assert [qkn_path(k, 300, 192, 512, fmt, w_fmt, text=40) for k in FP6_KERNELS] == ["t128x128", "t128x128", "p256"]


def test_mxfp8_operands_with_mxfp6_output_and_mxfp8_launches_under_the_flag():
    from bind_your_avatar_implementation_amd import ops
    from test_mx_p256_cpu import gemm_args
    lib_and_hip()
    for w_fmt in ("mxfp8", "mxfp4"):
        assert quant_path(17, 17776, 12288, 3072, "mxfp8", w_fmt, "mxfp6") == "p256"
        assert quant_path(1, 17776, 12288, 3072, "mxfp8", w_fmt, "mxfp6") == "t128x128"
        assert quant_path(18, 300, 256, 512, "mxfp8", w_fmt, "mxfp6") == "p256"
        assert quant_path(16, 17776, 12288, 3072, "mxfp8", w_fmt, "mxfp6") == "t128x128"
    # mxfp8 launches: 17 / 18 answer what 1 / 2 answer, 16 what 0 answers
    for shape in ((17776, 9216, 3072), (300, 264, 512), (300, 264, 256), (300, 260, 512), (1811, 3848, 640)):
        for w_fmt in ("mxfp8", "mxfp4"):
            for k in (0, 1, 2):
                assert bf16_path(16 + k, *shape, "mxfp8", w_fmt) == bf16_path(k, *shape, "mxfp8", w_fmt), (shape, w_fmt, k)
        for k in (0, 1, 2):
            a = gemm_args(*shape, "mxfp8")
            got = ops.gemm_mx_call_plan(a.pop("a_codes"), a.pop("a_scales"), a.pop("w_codes"), a.pop("w_scales"), a.pop("out"), 16 + k, **a)
            with ops.options(mx_kernel=k):
                assert got == ops.gemm_mx_plan(**gemm_args(*shape, "mxfp8")), (shape, k)
    for k in (0, 1, 2):
        assert quant_path(16 + k, 17776, 9216, 3072) == quant_path(k, 17776, 9216, 3072)
        assert qkn_path(16 + k, 17776, 3072, 3072, text=226) == qkn_path(k, 17776, 3072, 3072, text=226)


def test_without_the_flag_mxfp6_stays_tiled_and_no_option_has_a_say():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()
    for o in (0, 2):
        with ops.options(mx_kernel=o):
            for fmt, w_fmt in PAIRS:
                assert [bf16_path(k, 17776, 9216, 3072, fmt, w_fmt) for k in (0, 1, 2)] == ["t256x256"] * 3
                assert [bf16_path(k, 17776, 9216, 3072, fmt, w_fmt) for k in FP6_KERNELS] == ["t256x256", "p256", "p256"]
    assert ops.get_option("mx_kernel") == 0


def test_errors_of_the_kernel_field():
    lib, _hip = lib_and_hip()
    for epi in ("bf16", "quant", "qkn"):
        for a_fmt, w_fmt in ((E2M3, E2M3), (E2M3, E2M1), (E4M3, E2M1)):
            for bad in (3, 19, 32, -1, 4, 20, 33, -16):
                assert raw(lib, _hip, bad, epi, a_fmt, w_fmt)[1:] == (ERR_SHAPE, ERR_SHAPE, -9), (epi, a_fmt, w_fmt, bad)
        for a_fmt, w_fmt in ((E2M3, E2M3), (E2M3, E2M1)):
            assert raw(lib, _hip, 18, epi, a_fmt, w_fmt)[1::2] == (OK, P256) and raw(lib, _hip, 16, epi, a_fmt, w_fmt)[1::2] == (OK, T128)
            assert raw(lib, _hip, 2, epi, a_fmt, w_fmt)[1::2] == (OK, T128)
        assert raw(lib, _hip, 18, "quant", out_fmt=E2M3)[1::2] == (OK, P256) and raw(lib, _hip, 2, "quant", out_fmt=E2M3)[1::2] == (OK, T128)
    for k in (0, 1, 2) + FP6_KERNELS:
        for epi in ("bf16", "quant", "qkn"):
            assert raw(lib, _hip, k, epi, a_fmt=E4M3, w_fmt=E2M3)[:3] == (ERR_UNSUPPORTED,) * 3                 # e4m3 x e2m3
            assert raw(lib, _hip, k, epi, a_fmt=E2M1, w_fmt=E2M1)[:3] == (ERR_UNSUPPORTED,) * 3                 # e2m1 activations
            assert raw(lib, _hip, k, epi, a_fmt=E2M3, w_fmt=E4M3)[:3] == (ERR_UNSUPPORTED,) * 3                 # e2m3 x e4m3


def test_bad_descriptors_get_the_old_entry_points_code_under_the_flag(monkeypatch):
    """The table of tests/test_mx_p256_w4_cpu.py, run under kernels 16 / 17 / 18; then a few of its rows on e2m3 operands."""
    monkeypatch.setattr(w4, "KERNELS", FP6_KERNELS)
    w4.test_bad_descriptors_get_the_old_entry_points_code_under_every_kernel()
    lib, _hip = lib_and_hip()
    ERR_ALIGN = w4.ERR_ALIGN
    table = [("bf16", dict(K=192), ERR_SHAPE), ("bf16", dict(lda=256), ERR_SHAPE), ("bf16", dict(lda=392), ERR_ALIGN),
             ("bf16", dict(act=2), ERR_UNSUPPORTED), ("quant", dict(N=264), ERR_SHAPE), ("quant", dict(ldc=392), ERR_ALIGN),
             ("qkn", dict(width=100), ERR_UNSUPPORTED), ("qkn", dict(text_rows=-1), ERR_SHAPE)]
    for epi, over, want in table:
        for k in FP6_KERNELS:
            for w_fmt in (E2M3, E2M1):
                old, new, launch, path = raw(lib, _hip, k, epi, E2M3, w_fmt, E2M3, **over)
                assert old == want and (new, launch, path) == (want, want, -9), (epi, over, k, w_fmt, old, new, launch, path)
    # a bias the persistent kernel's 16-byte loads cannot take (legal for the tiled kernel): tiled, not refused
    assert raw(lib, _hip, 18, "bf16", E2M3, E2M3, call=dict(bias=BASE + 8))[1::2] == (OK, T128)


def test_model_switch_and_the_engines_kernel_value():
    from bind_your_avatar_implementation_amd import engine
    from bind_your_avatar_implementation_amd.transformer import BindyouravatarTransformer3DModel as Model
    fake = types.SimpleNamespace(invalidate_engine=lambda: None)
    for value in (True, "always"):
        Model.enable_mx_weights(fake, "mxfp6", persistent_gemm_mxfp6=value)
        assert fake._mx_persistent_gemm_mxfp6 == value and not hasattr(fake, "_mx_persistent_gemm")
    Model.enable_mx_weights(fake, "mxfp6")
    assert not hasattr(fake, "_mx_persistent_gemm_mxfp6")
    Model.enable_mx_weights(fake, "mxfp6", enabled=False, persistent_gemm_mxfp6=True)
    assert not hasattr(fake, "_mx_persistent_gemm_mxfp6")
    for bad in ("yes", 2, None, "Always"):
        with pytest.raises(ValueError, match="persistent_gemm_mxfp6"):
            Model.enable_mx_weights(fake, "mxfp6", persistent_gemm_mxfp6=bad)
    with pytest.raises(TypeError):
        Model.enable_mx_weights(fake, "mxfp6", None, None, None, True)                     # keyword only
    pick = engine.mx_call_kernel
    for w in ("mxfp6", "mxfp4"):
        assert [pick("mxfp6", w, pg, v) for pg in (False, True, "always") for v in (True, "always", False)] == [17, 18, 0] * 3
    # mxfp8 activations: the new switch does nothing
    assert [pick("mxfp8", "mxfp4", pg, v) for pg in (True, "always", False) for v in (True, "always")] == [1, 1, 2, 2, 0, 0]
    assert [pick("mxfp8", "mxfp8", pg, v) for pg in (True, "always", False) for v in (True, "always")] == [0] * 6
    # the old calls, fourth argument omitted
    assert [pick("mxfp8", "mxfp4", v) for v in (True, "always", False)] == [1, 2, 0]
    assert [pick("mxfp6", w, v) for w in ("mxfp6", "mxfp4") for v in (True, "always", False)] == [0] * 6
    assert [pick("mxfp8", "mxfp8", v) for v in (True, "always", False)] == [0] * 3


def test_generated_bodies_are_current_and_count_their_pieces():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_gemm_mx_schedule.py"), "--check"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=os.path.join(ROOT, "tools"))
    assert r.returncode == 0, r.stdout.decode()
    src = open(os.path.join(ROOT, "bind_your_avatar_implementation_amd", "csrc", "gemm_mx_v4.hip")).read()
    for tag, n_w in (("A6", 6), ("A6W4", 4)):
        body = src.split(f"// GENERATED-{tag}-BEGIN")[1].split(f"// GENERATED-{tag}-END")[0]
        pieces = [f"PIECE({q}, {w})" for w, n in (("false", 6), ("true", n_w)) for q in range(n)] + ["SPIECE(false)", "SPIECE(true)"]
        assert len(pieces) == 8 + n_w and body.count("PIECE(") == 8 + n_w and all(body.count(" " + p + ";") == 1 for p in pieces)
        assert body.count("MFX(") == 64 and "PIECE(6, false)" not in body and f"PIECE({n_w}, true)" not in body
        assert body.count("B1();") == 1 and body.count("B2(") == 1 and body.count("REREAD_W();") == 1 and body.count("REREAD_A(") == 8
        # B2 counts the pieces requested in front of it; B1 stands in front of every piece
        head = body.split("B2(")[0]
        assert f"B2({head.count('PIECE(')})" in body and "PIECE(" not in body.split("B1();")[0]
        # the prologue and tile-end waits come from the generator's table
        assert f"MX_PIECES_{tag} = {8 + n_w}" in src.split("// GENERATED-PIECES-BEGIN")[1].split("// GENERATED-PIECES-END")[0]
    assert '"s_waitcnt vmcnt(%0)" TAIL :: "n"(W4 ? MX_PIECES_A6W4 : MX_PIECES_A6)' in src
