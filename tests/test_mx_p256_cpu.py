"""Option mx_kernel (BYA_OPT_MX_KERNEL) and what the MX plan queries answer under it -- no GPU needed: the queries launch
nothing.  0 keeps every MX GEMM on the tiled kernels of csrc/gemm_mx.hip; 1 sends e4m3 x e4m3 launches of at least 200
256 x 256 tiles that are eligible to the persistent kernel of csrc/gemm_mx_v4.hip ("p256"); 2 drops the tile count."""
import os
import re
import subprocess
import sys
import types

import pytest
import torch

from test_mx_qkn_cpu import meta_args as qkn_meta_args

BITS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_and_hip():
    from bind_your_avatar_implementation_amd import _hip
    return _hip.load(), _hip


def test_option_key_matches_the_header_and_refuses_other_values():
    lib, _hip = lib_and_hip()
    src = open(os.path.join(ROOT, "include", "bya.h")).read()
    keys = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"BYA_OPT_(\w+) = (\d+)", src))
    count = keys.pop("count")
    assert keys == _hip.OPTIONS and count == len(keys) == 9 and keys["mx_kernel"] == 8
    assert _hip.OPTION_DEFAULTS["mx_kernel"] == 0 and _hip.get_option("mx_kernel") == 0
    for bad in (3, -1):
        assert lib.bya_set_option(_hip.OPTIONS["mx_kernel"], bad) == -1 and _hip.get_option("mx_kernel") == 0
    for ok in (1, 2, 0):
        assert lib.bya_set_option(_hip.OPTIONS["mx_kernel"], ok) == 0 and _hip.get_option("mx_kernel") == ok


def u8(*s):
    return torch.empty(*s, dtype=torch.uint8, device="meta")


def gemm_args(M, N, K, fmt, w_fmt=None, batch=1):
    lead = (batch, M) if batch > 1 else (M,)
    return dict(a_codes=u8(*lead, K * BITS[fmt] // 8), a_scales=u8(*lead, K // 32), w_codes=u8(N, K * BITS[w_fmt or fmt] // 8),
                w_scales=u8(N, K // 32), out=torch.empty(*lead, N, dtype=torch.bfloat16, device="meta"), fmt=fmt, w_fmt=w_fmt,
                bias=torch.empty(N, dtype=torch.bfloat16, device="meta"))


def quant_args(M, N, K, fmt, out_fmt):
    a = gemm_args(M, N, K, fmt)
    del a["out"]
    return dict(a, out_codes=u8(M, N * BITS[out_fmt] // 8), out_scales=u8(M, N // 32), out_fmt=out_fmt, act="gelu_tanh")


def test_plan_queries_follow_the_option():
    from bind_your_avatar_implementation_amd import ops
    lib_and_hip()

    def path(opt, **kw):
        with ops.options(mx_kernel=opt):
            return ops.gemm_mx_plan(**kw)["path"]

    def qpath(opt, **kw):
        with ops.options(mx_kernel=opt):
            return ops.gemm_mx_quant_plan(**kw)["path"]

    big = gemm_args(17776, 9216, 3072, "mxfp8")
    assert [path(o, **big) for o in (0, 1, 2)] == ["t128x128", "p256", "p256"]
    assert [path(o, **gemm_args(17776, 9216, 3072, "mxfp6")) for o in (0, 1, 2)] == ["t256x256"] * 3
    assert [path(o, **gemm_args(17776, 9216, 3072, "mxfp8", "mxfp4")) for o in (0, 1, 2)] == ["t128x128"] * 3
    small = gemm_args(300, 264, 512, "mxfp8")
    assert [path(o, **small) for o in (0, 1, 2)] == ["t128x128", "t128x128", "p256"]
    assert path(2, **gemm_args(300, 264, 256, "mxfp8")) == "t128x128"                     # fewer than four K-tiles
    assert path(2, **gemm_args(300, 260, 512, "mxfp8")) == "t128x128"                     # N % 8 != 0
    assert path(1, **gemm_args(1811, 3848, 640, "mxfp8", batch=2)) == "p256"              # the batch counts: 2 x 8 x 16 tiles
    assert path(1, **gemm_args(1811, 3848, 640, "mxfp8")) == "t128x128"
    # the quantising epilogue: out e4m3 follows, out e2m3 stays on the tiled kernel
    assert [qpath(o, **quant_args(17776, 12288, 3072, "mxfp8", "mxfp8")) for o in (0, 1, 2)] == ["t128x128", "p256", "p256"]
    assert [qpath(o, **quant_args(17776, 12288, 3072, "mxfp8", "mxfp6")) for o in (0, 1, 2)] == ["t128x128"] * 3
    assert [qpath(o, **quant_args(300, 256, 512, "mxfp8", "mxfp8")) for o in (0, 1, 2)] == ["t128x128", "t128x128", "p256"]
    assert [qpath(o, **quant_args(17776, 12288, 3072, "mxfp6", "mxfp6")) for o in (0, 1, 2)] == ["t256x256"] * 3
    # the q/k-norm epilogue answers as ever
    for fmt, want in (("mxfp8", "t128x128"), ("mxfp6", "t256x256")):
        for o in (0, 1, 2):
            with ops.options(mx_kernel=o):
                assert ops.gemm_mx_qkv_norm_rope_plan(**qkn_meta_args(17776, 3072, 3072, fmt))["path"] == want
    assert ops.get_option("mx_kernel") == 0


def test_model_switch_validates_its_value():
    from bind_your_avatar_implementation_amd.transformer import BindyouravatarTransformer3DModel as Model
    fake = types.SimpleNamespace(invalidate_engine=lambda: None)
    Model.enable_mx_weights(fake, "mxfp8")
    assert getattr(fake, "_mx_persistent_gemm", False) is False
    Model.enable_mx_weights(fake, "mxfp8", persistent_gemm=True)
    assert fake._mx_persistent_gemm is True
    Model.enable_mx_weights(fake, "mxfp8", persistent_gemm="always")
    assert fake._mx_persistent_gemm == "always"
    with pytest.raises(ValueError):
        Model.enable_mx_weights(fake, "mxfp8", persistent_gemm="yes")
    assert fake._mx_persistent_gemm == "always"                                           # a refused call changes nothing
    Model.enable_mx_weights(fake, "mxfp8")                                                # off again
    assert getattr(fake, "_mx_persistent_gemm", False) is False
    with pytest.raises(TypeError):
        Model.enable_mx_weights(fake, "mxfp8", None, None, None, True, False, False, True)   # keyword only


def test_environment_variable_takes_names_and_numbers_and_refuses_the_rest():
    from bind_your_avatar_implementation_amd import _hip
    name, parse = _hip.ENV_OPTIONS["BYA_MX_KERNEL"]
    assert name == "mx_kernel"
    assert [parse(v) for v in ("0", "1", "p256", "2", "always")] == [0, 1, 1, 2, 2]
    for bad in ("yes", "3", "P256"):
        with pytest.raises(ValueError):
            parse(bad)


def test_generated_ktile_body_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_gemm_mx_schedule.py"), "--check"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=os.path.join(ROOT, "tools"))
    assert r.returncode == 0, r.stdout.decode()
