"""CPU: what the GEMM front end of ops.py hands to the library -- entry point, pointers, descriptor bytes -- for every
``*_plan`` wrapper from ``gemm_plan`` to ``gemm_mx_call_plan``, against a recording taken before the wrappers were folded onto
shared helpers (tests/golden/ops_gemm_descriptors.json).  The library is replaced by a stub that records its arguments and
answers 0, so nothing is built and nothing launched; meta tensors stand for device tensors, and their "addresses" are
``ops._META_BASE`` + the view's offset, so the recording is the same in every process.

``python tests/test_ops_descriptors_cpu.py`` rewrites the recording from the ``ops`` module on the path.  It pins a refactor to
the code before it: regenerate it only when a descriptor is MEANT to change, from the commit that is meant to be matched."""
import ctypes
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_gemm_descriptors.json")
BITS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}
M, N, K, B, WIDTH = 300, 384, 256, 2, 128


def bf(*s):
    return torch.empty(*s, dtype=torch.bfloat16, device="meta")


def u8(*s):
    return torch.empty(*s, dtype=torch.uint8, device="meta")


def f32(*s):
    return torch.empty(*s, dtype=torch.float32, device="meta")


def _encode(arg):
    from bind_your_avatar_implementation_amd import _hip
    obj = getattr(arg, "_obj", None)                                     # ctypes.byref(struct)
    if obj is None:
        return arg                                                        # an address, a format code, a kernel number, None
    raw = bytearray(bytes(obj))
    if isinstance(obj, _hip.MxGemmCall):                                  # .norm is a HOST address: record what it points to
        f = _hip.MxGemmCall.norm
        raw[f.offset:f.offset + f.size] = bytes(f.size)
        return [raw.hex(), bytes(obj.norm.contents).hex() if obj.norm else None]
    return raw.hex()


class StubLibrary:
    """Stands for the loaded library: every entry point records (name, arguments) and answers 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append([name, [_encode(a) for a in args]])
            return 0
        entry.__name__ = name
        return entry


# ---- operands of one launch in each format: (positional arguments up to ``out``, the output's leading shape) ---------------
def bf16_ops(lead, n=N):
    return [bf(*lead, K), bf(n, K)]


def fp8_ops(lead, n=N):
    return [u8(*lead, K), f32(*lead), u8(n, K), f32(n)]


def mx_ops(lead, fmt, w_fmt=None, n=N):
    return [u8(*lead, K * BITS[fmt] // 8), u8(*lead, K // 32), u8(n, K * BITS[w_fmt or fmt] // 8), u8(n, K // 32)]


def epilogues(rowscale):
    """(name, leading shape, out, keyword arguments) of the bf16-output epilogue cases every format shares."""
    two, three = (M,), (B, M)
    yield "2d", two, bf(M, N), {}
    yield "3d_bias", three, bf(B, M, N), dict(bias=bf(N))
    yield "out_view", two, bf(M, 2 * N + 8)[:, 8:8 + N], {}
    yield "out_view_3d", three, bf(B, M, 2 * N)[:, :, N:], {}
    yield "res_2d", two, bf(M, N), dict(res=bf(M, N))
    yield "res_broadcast", three, bf(B, M, N), dict(res=bf(M, 2 * N)[:, N:])
    yield "res_3d", three, bf(B, M, N), dict(res=bf(B, M, N))
    yield "gate0", three, bf(B, M, N), dict(gate0=bf(B, N), gate_batch_stride=N)
    yield "gate01", three, bf(B, M, N), dict(gate0=bf(B, N), gate1=bf(B, N), gate_split=226, gate_batch_stride=6 * N, res=bf(B, M, N))
    yield "gelu", two, bf(M, N), dict(act="gelu_tanh", bias=bf(N))
    yield "split", three, bf(3, B, M, N // 3)[0], dict(split=(N // 3, B * M * (N // 3)))
    yield "alpha", two, bf(M, N), dict(alpha=0.5)
    if rowscale:
        yield "rowscale", three, bf(B, M, N), dict(bias=bf(N), bias_rowscale=f32(B * M))
        yield "rowscale_bad!", two, bf(M, N), dict(bias_rowscale=f32(M + 1))
    yield "res_shape!", two, bf(M, N), dict(res=bf(M, N + 64))
    yield "res_batch!", two, bf(M, N), dict(res=bf(B, M, N))
    yield "act_unknown!", two, bf(M, N), dict(act="swish")


def norm_cases():
    """(name, leading shape, tensors, the q/k-norm arguments after ``split`` as keywords) of the q/k-norm epilogue cases."""
    p = lambda: dict(qw=bf(64), qb=bf(64), kw=bf(64), kb=bf(64))
    yield "t3", (M,), 3, dict(**p(), cos=f32(M, 64), sin=f32(M, 64), text_rows=0)
    yield "t2_text", (M,), 2, dict(**p(), cos=f32(M - 44, 64), sin=f32(M - 44, 64), text_rows=44, eps=1e-5, k_scale=0.18)
    yield "no_rope_3d", (B, M), 3, dict(**p(), cos=None, sin=None, text_rows=M, k_scale=0.125)
    yield "t4!", (M,), 4, dict(**p(), cos=None, sin=None, text_rows=M)
    yield "cos_shape!", (M,), 3, dict(**p(), cos=f32(M, 64), sin=f32(M, 64), text_rows=44)


def qkn_out(lead, tensors):
    rows = M * (B if len(lead) == 2 else 1)
    return bf(tensors, *lead, WIDTH)[0], (WIDTH, rows * WIDTH)


def cases():
    """-> [(case id, name of the ops function, positional arguments, keyword arguments)]; an id ending in "!" is refused."""
    out = []
    add = lambda cid, fn, args, kw: out.append((cid, fn, args, kw))
    for name, lead, o, kw in epilogues(rowscale=True):
        add(f"bf16/{name}", "gemm_plan", [*bf16_ops(lead, 3 * (N // 3) if "split" in kw else N), o], kw)
    for name, lead, o, kw in epilogues(rowscale=False):
        add(f"fp8/{name}", "gemm_fp8_plan", [*fp8_ops(lead), o], kw)
    for fmt, w_fmt in (("mxfp6", None), ("mxfp8", None), ("mxfp8", "mxfp4"), ("mxfp6", "mxfp4")):
        for name, lead, o, kw in epilogues(rowscale=True):
            add(f"mx/{fmt}*{w_fmt}/{name}", "gemm_mx_plan", [*mx_ops(lead, fmt, w_fmt), o, fmt], dict(kw, w_fmt=w_fmt))
    add("mx/e2m1_activations!", "gemm_mx_plan", [*mx_ops((M,), "mxfp4"), bf(M, N), "mxfp4"], {})
    add("mx/w_fmt_mismatch!", "gemm_mx_plan", [*mx_ops((M,), "mxfp8", "mxfp6"), bf(M, N), "mxfp8"], dict(w_fmt="mxfp6"))

    # the quantising epilogue: MX codes out
    for fmt, w_fmt, out_fmt in (("mxfp6", None, None), ("mxfp8", None, None), ("mxfp8", "mxfp4", None), ("mxfp8", None, "mxfp6"),
                                ("mxfp6", "mxfp4", "mxfp8")):
        ob = BITS[out_fmt or fmt]
        for name, lead, kw in (("2d", (M,), {}), ("3d_gelu", (B, M), dict(bias=bf(N), act="gelu_tanh")), ("alpha", (M,), dict(alpha=0.25))):
            add(f"quant/{fmt}*{w_fmt}>{out_fmt}/{name}", "gemm_mx_quant_plan",
                [*mx_ops(lead, fmt, w_fmt), u8(*lead, N * ob // 8), u8(*lead, N // 32), fmt, w_fmt, out_fmt], kw)
    add("quant/out_size!", "gemm_mx_quant_plan", [*mx_ops((M,), "mxfp8"), u8(M, N - 32), u8(M, N // 32), "mxfp8"], {})
    add("quant/out_fmt_e2m1!", "gemm_mx_quant_plan", [*mx_ops((M,), "mxfp8"), u8(M, N // 2), u8(M, N // 32), "mxfp8", None, "mxfp4"], {})

    # the q/k-norm + RoPE epilogue in the three operand formats
    for name, lead, tensors, nk in norm_cases():
        o, split = qkn_out(lead, tensors)
        n = tensors * WIDTH
        add(f"qkn_bf16/{name}", "gemm_qkv_norm_rope_plan", [*bf16_ops(lead, n), o, bf(n), split], dict(nk, tensors=tensors))
        add(f"qkn_fp8/{name}", "gemm_fp8_qkv_norm_rope_plan", [*fp8_ops(lead, n), o, bf(n), split], dict(nk, tensors=tensors))
        for fmt, w_fmt, kernel in (("mxfp6", None, 0), ("mxfp8", "mxfp4", 0), ("mxfp8", None, 1), ("mxfp8", None, 2)):
            add(f"qkn_mx/{fmt}*{w_fmt}/k{kernel}/{name}", "gemm_mx_qkv_norm_rope_plan", [*mx_ops(lead, fmt, w_fmt, n), o, None, split],
                dict(nk, tensors=tensors, fmt=fmt, w_fmt=w_fmt, kernel=kernel))
    _, _, _, nk = next(norm_cases())
    o, split = qkn_out((M,), 3)
    n = 3 * WIDTH
    add("qkn_bf16/split_none!", "gemm_qkv_norm_rope_plan", [*bf16_ops((M,), n), o, None, None], nk)
    add("qkn_bf16/w_rows!", "gemm_qkv_norm_rope_plan", [*bf16_ops((M,), n + 1), o, None, split], nk)
    add("qkn_bf16/rows!", "gemm_qkv_norm_rope_plan", [*bf16_ops((M + 1,), n), o, None, split], nk)
    add("qkn_fp8/split_none!", "gemm_fp8_qkv_norm_rope_plan", [*fp8_ops((M,), n), o, None, None], nk)
    add("qkn_mx/split_none!", "gemm_mx_qkv_norm_rope_plan", [*mx_ops((M,), "mxfp6", None, n), o, None, None], nk)
    # descriptor fields the launches never set: the plan queries pass them on (fp8: the residual's leading dimension)
    add("qkn_fp8/res", "gemm_fp8_qkv_norm_rope_plan", [*fp8_ops((M,), n), o, None, split], dict(nk, res=bf(M, 2 * n)[:, n:]))
    add("qkn_fp8/res_3d", "gemm_fp8_qkv_norm_rope_plan", [*fp8_ops((B, M), n), qkn_out((B, M), 3)[0], None, qkn_out((B, M), 3)[1]],
        dict(nk, cos=None, sin=None, res=bf(B, M, n)))
    add("qkn_fp8/act_alpha", "gemm_fp8_qkv_norm_rope_plan", [*fp8_ops((M,), n), o, None, split], dict(nk, act="gelu_tanh", alpha=0.5))
    add("qkn_mx/act_alpha", "gemm_mx_qkv_norm_rope_plan", [*mx_ops((M,), "mxfp6", None, n), o, None, split],
        dict(nk, act="gelu_tanh", alpha=0.5))

    # one call, the kernel an argument: every epilogue on kernels 0, 1 and 17
    for kernel, fmt, w_fmt in ((0, "mxfp8", None), (0, "mxfp6", "mxfp4"), (1, "mxfp8", None), (1, "mxfp8", "mxfp4"), (17, "mxfp6", None)):
        tag = f"call/k{kernel}/{fmt}*{w_fmt}"
        for name, lead, o, kw in epilogues(rowscale=True):
            add(f"{tag}/{name}", "gemm_mx_call_plan", [*mx_ops(lead, fmt, w_fmt), o, kernel, fmt, w_fmt], kw)
        for name, lead, kw in (("2d", (M,), {}), ("3d_gelu", (B, M), dict(bias=bf(N), act="gelu_tanh", alpha=0.25, out_fmt=fmt))):
            add(f"{tag}/quant_{name}", "gemm_mx_call_plan", [*mx_ops(lead, fmt, w_fmt), u8(*lead, N * BITS[fmt] // 8), kernel, fmt, w_fmt],
                dict(kw, out_scales=u8(*lead, N // 32)))
        for name, lead, tensors, nk in norm_cases():
            o, split = qkn_out(lead, tensors)
            n = tensors * WIDTH
            nk = {k: v for k, v in nk.items() if v is not None}
            add(f"{tag}/norm_{name}", "gemm_mx_call_plan", [*mx_ops(lead, fmt, w_fmt, n), o, kernel, fmt, w_fmt],
                dict(bias=bf(n), split=split, norm=dict(nk, tensors=tensors)))
        nk = dict(next(norm_cases())[3])
        o, split = qkn_out((M,), 3)
        n = 3 * WIDTH
        add(f"{tag}/norm_defaults", "gemm_mx_call_plan", [*mx_ops((M,), fmt, w_fmt, n), o, kernel, fmt, w_fmt], dict(split=split, norm=nk))
        add(f"{tag}/norm_act_alpha", "gemm_mx_call_plan", [*mx_ops((M,), fmt, w_fmt, n), o, kernel, fmt, w_fmt],
            dict(split=split, norm=nk, act="gelu_tanh", alpha=0.5))
        add(f"{tag}/both", "gemm_mx_call_plan", [*mx_ops((M,), fmt, w_fmt, n), o, kernel, fmt, w_fmt],
            dict(split=split, norm=nk, out_scales=u8(M, n // 32), res=bf(M, n), act="gelu_tanh"))
        add(f"{tag}/norm_split_none!", "gemm_mx_call_plan", [*mx_ops((M,), fmt, w_fmt, n), o, kernel, fmt, w_fmt], dict(norm=nk))
        add(f"{tag}/norm_rowscale!", "gemm_mx_call_plan", [*mx_ops((M,), fmt, w_fmt, n), o, kernel, fmt, w_fmt],
            dict(split=split, norm=nk, bias_rowscale=f32(M)))
        add(f"{tag}/quant_rowscale!", "gemm_mx_call_plan", [*mx_ops((M,), fmt, w_fmt), u8(M, N * BITS[fmt] // 8), kernel, fmt, w_fmt],
            dict(out_scales=u8(M, N // 32), bias_rowscale=f32(M)))
        add(f"{tag}/quant_out_size!", "gemm_mx_call_plan", [*mx_ops((M,), fmt, w_fmt), u8(M, N), kernel, fmt, w_fmt],
            dict(out_scales=u8(M, N // 32 - 1)))
    assert len({c[0] for c in out}) == len(out)
    return out


def record(monkeypatch_setattr):
    """Run the table against the stub -> {case id: {"calls": [[entry point, arguments]], "raises": type name or None}}."""
    from bind_your_avatar_implementation_amd import _hip, ops
    seen = {}
    for cid, fn, args, kw in cases():
        stub = StubLibrary()
        monkeypatch_setattr(_hip, "load", lambda stub=stub: stub)
        raised = None
        try:
            getattr(ops, fn)(*args, **kw)
        except Exception as e:                                           # (the type is what is pinned)
            raised = type(e).__name__
        seen[cid] = {"calls": stub.calls, "raises": raised}
    return seen


@pytest.fixture(scope="module")
def recorded():
    with pytest.MonkeyPatch.context() as mp:
        return record(mp.setattr)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(recorded, golden):
    assert sorted(recorded) == sorted(golden)


def test_refused_cases_raise_before_the_library_is_asked(recorded):
    for cid, got in recorded.items():
        if cid.endswith("!"):
            assert got["raises"] in ("ValueError", "TypeError", "AssertionError", "KeyError"), (cid, got["raises"])
            assert got["calls"] == [], cid
        else:
            assert got["raises"] is None and len(got["calls"]) == 1, (cid, got["raises"])


@pytest.mark.parametrize("group", ["bf16", "fp8", "mx", "quant", "qkn_bf16", "qkn_fp8", "qkn_mx", "call"])
def test_entry_point_arguments_and_descriptor_bytes(recorded, golden, group):
    ids = [c for c in golden if c.split("/")[0] == group]
    assert ids
    for cid in ids:
        assert json.loads(json.dumps(recorded[cid])) == golden[cid], cid


def test_the_recording_covers_what_it_should(golden):
    entries = {c["calls"][0][0] for c in golden.values() if c["calls"]}
    assert entries == {"bya_gemm_bf16_plan", "bya_gemm_fp8_plan", "bya_gemm_mx_plan", "bya_gemm_mx_mixed_plan", "bya_gemm_mx_quant_plan",
                       "bya_gemm_qkv_norm_rope_plan", "bya_gemm_fp8_qkv_norm_rope_plan", "bya_gemm_mx_qkv_norm_rope_plan",
                       "bya_gemm_mx_qkv_norm_rope_on_plan", "bya_gemm_mx_call_plan"}
    raises = {cid: c["raises"] for cid, c in golden.items() if c["raises"]}
    assert all(cid.endswith("!") for cid in raises)
    for fmt in ("bf16", "fp8", "mx/mxfp6*None", "call/k0/mxfp8*None", "call/k17/mxfp6*None"):
        assert raises[f"{fmt}/res_shape!"] == "ValueError"
    for q in ("qkn_bf16", "qkn_fp8", "qkn_mx/mxfp6*None/k0", "call/k1/mxfp8*None/norm"):
        assert raises[q + ("_t4!" if q.startswith("call") else "/t4!")] == "ValueError"
    assert raises["qkn_bf16/split_none!"] == "TypeError"                 # (the bf16 form unpacks it; the others ask first)
    assert raises["qkn_fp8/split_none!"] == raises["qkn_mx/split_none!"] == raises["call/k0/mxfp8*None/norm_split_none!"] == "ValueError"
    assert raises["call/k1/mxfp8*None/norm_rowscale!"] == "ValueError"


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    table = record(setattr)
    with open(GOLDEN, "w") as f:                                         # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(table[cid])}" for cid in sorted(table)) + "\n}\n")
    print(f"{len(table)} cases -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
