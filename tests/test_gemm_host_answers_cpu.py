"""CPU: what the GEMM host code answers -- the return code and the five plan fields of every ``*_plan`` query of the GEMM
family, and the return code of the launch entry point where the query refuses -- against a recording taken from the library
BEFORE its argument functions, row split and launch / plan bodies were folded onto shared helpers
(tests/golden/gemm_host_answers.json).  The real library answers: it loads without a GPU, the pointers are made-up addresses
(``1 << 40`` plus offsets) that nothing on these paths dereferences, and every case is ONE mutation of a valid base per entry
point -- a pointer null or misaligned, a dimension or leading dimension off, an activation, a split, a format, a kernel value,
a norm descriptor field -- or a shape / option state that moves the path rules.

A launch entry point is called only where the recorded plan query (asked with a plan to fill) refused the same arguments, so
it returns before anything is launched; ``bya_gemm_skinny_bf16``, which has no query, only with arguments its own rules refuse.

``BYA_HIP_LIB=<the library to be matched> python tests/test_gemm_host_answers_cpu.py`` rewrites the recording.  It pins a
refactor to the code before it: regenerate it only when an answer is MEANT to change, from the commit that is meant to be
matched -- never from the code under test."""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_host_answers.json")
SENTINEL = -9
E4M3, E2M3, E2M1 = 0, 2, 4
M, N, K, WIDTH = 300, 384, 512, 128

POINTERS = ("A", "a_scale", "W", "w_scale", "bias", "C", "res", "gate0", "gate1", "q_scales", "bias_rowscale",
            "qw", "qb", "kw", "kb", "cos", "sin")
ADDR = {name: (1 << 40) + (i << 33) for i, name in enumerate(POINTERS)}
NORM_PTRS = ("qw", "qb", "kw", "kb", "cos", "sin")

# entry -> (plan query, launch entry point, its pointer arguments, the epilogue its base describes)
ENTRIES = {
    "bf16": ("bya_gemm_bf16_plan", "bya_gemm_bf16", ("A", "W", "bias", "C", "res", "gate0", "gate1"), "plain"),
    "skinny": (None, "bya_gemm_skinny_bf16", ("A", "W", "bias", "C", "res"), "plain"),
    "qkn_bf16": ("bya_gemm_qkv_norm_rope_plan", "bya_gemm_qkv_norm_rope", ("A", "W", "bias", "C"), "norm"),
    "fp8": ("bya_gemm_fp8_plan", "bya_gemm_fp8", ("A", "a_scale", "W", "w_scale", "bias", "C", "res", "gate0", "gate1"), "plain"),
    "qkn_fp8": ("bya_gemm_fp8_qkv_norm_rope_plan", "bya_gemm_fp8_qkv_norm_rope", ("A", "a_scale", "W", "w_scale", "bias", "C"), "norm"),
    "mx": ("bya_gemm_mx_plan", "bya_gemm_mx", ("A", "a_scale", "W", "w_scale", "bias", "C", "res", "gate0", "gate1"), "plain"),
    "mx_mixed": ("bya_gemm_mx_mixed_plan", "bya_gemm_mx_mixed", ("A", "a_scale", "W", "w_scale", "bias", "C", "res", "gate0", "gate1"),
                 "plain"),
    "mx_quant": ("bya_gemm_mx_quant_plan", "bya_gemm_mx_quant", ("A", "a_scale", "W", "w_scale", "bias", "C", "q_scales"), "quant"),
    "qkn_mx": ("bya_gemm_mx_qkv_norm_rope_plan", "bya_gemm_mx_qkv_norm_rope", ("A", "a_scale", "W", "w_scale", "bias", "C"), "norm"),
    "qkn_mx_on": ("bya_gemm_mx_qkv_norm_rope_on_plan", "bya_gemm_mx_qkv_norm_rope_on", ("A", "a_scale", "W", "w_scale", "bias", "C"),
                  "norm"),
    "call": ("bya_gemm_mx_call_plan", "bya_gemm_mx_call", ("A", "a_scale", "W", "w_scale", "bias", "C", "res", "gate0", "gate1"), "plain"),
    "call_quant": ("bya_gemm_mx_call_plan", "bya_gemm_mx_call", ("A", "a_scale", "W", "w_scale", "bias", "C", "q_scales"), "quant"),
    "call_norm": ("bya_gemm_mx_call_plan", "bya_gemm_mx_call", ("A", "a_scale", "W", "w_scale", "bias", "C"), "norm"),
}
MX_ENTRIES = ("mx", "mx_mixed", "mx_quant", "qkn_mx", "qkn_mx_on", "call", "call_quant", "call_norm")
HAS_KERNEL = ("qkn_mx_on", "call", "call_quant", "call_norm")
OPTIONS_OF = {"bf16": ("gemm_tile", "gemm_variant"), "qkn_bf16": ("gemm_tile", "gemm_variant"), "fp8": ("fp8_kernel",),
              "qkn_fp8": ("fp8_kernel",), **{e: ("mx_kernel",) for e in MX_ENTRIES}}
OPTION_VALUES = {"gemm_tile": range(-1, 7), "gemm_variant": (0, 1), "fp8_kernel": (0, 1), "mx_kernel": (0, 1)}
KERNELS = (-1, 0, 1, 2, 3, 16, 17, 18, 19)
FMTS = (E4M3, E2M3, E2M1, 7)
VALID_FMTS = ((E4M3, E4M3), (E2M3, E2M3), (E4M3, E2M1), (E2M3, E2M1))
# rows x columns x K x batch: the smallest launch, the DiT Linears at one and at eight GPUs' row counts, either side of the
# 200-tile line of the persistent fp8 / MX kernels (198, 200 and 2 x 100 tiles of 256 x 256), rows that need chunks, batch 2
SHAPES = [(300, 64, 512, 1)] + [(m, n, k, 1) for m in (17776, 2222) for n, k in ((3072, 3072), (9216, 3072), (12288, 3072), (3072, 12288))] + \
    [(2816, 4608, 512, 1), (2560, 5120, 512, 1), (2560, 2560, 512, 2), (2304, 2560, 512, 2), (90226, 12288, 3072, 1), (2222, 3072, 3072, 2)]


def base(entry):
    """A valid set of arguments of ``entry``: every pointer it takes set, 300 x 384 x 512, batch 1."""
    kind = ENTRIES[entry][3]
    v = {p: 0 for p in POINTERS}
    v.update({p: ADDR[p] for p in ENTRIES[entry][2]})
    v.update(M=M, N=N, K=K, batch=1, lda=K, ldw=K, ldc=N, ldres=N, a_batch_stride=M * K, c_batch_stride=M * N,
             res_batch_stride=M * N, gate_batch_stride=6 * N, gate_split=226, act=0, n_split=0, c_split_stride=0, alpha=0.0,
             a_fmt=E4M3, w_fmt=E4M3, out_fmt=E4M3, kernel=0, text_rows=44, width=WIDTH, eps=1e-5, k_scale=0.18,
             d_null=False, n_null=False, call_null=False, plan_null=False)
    if kind != "plain":
        v.update(ldres=0, res_batch_stride=0, gate_batch_stride=0, gate_split=0)
    if kind == "norm":                                   # C = [3, M, WIDTH]: q, k and v apart
        v.update({p: ADDR[p] for p in NORM_PTRS}, ldc=WIDTH, c_batch_stride=M * WIDTH, n_split=WIDTH, c_split_stride=M * WIDTH)
    return v


def shaped(entry, v, m, n, k, batch):
    v = dict(v, M=m, N=n, K=k, batch=batch, lda=k, ldw=k, a_batch_stride=m * k)
    kind = ENTRIES[entry][3]
    if kind == "norm":
        width = n // 3 if n % 3 == 0 else n // 2
        return dict(v, width=width, n_split=width, ldc=width, c_batch_stride=m * width, c_split_stride=batch * m * width)
    v.update(ldc=n, c_batch_stride=m * n)
    if kind == "plain":
        v.update(ldres=n, res_batch_stride=m * n, gate_batch_stride=6 * n)
    return v


# Entry points that are another one with an argument fixed, before the fold and after it (bya_gemm_mx = bya_gemm_mx_mixed with
# one format, bya_gemm_mx_qkv_norm_rope = ..._on with kernel 0), and the two other epilogues of bya_gemm_mx_call, whose argument
# functions are bya_gemm_mx_quant's and bya_gemm_mx_qkv_norm_rope_on's: they get what is their own -- null pointers, formats,
# kernel values, which epilogue a call names -- and leave the shared checks to the entry point that owns them.
THIN = ("mx", "qkn_mx", "call_quant", "call_norm", "skinny")       # (skinny: 300 rows refuse whatever else is off -- rows32 below)


def mutations(entry):
    """-> (name, arguments): the base and every single change of it."""
    _, _, ptrs, kind = ENTRIES[entry]
    b = base(entry)
    full = entry not in THIN
    yield "base", b
    for flag in ("d_null", "plan_null") + (("n_null",) if kind == "norm" else ()) + (("call_null",) if entry.startswith("call") else ()):
        if not (flag == "plan_null" and entry == "skinny"):
            yield flag, dict(b, **{flag: True})
    for p in ptrs + (NORM_PTRS if kind == "norm" else ()):
        yield f"{p}=null", dict(b, **{p: 0})
        for off in (2, 4, 8) if full and p not in NORM_PTRS[1:] else (8,) if full else ():      # (qw | qb | ... is one 16-byte check)
            yield f"{p}+{off}", dict(b, **{p: b[p] + off})
    for dim in ("M", "N", "K", "batch"):
        for bad in (0, -1):
            yield f"{dim}={bad}", dict(b, **{dim: bad})
    yield "batch=2", dict(b, batch=2)
    yield "ldc_out_of_reach", dict(b, ldc=1 << 23)      # not even one 256-row block within 2 GiB: chunk 0
    if full:
        for dk in (32, 64):                              # K off its tile (bf16: 64, fp8 / MX: 128)
            yield f"K+{dk}", dict(b, K=K + dk, lda=K + dk, ldw=K + dk)
        for dn in (2, 4):
            yield f"N+{dn}", dict(b, N=N + dn)
        for ld in ("lda", "ldw", "ldc") + (("ldres",) if kind == "plain" else ()):
            for off in (2, 4, 8):
                yield f"{ld}+{off}", dict(b, **{ld: b[ld] + off})
        for bs in ("a_batch_stride", "c_batch_stride", "res_batch_stride", "gate_batch_stride"):
            for off in (4, 8):
                yield f"{bs}+{off}", dict(b, batch=2, **{bs: b[bs] + off})
        for act in range(0, 8):
            yield f"act={act}", dict(b, act=act)
        nores = dict(b, res=0)
        for ns in (-4, 2, 4, 12, 128) if kind != "norm" else (-8, 0, 4, 12, 192):
            yield f"n_split={ns}", dict(nores, n_split=ns, c_split_stride=M * abs(ns))
        if kind == "plain":
            yield "n_split=128+res", dict(b, n_split=128, c_split_stride=M * 128)
        for off in (2, 4):
            yield f"c_split_stride+{off}", dict(nores, n_split=128, c_split_stride=M * 128 + off)
        for alpha in (1.0, 0.5):
            yield f"alpha={alpha}", dict(b, alpha=alpha)
        yield "bias_rowscale", dict(b, bias_rowscale=ADDR["bias_rowscale"])
    if entry == "skinny":
        for act in (-1, 6, 7):
            yield f"act={act}", dict(b, act=act)
    if kind != "plain":                                  # descriptor fields these entry points have no argument for
        yield "ldres=N", dict(b, ldres=N)
        yield "res_batch_stride=M*N", dict(b, res_batch_stride=M * N)
        yield "gate_batch_stride=N", dict(b, gate_batch_stride=N)
        yield "gate_split=226", dict(b, gate_split=226)
    if kind == "plain" and "gate0" in ptrs and full:
        yield "gate0_only_in_gate1", dict(b, gate0=0)
        yield "gate_split=0", dict(b, gate_split=0)
        yield "gate_split>M", dict(b, gate_split=M + 5)
        yield "ldres_out_of_reach", dict(b, ldres=1 << 23)
    if entry in MX_ENTRIES:
        if full:
            for ld in ("lda", "ldw"):                    # shorter than a row of codes
                yield f"{ld}_short", dict(b, **{ld: K - 16})
            yield "lda_short_e2m3", dict(b, a_fmt=E2M3, w_fmt=E2M3, lda=K * 6 // 8 - 16)
            yield "ldw_short_e2m1", dict(b, w_fmt=E2M1, ldw=K // 2 - 16)
        for a_fmt in FMTS:                               # every format the entry point takes
            for w_fmt in FMTS if entry != "mx" else (a_fmt,):
                for out_fmt in FMTS if entry == "call_quant" or (entry == "mx_quant" and a_fmt == w_fmt == E4M3) else (E4M3,):
                    yield f"fmt={a_fmt}{w_fmt}{out_fmt}", dict(b, a_fmt=a_fmt, w_fmt=w_fmt, out_fmt=out_fmt)
    if kind == "quant":
        yield "ldc_short", dict(b, ldc=N - 16)
        yield "ldc_e2m3", dict(b, out_fmt=E2M3, ldc=N * 6 // 8)
        yield "ldc_short_e2m3", dict(b, out_fmt=E2M3, ldc=N * 6 // 8 - 16)
        yield "N=320", dict(b, N=320)
    if entry in HAS_KERNEL:
        for kernel in KERNELS:
            yield f"kernel={kernel}", dict(b, kernel=kernel)
    if kind == "norm" and entry != "qkn_mx":
        for width in (0, 64, 192, 256):                  # 192 = N / 2: the q|k form, off the bf16 kernel's 128
            yield f"width={width}", dict(b, width=width)
        yield "width=64_q|k|v", dict(b, width=64, N=192, n_split=64, c_split_stride=M * 64, ldc=64)
        for tr in (-1, 0, M, M + 7):
            yield f"text_rows={tr}", dict(b, text_rows=tr)
            yield f"text_rows={tr},cos=null", dict(b, text_rows=tr, cos=0)
            yield f"text_rows={tr},cos=sin=null", dict(b, text_rows=tr, cos=0, sin=0)
        yield "text_rows=0,sin=null", dict(b, text_rows=0, sin=0)
        yield "k_scale=0", dict(b, k_scale=0.0)
    if entry == "call":                                  # one epilogue per call
        nb = base("call_norm")
        yield "norm+q_scales", dict(nb, q_scales=ADDR["q_scales"])
        for extra in ("res", "gate0", "gate1"):
            yield f"norm+{extra}", dict(nb, **{extra: ADDR[extra]})
            yield f"q_scales+{extra}", dict(base("call_quant"), **{extra: ADDR[extra]})


# where the formats and the kernel value are crossed: several rounds of tiles, and either side of the 200-tile line
CROSS_SHAPES = [(17776, 3072, 3072, 1), (2816, 4608, 512, 1), (2560, 5120, 512, 1)]
CHUNKED = (90226, 12288, 3072, 1)


def cases():
    """-> [(case id, entry, {option: value}, arguments)]"""
    out = []

    def add(entry, opts, tag, v):
        otag = ",".join(f"{o}={val}" for o, val in opts.items())
        out.append((f"{entry}/{otag}/{tag}", entry, opts, v))

    for entry in ENTRIES:
        for name, v in mutations(entry):
            out.append((f"{entry}/{name}", entry, {}, v))
        b = base(entry)
        if entry == "skinny":                            # one reason to refuse at a time, from a launch the kernel would take
            ok = dict(b, M=32, lda=K, a_batch_stride=32 * K)
            for name, ch in (("K=128", dict(K=128)), ("K=528", dict(K=528, lda=528, ldw=528)), ("N=392", dict(N=392)), ("N=8448", dict(N=8448)),
                             ("M=65", dict(M=65)), ("lda+4", dict(lda=K + 4)), ("ldw+4", dict(ldw=K + 4)), ("a_batch_stride+4", dict(a_batch_stride=32 * K + 4)),
                             ("A+8", dict(A=ADDR["A"] + 8)), ("W+8", dict(W=ADDR["W"] + 8)), ("n_split=128", dict(n_split=128)),
                             ("bias_rowscale", dict(bias_rowscale=ADDR["bias_rowscale"])), ("act=7", dict(act=7)), ("M=0", dict(M=0))):
                out.append((f"{entry}/rows32/{name}", entry, {}, dict(ok, **ch)))
            continue
        # 1. every shape under every value of each option (bf16: the 8-wave variant with the tiles it changes)
        states = [{o: val} for o in OPTIONS_OF[entry] for val in OPTION_VALUES[o]
                  if not (entry == "qkn_bf16" and o == "gemm_tile" and val in (1, 2, 3, 4))]      # (its row plan reads 5 and 6 only)
        if "gemm_variant" in OPTIONS_OF[entry]:
            states += [dict(gemm_tile=t, gemm_variant=1) for t in (4, 5, 6)]
        few = CROSS_SHAPES + [CHUNKED, (2222, 9216, 3072, 1), (2560, 2560, 512, 2)]
        for opts in states:
            forced = opts.get("gemm_tile", -1) >= 0      # (a forced tile is the path whatever the shape)
            for m, n, k, batch in few if entry in THIN or forced else SHAPES:
                add(entry, opts, f"{m}x{n}x{k}x{batch}", shaped(entry, b, m, n, k, batch))
            if entry == "bf16" and opts.get("gemm_tile") in (-1, 4) and len(opts) == 1:  # a forced tile against every activation and what makes a launch ineligible
                big = shaped(entry, b, 17776, 3072, 3072, 1)
                for act in range(1, 8):
                    add(entry, opts, f"17776x3072x3072x1/act={act}", dict(big, act=act))
                for name, ch in (("res=null", dict(res=0)), ("gates=null", dict(gate0=0, gate1=0)), ("C+8", dict(C=ADDR["C"] + 8)),
                                 ("K=128", dict(K=128, lda=128, ldw=128)), ("K=192", dict(K=192, lda=192, ldw=192)), ("ldc+4", dict(ldc=3076))):
                    add(entry, opts, f"17776x3072x3072x1/{name}", dict(big, **ch))
        # 2. MX: formats x what names the kernel (the option for the older entry points, the argument for _on and bya_gemm_mx_call)
        if entry in MX_ENTRIES:
            fmts = VALID_FMTS if entry != "mx" else ((E4M3, E4M3), (E2M3, E2M3))
            named = [({}, kn) for kn in ((0, 1, 2) if entry == "qkn_mx_on" else (0, 1, 2, 17, 18))] if entry in HAS_KERNEL else \
                [({"mx_kernel": val}, 0) for val in (0, 1, 2)]
            if entry.startswith("call"):
                named.append(({"mx_kernel": 1}, 0))      # (the option is not read there)
            for m, n, k, batch in CROSS_SHAPES + ([CHUNKED] if entry in ("mx_mixed", "call") else []):
                for a_fmt, w_fmt in fmts:
                    for out_fmt in ((a_fmt, E4M3 + E2M3 - a_fmt) if ENTRIES[entry][3] == "quant" else (E4M3,)):
                        for opts, kernel in named:
                            if out_fmt != a_fmt and kernel not in (1, 17) and opts.get("mx_kernel") != 1:
                                continue                 # (output in the other format: where it decides, once)
                            v = dict(shaped(entry, b, m, n, k, batch), a_fmt=a_fmt, w_fmt=w_fmt, out_fmt=out_fmt, kernel=kernel)
                            add(entry, opts, f"{m}x{n}x{k}x{batch}/f{a_fmt}{w_fmt}{out_fmt}/k{kernel}", v)
    assert len({c[0] for c in out}) == len(out)
    return out


def skinny_refuses(v):
    """bya_gemm_skinny_bf16 has no plan query: its own rules, restated, say that a case launches nothing."""
    if v["d_null"] or not (v["A"] and v["W"] and v["C"]) or min(v["M"], v["N"], v["K"], v["batch"]) <= 0 or not 0 <= v["act"] <= 6:
        return True
    return (v["M"] > 64 or v["N"] > 8192 or v["K"] < 256 or v["K"] % 32 or v["N"] % 16 or v["lda"] % 8 or v["ldw"] % 8 or
            v["a_batch_stride"] % 8 or v["bias_rowscale"] or v["n_split"] != 0 or ((v["A"] | v["W"]) & 15)) != 0


def arguments(entry, v):
    """The ctypes arguments of ``entry`` up to (not including) its last one, the plan or the stream; and what must stay alive."""
    from bind_your_avatar_implementation_amd import _hip
    vp = lambda name: ctypes.c_void_p(v[name] or None)
    d = _hip.GemmDesc(v["M"], v["N"], v["K"], v["batch"], v["lda"], v["ldw"], v["ldc"], v["ldres"], v["a_batch_stride"], v["c_batch_stride"],
                      v["res_batch_stride"], v["gate_batch_stride"], v["gate_split"], v["act"], v["n_split"], v["c_split_stride"],
                      v["bias_rowscale"] or None, v["alpha"])
    n = _hip.QkNormDesc(*(v[p] or None for p in NORM_PTRS), v["text_rows"], v["width"], v["eps"], v["k_scale"])
    dp = None if v["d_null"] else ctypes.byref(d)
    np_ = None if v["n_null"] else ctypes.byref(n)
    ops8 = [vp(p) for p in ("A", "a_scale", "W", "w_scale", "bias", "C")]
    epi = [vp(p) for p in ("res", "gate0", "gate1")]
    if entry == "bf16":
        return [vp("A"), vp("W"), vp("bias"), vp("C"), *epi, dp], (d, n)
    if entry == "skinny":
        return [vp("A"), vp("W"), vp("bias"), vp("C"), vp("res"), dp], (d, n)
    if entry == "qkn_bf16":
        return [vp("A"), vp("W"), vp("bias"), vp("C"), dp, np_], (d, n)
    if entry == "fp8":
        return [*ops8, *epi, dp], (d, n)
    if entry == "qkn_fp8":
        return [*ops8, dp, np_], (d, n)
    if entry == "mx":
        return [*ops8, *epi, dp, v["a_fmt"]], (d, n)
    if entry == "mx_mixed":
        return [*ops8, *epi, dp, v["a_fmt"], v["w_fmt"]], (d, n)
    if entry == "mx_quant":
        return [*ops8, vp("q_scales"), dp, v["a_fmt"], v["w_fmt"], v["out_fmt"]], (d, n)
    if entry == "qkn_mx":
        return [*ops8, v["a_fmt"], v["w_fmt"], dp, np_], (d, n)
    if entry == "qkn_mx_on":
        return [*ops8, v["a_fmt"], v["w_fmt"], dp, np_, v["kernel"]], (d, n)
    call = _hip.MxGemmCall(*(v[p] or None for p in ("A", "a_scale", "W", "w_scale", "bias", "C", "res", "gate0", "gate1", "q_scales")),
                           ctypes.pointer(n) if any(v[p] for p in NORM_PTRS) and not v["n_null"] else None,
                           v["a_fmt"], v["w_fmt"], v["out_fmt"], v["kernel"])
    return [None if v["call_null"] else ctypes.byref(call), dp], (d, n, call)


def answer(lib, entry, v, refused_before=None):
    """[return code, path, m0, tail, split_k, row_chunks (from the sentinel)] of the plan query, + the launch entry point's return
    code where the query refuses (``refused_before``: whether the RECORDED query did -- None while recording)."""
    from bind_your_avatar_implementation_amd import _hip
    plan_fn, launch_fn, _, _ = ENTRIES[entry]
    args, _alive = arguments(entry, v)
    if plan_fn is None:
        assert skinny_refuses(v), (entry, v)
        return [getattr(lib, launch_fn)(*args, None)]
    if v["plan_null"]:
        return [getattr(lib, plan_fn)(*args, None)]
    plan = _hip.GemmPlan(*[SENTINEL] * 5)
    rc = getattr(lib, plan_fn)(*args, ctypes.byref(plan))
    got = [rc, plan.path, plan.m0, plan.tail, plan.split_k, plan.row_chunks]
    if rc != 0 and refused_before is not False:
        got.append(getattr(lib, launch_fn)(*args, None))
    return got


def replay(lib, golden=None):
    """Every case against ``lib`` -> {case id: answer}; the options go back to what they were."""
    from bind_your_avatar_implementation_amd import _hip
    assert _hip.get_option("gemm_splitk") == 0            # (its answers depend on a registered workspace: left alone)
    names = sorted({o for opts in OPTIONS_OF.values() for o in opts})
    before = {o: _hip.get_option(o) for o in names}
    out = {}
    try:
        for cid, entry, opts, v in cases():
            for o in names:
                _hip.set_option(o, opts.get(o, _hip.OPTION_DEFAULTS[o]))
            refused = None if golden is None else (cid in golden and golden[cid][0] != 0)
            out[cid] = answer(lib, entry, v, refused)
    finally:
        for o, val in before.items():
            _hip.set_option(o, val)
    assert {o: _hip.get_option(o) for o in names} == before
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def answers(golden):
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    return replay(_hip.load(), golden)


def test_the_table_is_the_recorded_one(answers, golden):
    assert sorted(answers) == sorted(golden)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_return_codes_and_plans_are_the_recorded_ones(answers, golden, entry):
    ids = [c for c in golden if c.split("/")[0] == entry]
    assert ids
    wrong = {c: (answers[c], golden[c]) for c in ids if answers[c] != golden[c]}
    assert not wrong, f"{len(wrong)} of {len(ids)}: " + "; ".join(f"{c}: got {g}, recorded {r}" for c, (g, r) in sorted(wrong.items())[:12])


def test_the_recording_covers_what_it_should(golden):
    OK, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -4
    for entry, (plan_fn, _, _, kind) in ENTRIES.items():
        rows = {c: a for c, a in golden.items() if c.split("/")[0] == entry}
        codes = {a[0] for a in rows.values()}
        if plan_fn is None:
            assert codes == {SHAPE, UNSUPPORTED}, codes                   # never launched
            continue
        assert {SHAPE, UNSUPPORTED} | ({ALIGN} if entry not in THIN else set()) <= codes, (entry, codes)
        assert OK in codes and rows[f"{entry}/base"][0] == OK, entry
        assert rows[f"{entry}/plan_null"] == [SHAPE]
        assert rows[f"{entry}/ldc_out_of_reach"][0] == (OK if kind == "quant" else UNSUPPORTED)      # (codes: 64-bit addressed)
        for cid, a in rows.items():
            if len(a) == 1:
                continue
            if a[0] != 0:                                                  # a refused query leaves the plan alone, and the launch
                assert a[1:6] == [SENTINEL] * 5 and a[6] == a[0], cid      # entry point refuses with the same code
            else:
                assert len(a) == 6 and a[1] >= 0 and a[5] >= 1, cid
    chunked = {c.split("/")[0] for c, a in golden.items() if a[0] == 0 and a[5] > 1}
    assert chunked == {"bf16", "fp8", "mx", "mx_mixed", "call"}            # the others never cut a launch
    paths = lambda entry: {a[1] for c, a in golden.items() if c.split("/")[0] == entry and a[0] == 0}
    assert paths("bf16") == set(range(8)) and {4, 5} <= paths("qkn_bf16")
    assert paths("fp8") == {1, 4} and paths("qkn_fp8") == {1, 4}
    for entry in MX_ENTRIES:
        assert {1, 3} <= paths(entry), entry
        assert (4 in paths(entry)) == (entry != "qkn_mx"), entry            # (bya_gemm_mx_qkv_norm_rope: the tiled kernel, always)
    assert any(a[0] == 0 and a[2] > 0 for c, a in golden.items() if c.startswith("bf16/"))       # a row split ...
    assert any(a[0] == 0 and a[2] > 0 for c, a in golden.items() if c.startswith("qkn_bf16/"))   # ... and the q/k-norm one
    # value 16 (the flag bit alone) is a kernel of bya_gemm_mx_call and not one of bya_gemm_mx_qkv_norm_rope_on
    assert golden["qkn_mx_on/kernel=16"][0] == SHAPE and golden["call_norm/kernel=16"][0] == OK


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bind_your_avatar_implementation_amd import _hip
    table = replay(_hip.load())
    with open(GOLDEN, "w") as f:                                         # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(table[cid], separators=(',', ':'))}" for cid in sorted(table)) + "\n}\n")
    print(f"{len(table)} cases from {_hip.LIB_PATH} -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
