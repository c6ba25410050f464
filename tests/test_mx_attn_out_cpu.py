"""CPU: the C ABI of the attention whose epilogue writes MX codes (include/bya.h, bya_attn_fwd_mx / bya_attn_mx_plan) --
declared, exported, bound; every argument check runs before any launch, so it runs here, without a GPU; the plan query makes
bya_attn_plan's decisions; the Python front end (ops.attention(mx_out=...), enable_mx_weights(fuse_attention_quant=...)); and
the data condition of the exact-data GPU test: the closed-form outputs of tests/exact_attn.py quantise to ordinary MX blocks.
tests/test_mx_attn_out_gpu.py checks the bytes."""
import ctypes
import os
import re
import types

import pytest
import torch

import exact_attn as X
from test_mx_cpu import dequant_mx, quant_mx_ref

E4M3, E2M3, E2M1 = 0, 2, 4
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("mxfp8", "mxfp6")
BASE = 1 << 40                                                            # never dereferenced: every launch below is refused


def lib_and_hip():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    return _hip.load(), _hip


def test_symbols_are_declared_exported_and_bound():
    lib, _hip = lib_and_hip()
    header = open(os.path.join(ROOT, "include", "bya.h")).read()
    for name, nargs in (("bya_attn_fwd_mx", 14), ("bya_attn_mx_plan", 12)):
        m = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/bya.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name]) == nargs
        fn = getattr(lib, name)                                          # exported (AttributeError otherwise)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    # bya_attn_desc and bya_attn_fwd stand as they were: the descriptor has no MX field
    desc = re.search(r"typedef struct bya_attn_desc \{(.*?)\} bya_attn_desc;", header, re.S).group(1)
    assert "codes" not in desc and "scales" not in desc and "fmt" not in desc
    assert len(re.search(r"\bint bya_attn_fwd\(([^;]*)\);", header).group(1).split(",")) == 6


def desc(_hip, head_dim=64, heads=8, nb1=1, nb2=1, Sq=300, Skv=300, prescaled=0, bound=0.0):
    d = _hip.AttnDesc()
    d.head_dim, d.heads, d.nb1, d.nb2, d.Sq, d.Skv = head_dim, heads, nb1, nb2, Sq, Skv
    ld = heads * head_dim
    d.q_s1, d.q_s2, d.q_row = nb2 * Sq * ld, 0, ld
    d.k_s1, d.k_s2, d.k_row = nb2 * Skv * ld, Skv * ld, ld
    d.v_s1, d.v_s2, d.v_row = nb2 * Skv * ld, Skv * ld, ld
    d.scale, d.scores_prescaled, d.score_bound = 0.125, prescaled, bound
    return d


def strides(d, fmt):
    cb, sb = d.heads * 2 * (32 if fmt == E4M3 else 24), d.heads * 2
    return [d.nb2 * d.Sq * cb, d.Sq * cb, cb, d.nb2 * d.Sq * sb, d.Sq * sb, sb]


def test_validation_table_runs_before_any_launch():
    lib, _hip = lib_and_hip()

    def call(d, fmt=E2M3, q=BASE, k=BASE, v=BASE, codes=BASE, scales=BASE, st=None):
        st = strides(d, fmt if fmt in (E4M3, E2M3) else E2M3) if st is None else st
        return lib.bya_attn_fwd_mx(q, k, v, codes, scales, ctypes.byref(d), fmt, *st, None)

    d = desc(_hip)
    # NULL pointers: BYA_ERR_SHAPE
    for kw in ({"q": None}, {"k": None}, {"v": None}, {"codes": None}, {"scales": None}):
        assert call(d, **kw) == ERR_SHAPE, kw
    assert lib.bya_attn_fwd_mx(BASE, BASE, BASE, BASE, BASE, None, E2M3, *strides(d, E2M3), None) == ERR_SHAPE
    # head_dim != 64: BYA_ERR_UNSUPPORTED (128 is a legal bya_attn_fwd head_dim, 96 is none)
    assert call(desc(_hip, head_dim=128)) == ERR_UNSUPPORTED
    assert call(desc(_hip, head_dim=96)) == ERR_UNSUPPORTED
    # e2m1 and unknown output formats: BYA_ERR_UNSUPPORTED
    for fmt in (E2M1, 1, 3, -1, 7):
        assert call(d, fmt=fmt) == ERR_UNSUPPORTED, fmt
    # bad shapes: BYA_ERR_SHAPE -- sizes, a code / scale row stride below the row, negative batch strides, o_* strides set
    for kw in ({"heads": 0}, {"nb1": 0}, {"nb2": 0}, {"Sq": 0}, {"Skv": 0}):
        assert call(desc(_hip, **kw), st=strides(d, E2M3)) == ERR_SHAPE, kw
    for fmt in (E4M3, E2M3):
        for i, delta in ((2, -4), (5, -1), (0, None), (1, None), (3, None), (4, None)):
            st = strides(d, fmt)
            st[i] = -4 if delta is None else st[i] + delta
            assert call(d, fmt=fmt, st=st) == ERR_SHAPE, (fmt, i)
    for name in ("o_s1", "o_s2", "o_row"):
        bad = desc(_hip)
        setattr(bad, name, 512)
        assert call(bad) == ERR_SHAPE, name
    # misaligned codes pointer or code strides (a lane stores 16 or 12 bytes as dwords): BYA_ERR_ALIGN; the scale bytes are
    # stored one by one -- any address and any stride
    for fmt in (E4M3, E2M3):
        for off in (1, 2, 3):
            assert call(d, fmt=fmt, codes=BASE + off) == ERR_ALIGN, (fmt, off)
        for i in (0, 1, 2):
            for off in (1, 2):
                st = strides(d, fmt)
                st[i] += off
                assert call(d, fmt=fmt, st=st) == ERR_ALIGN, (fmt, i, off)
    # what bya_attn_fwd refuses for q, k, v holds here too
    assert call(d, q=BASE + 8) == ERR_ALIGN
    odd = desc(_hip)
    odd.k_row += 4
    assert call(odd) == ERR_ALIGN
    # the same table through the plan query; the plan is untouched on rejection
    pl = _hip.AttnPlan(-9, -9, -9, -9, -9, -9, -9, -9)
    q = lambda dd, fmt=E2M3, codes=BASE, st=None: lib.bya_attn_mx_plan(
        ctypes.byref(dd), codes, BASE, fmt, *(strides(dd, E2M3) if st is None else st), 0, ctypes.byref(pl))
    assert q(desc(_hip, head_dim=128)) == ERR_UNSUPPORTED and q(d, fmt=E2M1) == ERR_UNSUPPORTED
    assert q(d, codes=BASE + 2) == ERR_ALIGN and q(desc(_hip, Sq=0), st=strides(d, E2M3)) == ERR_SHAPE
    assert (pl.variant, pl.grid, pl.q_tile, pl.o_wide) == (-9, -9, -9, -9)
    assert lib.bya_attn_mx_plan(ctypes.byref(d), BASE, BASE, E2M3, *strides(d, E2M3), 0, None) == ERR_SHAPE


def test_plan_query_makes_the_decisions_of_the_bf16_launch():
    lib, _hip = lib_and_hip()
    pm, pb = _hip.AttnPlan(), _hip.AttnPlan()
    cases = [dict(), dict(prescaled=1), dict(prescaled=1, bound=88.0), dict(prescaled=1, bound=200.0),
             dict(prescaled=1, bound=88.0, heads=48, Sq=17776, Skv=17776), dict(prescaled=1, bound=88.0, heads=6, Sq=2222, Skv=17776),
             dict(prescaled=1, bound=88.0, heads=32, Sq=5056, Skv=5056), dict(heads=3, Sq=1031, Skv=4133, nb1=2, nb2=2)]
    for kw in cases:
        for ws in (0, 1):
            for fmt in (E4M3, E2M3):
                d = desc(_hip, **kw)
                assert lib.bya_attn_mx_plan(ctypes.byref(d), BASE, BASE, fmt, *strides(d, fmt), ws, ctypes.byref(pm)) == OK
                d.o_s1, d.o_s2, d.o_row = d.q_s1, d.Sq * d.q_row, d.q_row
                assert lib.bya_attn_plan(ctypes.byref(d), BASE, ws, ctypes.byref(pb)) == OK
                same = ("variant", "grid", "q_tile", "stream_k", "sk_rem", "sk_cut", "second_launch")
                assert [getattr(pm, f) for f in same] == [getattr(pb, f) for f in same], (kw, ws)
                assert pm.o_wide == 0
    d = desc(_hip, prescaled=1, bound=88.0, heads=48, Sq=17776, Skv=17776)
    assert lib.bya_attn_mx_plan(ctypes.byref(d), BASE, BASE, E2M3, *strides(d, E2M3), 1, ctypes.byref(pm)) == OK
    assert pm.stream_k == 1 and pm.q_tile == 512                             # the flagship shape: the stream-K grid


def test_python_front_end():
    from bind_your_avatar_implementation_amd import ops
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device="meta")
    kw = dict(head_dim=64, heads=8, nb1=2, nb2=1, Sq=300, Skv=300, q_strides=(300 * 512, 0, 512), k_strides=(300 * 512, 0, 512),
              v_strides=(300 * 512, 0, 512), scale=1.0, prescaled=True, score_bound=88.0)
    for fmt in FORMATS:
        pair = (u8(2, 300, ops.mx_code_bytes(512, fmt)), u8(2, 300, 16), fmt)
        plan = ops.attention_plan(None, mx_out=pair, workspace=False, **kw)
        assert plan["mx_out"] == fmt and plan["variant"] == "d64_static_bound_w4" and plan["q_tile"] == 512
        assert ops.attention_plan_key(plan) == "d64_static_bound_w4/" + fmt
    # the bf16 plan and its key are what they were
    plan = ops.attention_plan(torch.empty(2, 300, 512, dtype=torch.bfloat16, device="meta"), o_strides=(300 * 512, 0, 512),
                              workspace=False, **kw)
    assert "mx_out" not in plan and ops.attention_plan_key(plan) == "d64_static_bound_w4/wide"
    good = (u8(2, 300, 384), u8(2, 300, 16))
    with pytest.raises(ValueError):                                       # e2m1 is never an activation format
        ops.attention_plan(None, mx_out=(u8(2, 300, 256), u8(2, 300, 16), "mxfp4"), workspace=False, **kw)
    with pytest.raises(ValueError):                                       # codes of the wrong size (mxfp8's, for mxfp6)
        ops.attention_plan(None, mx_out=(u8(2, 300, 512), good[1], "mxfp6"), workspace=False, **kw)
    with pytest.raises(ValueError):                                       # scales of the wrong size
        ops.attention_plan(None, mx_out=(good[0], u8(2, 300, 8), "mxfp6"), workspace=False, **kw)
    with pytest.raises(ValueError):                                       # a row too few
        ops.attention_plan(None, mx_out=(u8(2, 299, 384), good[1], "mxfp6"), workspace=False, **kw)
    with pytest.raises(TypeError):                                        # codes are bytes
        ops.attention_plan(None, mx_out=(torch.empty(2, 300, 192, dtype=torch.bfloat16, device="meta"), good[1], "mxfp6"),
                           workspace=False, **kw)
    with pytest.raises(TypeError):
        ops.attention_plan(None, mx_out=(good[0], good[1].to(torch.int8), "mxfp6"), workspace=False, **kw)
    with pytest.raises(ValueError):                                       # a bf16 output AND an MX pair
        ops.attention_plan(torch.empty(2, 300, 512, dtype=torch.bfloat16, device="meta"), mx_out=(*good, "mxfp6"),
                           workspace=False, **kw)
    with pytest.raises(ValueError):                                       # head_dim 128 has no MX epilogue
        ops.attention_plan(None, mx_out=(u8(2, 300, 768), u8(2, 300, 32), "mxfp6"), workspace=False, **{**kw, "head_dim": 128})
    # the launch wrappers check the pair before anything is launched (no GPU here: CPU tensors of the wrong kind)
    cpu = lambda *s: torch.empty(*s, dtype=torch.uint8)
    q = torch.empty(2, 300, 512, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.attention(q, q, q, None, mx_out=(cpu(2, 300, 256), cpu(2, 300, 16), "mxfp4"), **kw)
    with pytest.raises(ValueError):
        ops.attention(q, q, q, None, mx_out=(cpu(2, 300, 512), cpu(2, 300, 16), "mxfp6"), **kw)
    with pytest.raises(TypeError):
        ops.attention(q, q, q, None, mx_out=(cpu(2, 300, 384).to(torch.int16), cpu(2, 300, 16), "mxfp6"), **kw)


def test_the_model_switch():
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    enable = BindyouravatarTransformer3DModel.enable_mx_weights
    calls = []
    fake = types.SimpleNamespace(invalidate_engine=lambda: calls.append(1))
    enable(fake, "mxfp6")
    assert fake._mx_fuse_attention_quant is False and fake._mx_fuse_activation_quant is True and calls == [1]   # off by default
    enable(fake, "mxfp6", fuse_attention_quant=True)
    assert fake._mx_fuse_attention_quant is True and fake._mx_fuse_activation_quant is True and calls == [1, 1]
    enable(fake, "mxfp6", fuse_attention_quant=False, fuse_activation_quant=False)
    assert fake._mx_fuse_attention_quant is False and fake._mx_fuse_activation_quant is False and calls == [1, 1, 1]
    # keyword only; a non-bool is refused and leaves the model as it was
    enable(fake, "mxfp8", fuse_attention_quant=True)
    before = dict(vars(fake))
    with pytest.raises(TypeError):
        enable(fake, "mxfp6", True, None, None, True, True)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError):
            enable(fake, "mxfp6", fuse_attention_quant=bad)
    assert vars(fake) == before and calls == [1, 1, 1, 1]
    assert fake._mx_weights == "mxfp8" and fake._mx_fuse_attention_quant is True


def d64_cases():
    return [c for c in X.ATTN_CASES if c["D"] == 64]


@pytest.mark.parametrize("case", [c for c in d64_cases() if c["Sq"] <= 5056], ids=lambda c: c["name"])
def test_exact_outputs_quantise_to_ordinary_blocks(case):
    """The closed-form outputs are multiples of 1/32 of magnitude in [1, 7] (exact_attn.py): every block has a non-zero
    maximum (no zero-scale block: scale byte 127 - emax .. 129 - emax, never the zero block's 127 with all-zero codes), nothing
    saturates (the block maximum, 1.75 * 2^n at most, maps onto or below the format's largest magnitude, 1.75 * 2^8 / 1.875 * 2^2), so the GPU comparison exercises the ordinary
    path: scale from the maximum's exponent, RNE of the scaled elements."""
    c = case
    d = X.attn_case_data(c, "cpu")
    want = d["want"].to(torch.bfloat16)
    assert torch.equal(want.float(), d["want"])
    for fmt in FORMATS:
        codes, scales = quant_mx_ref(want, fmt)
        back = dequant_mx(codes, scales, fmt)
        emax, top = (8, 448.0) if fmt == "mxfp8" else (2, 7.5)
        amax = want.float().abs().reshape(*want.shape[:-1], -1, 32).amax(-1)
        assert float(amax.min()) >= 1.0 and float(amax.max()) <= 7.0
        assert int(scales.min()) >= 127 - emax and int(scales.max()) <= 129 - emax          # 2^0 .. 2^2 = floor(log2 amax)
        scaled = want.double().reshape(*want.shape[:-1], -1, 32) * torch.exp2(127.0 - scales.double())[..., None]
        assert float(scaled.abs().max()) <= top                   # nothing is clamped: at most the largest magnitude itself
        assert bool((codes.reshape(*scales.shape, -1).amax(-1) != 0).all())                   # no all-zero block
        # the round trip: within half a step of the block's largest binade (3 mantissa bits: 2^-4 relative to the block maximum)
        err = (back - want.double()).abs().reshape(*want.shape[:-1], -1, 32).amax(-1)
        assert bool((err <= amax.double() * 2.0 ** -4).all())
        if fmt == "mxfp8":
            # e4m3 keeps 4 significant bits per element: values with at most 4 are exact
            few = (want.double() * 32).abs()
            exact = (few / torch.exp2(torch.floor(torch.log2(few.clamp(min=1))) - 3)) % 1 == 0
            assert torch.equal(back[exact], want.double()[exact])
