"""bya_gemm_fp8 on exact data (tests/exact_gemm.py, "The fp8 product through the whole epilogue"): every epilogue kind, both
kernels -- the 128 x 128 one (csrc/gemm_fp8_kernel*.h, path "t128x128") and the hand-placed persistent 256 x 256 one
(csrc/gemm_fp8_v4.hip, "p256") -- ragged and misaligned outputs, every K-tile count parity, batch 2 and row chunks.

Each case first asserts, through ``ops.gemm_fp8_plan``, the kernel it is written for (or the fallback / the error the library
answers where a kernel's eligibility rule excludes the case: a later change of the rule fails here), runs inside a ``GuardedOut``
(NaN-poisoned view, sentinel guard band) and compares BIT FOR BIT with the definition of include/bya.h restated in fp64.  The
tables are module constants: test_fp8_exact_cpu.py plans them on meta tensors and test_gemm_exact_cpu.py asserts what they cover.

K-tiles (128 bytes) and the two-stage LDS ring: the 128 x 128 kernel runs at exactly 1, 2 and 3 K-tiles (K = 128, 256, 384) and
at 96 (K = 12288); the persistent kernel's K loop is variant A, (K-tiles - 3) x variant B, C, D -- K = 512, 640, 768, 1152 are
4, 5, 6, 9 K-tiles: B once, twice, three and six times, and with an odd count the ring parity changes between consecutive tiles
of one workgroup.  Below 4 K-tiles the persistent kernel is not eligible (the "p-k384-fallback" case)."""
import pytest
import torch
import torch.nn.functional as F

from exact_gemm import (BF, CHUNK_LD, SENTINEL, GuardedOut, assert_exact, bf16_ulps, chunk_view, exact_fp8_epilogue,
                        exact_fp8_operand, reference, strided)
from exact_norm import quant_rows_fp8_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from bind_your_avatar_implementation_amd import ops
    return ops


ALL = dict(bias=True, alpha=2.0, gates="two", res="alias")          # "everything at once" (+ a gate_split inside a tile)
T128 = dict(fp8_kernel=1)

# (id, B, M, N, K, options, expected path -- or the error the library answers --, case arguments)
#   case arguments: bias, alpha, gates ("one": gate1 absent, "two"), gate_split, res ("alias": the residual IS the output,
#   "separate"), parts (n_split outputs with gaps between them), col0 (first column of the view: 4 = 8- but not 16-byte aligned),
#   batch_gates (gate vectors per batch entry: gate_batch_stride = N)
FP8_EXACT_CASES = [
    # ---- the 128 x 128 kernel: M one above / below a multiple of 128 / 256, N = 260 (N % 16 != 0), K of 1, 2, 3 K-tiles
    ("t-bare-k128", 1, 129, 260, 128, {}, "t128x128", {}),
    ("t-bias-k256", 1, 127, 260, 256, {}, "t128x128", dict(bias=True)),
    ("t-alpha-k384", 1, 257, 260, 384, {}, "t128x128", dict(bias=True, alpha=0.5)),
    ("t-gate1", 1, 255, 260, 256, {}, "t128x128", dict(bias=True, gates="one")),
    ("t-gates-inside", 1, 300, 260, 256, {}, "t128x128", dict(bias=True, gates="two", gate_split=70)),
    ("t-gates-boundary", 1, 300, 260, 128, {}, "t128x128", dict(gates="two", gate_split=256)),
    ("t-gates-at-0", 1, 300, 260, 384, {}, "t128x128", dict(gates="two", gate_split=0)),
    ("t-gates-at-m", 1, 300, 260, 256, {}, "t128x128", dict(gates="two", gate_split=300)),
    ("t-res-separate", 1, 129, 260, 384, {}, "t128x128", dict(bias=True, res="separate")),
    ("t-res-alias", 1, 255, 260, 128, {}, "t128x128", dict(bias=True, res="alias")),
    ("t-split3", 1, 255, 264, 256, {}, "t128x128", dict(bias=True, parts=3)),
    ("t-split3-res-refused", 1, 255, 264, 256, {}, "BYA_ERR_SHAPE", dict(bias=True, parts=3, res="separate")),
    ("t-everything", 1, 257, 260, 384, {}, "t128x128", dict(ALL, gate_split=130)),
    ("t-m1", 1, 1, 260, 256, {}, "t128x128", dict(bias=True, res="separate")),
    ("t-misaligned-c", 1, 129, 260, 256, {}, "t128x128", dict(col0=4, bias=True, res="alias")),
    ("t-k12288", 1, 130, 132, 12288, {}, "t128x128", dict(ALL, gate_split=100)),
    ("t-forced-many-tiles", 1, 3621, 3848, 512, T128, "t128x128", dict(ALL, gate_split=1000)),
    ("t-batch2", 2, 129, 260, 384, {}, "t128x128", dict(bias=True, gates="two", gate_split=70, res="separate", batch_gates=True)),
    ("t-batch2-alias-k256", 2, 255, 264, 256, {}, "t128x128", dict(ALL, gate_split=128, batch_gates=True)),
    # ---- the persistent kernel: at least 200 tiles of 256 x 256, K >= 512; M one above / below 14 * 256, N % 16 == 8
    ("p-bare-k512", 1, 3621, 3848, 512, {}, "p256", {}),
    ("p-bias-k640", 1, 3585, 3848, 640, {}, "p256", dict(bias=True)),
    ("p-alpha-k768", 1, 3583, 3848, 768, {}, "p256", dict(bias=True, alpha=0.5)),
    ("p-gate1", 1, 3621, 3848, 512, {}, "p256", dict(bias=True, gates="one")),
    ("p-gates-inside", 1, 3621, 3848, 640, {}, "p256", dict(bias=True, gates="two", gate_split=1000)),
    ("p-gates-boundary", 1, 3621, 3848, 512, {}, "p256", dict(gates="two", gate_split=1024)),
    ("p-gates-at-0", 1, 3621, 3848, 512, {}, "p256", dict(gates="two", gate_split=0)),
    ("p-gates-at-m", 1, 3621, 3848, 640, {}, "p256", dict(gates="two", gate_split=3621)),
    ("p-res-separate", 1, 3585, 3848, 768, {}, "p256", dict(bias=True, res="separate")),
    ("p-res-alias", 1, 3583, 3848, 1152, {}, "p256", dict(bias=True, res="alias")),
    ("p-split3", 1, 3621, 3840, 512, {}, "p256", dict(bias=True, parts=3)),
    ("p-split3-res-refused", 1, 3621, 3840, 512, {}, "BYA_ERR_SHAPE", dict(bias=True, parts=3, res="separate")),
    ("p-everything-k1152", 1, 3621, 3848, 1152, {}, "p256", dict(ALL, gate_split=2000)),
    ("p-m1", 1, 1, 51200, 512, {}, "p256", dict(bias=True, res="separate")),
    ("p-n264-tall", 1, 25601, 264, 640, {}, "p256", dict(ALL, gate_split=12345)),
    ("p-batch2", 2, 1811, 3848, 640, {}, "p256", dict(bias=True, gates="two", gate_split=1000, res="separate", batch_gates=True)),
    ("p-batch2-alias-k768", 2, 1811, 3848, 768, {}, "p256", dict(ALL, gate_split=300, batch_gates=True)),
    # ... and what its eligibility rule (bya_gemm256p_fp8_eligible) and fp8_path's tile count send to the 128 x 128 kernel
    ("p-n260-fallback", 1, 25601, 260, 512, {}, "t128x128", dict(bias=True)),                      # N % 8 != 0
    ("p-misaligned-c-fallback", 1, 3621, 3848, 512, {}, "t128x128", dict(col0=4, bias=True, res="alias")),
    ("p-k384-fallback", 1, 3621, 3848, 384, {}, "t128x128", dict(bias=True)),                      # fewer than 4 K-tiles
    ("p-single-tile-fallback", 1, 256, 256, 512, {}, "t128x128", dict(bias=True)),                 # under 200 tiles
]

# what test_gemm_exact_cpu.py asks of the table above, for each of the two kernels (``epilogue_kinds``)
REQUIRED_KINDS = {"bare", "bias", "bias+alpha", "one-gate", "gates-split-inside", "gates-split-boundary", "gates-split-0",
                  "gates-split-m", "res-separate", "res-alias", "n_split3", "everything"}


def epilogue_kinds(M, kw):
    """The epilogue kinds of the issue's list that a case with arguments ``kw`` exercises."""
    bias, alpha, gates, res, parts = kw.get("bias"), kw.get("alpha", 1.0), kw.get("gates"), kw.get("res"), kw.get("parts", 1)
    kinds = set()
    if not (bias or gates or res) and alpha == 1.0 and parts == 1:
        kinds.add("bare")
    if bias and not (gates or res) and parts == 1:
        kinds.add("bias" if alpha == 1.0 else "bias+alpha")
    if gates == "one":
        kinds.add("one-gate")
    if gates == "two":
        gs = kw.get("gate_split", 0)
        kinds.add("gates-split-0" if gs == 0 else "gates-split-m" if gs == M else
                  "gates-split-boundary" if gs % 256 == 0 else "gates-split-inside")
    if res:
        kinds.add("res-" + res)
    if parts == 3:
        kinds.add("n_split3")
    if bias and alpha != 1.0 and gates == "two" and res and kw.get("gate_split", 0) % 128:
        kinds.add("everything")
    return kinds


def _seed(B, M, N, K):
    return (M * 131 + N * 7 + K + 17 * B) % 100003


def meta_case(B, M, N, K, bias=False, alpha=1.0, gates=None, gate_split=0, res=None, parts=1, col0=8, batch_gates=False):
    """The arguments of a case on the meta device (the shapes, strides and view offsets of ``build_case``): for the plan
    queries without a GPU."""
    def m(*shape, dtype=BF):
        return torch.empty(*shape, dtype=dtype, device="meta")
    out = GuardedOut(M, N, "meta", batch=B, parts=parts, col0=col0)
    gshape = (B, N) if batch_gates else (N,)
    return dict(a8=m(B, M, K, dtype=torch.uint8) if B > 1 else m(M, K, dtype=torch.uint8), a_scale=m(B * M, dtype=torch.float32),
                w8=m(N, K, dtype=torch.uint8), w_scale=m(N, dtype=torch.float32), out=out.view(), bias=m(N) if bias else None,
                res=None if not res else (out.view() if res == "alias" else (m(B, M, N) if B > 1 else m(M, N))),
                gate0=m(*gshape) if gates else None, gate1=m(*gshape) if gates == "two" else None, gate_split=gate_split,
                gate_batch_stride=N if batch_gates else 0, split=out.split, alpha=alpha)


def build_case(dev, B, M, N, K, bias=False, alpha=1.0, gates=None, gate_split=0, res=None, parts=1, col0=8, batch_gates=False,
               a_scale_mul=1.0):
    """-> (args of ops.gemm_fp8 / gemm_fp8_plan, the GuardedOut, the fp64 reference, the residual values or None)."""
    seed = _seed(B, M, N, K)
    a8, sa, da = exact_fp8_operand(B * M, K, dev, seed)
    w8, sw, dw = exact_fp8_operand(N, K, dev, seed + 5)
    sa, da = sa * a_scale_mul, da * a_scale_mul
    ep = exact_fp8_epilogue(N, dev, seed + 11, bias=bias, gates=gates, alpha=alpha, res_rows=M if res else None, batch=B,
                            batch_gates=batch_gates)
    out = GuardedOut(M, N, dev, batch=B, parts=parts, col0=col0)
    res_t = res_v = None
    if res:
        res_v = ep["res"] if B > 1 else ep["res"][0]
        assert torch.equal(res_v.to(BF).float(), res_v)              # (the residual grid is exact in bf16)
        if res == "alias":
            out.fill(res_v)
            res_t = out.view()
        else:
            res_t = res_v.to(BF)
    if B > 1:
        a8, da = a8.reshape(B, M, K), da.reshape(B, M, K)
    args = dict(a8=a8, a_scale=sa, w8=w8, w_scale=sw, out=out.view(), bias=ep["bias"], res=res_t, gate0=ep["gate0"],
                gate1=ep["gate1"], gate_split=gate_split, gate_batch_stride=N if batch_gates else 0, split=out.split, alpha=alpha)
    ref = reference(da, dw, ep["bias"], ep["gate0"], ep["gate1"], gate_split, res_v, None, alpha)
    return args, out, ref, res_v


def _call(fn, args, **more):
    kw = dict(args, **more)
    return fn(kw.pop("a8"), kw.pop("a_scale"), kw.pop("w8"), kw.pop("w_scale"), kw.pop("out"), **kw)


def entry_of(args, z, M, res_v, out):
    """The B = 1 launch on batch entry ``z``'s operands of a batched case, into the GuardedOut ``out``."""
    one = dict(args, a8=args["a8"][z], a_scale=args["a_scale"][z * M:(z + 1) * M], out=out.view(), gate_batch_stride=0)
    if args["gate_batch_stride"]:
        one["gate0"] = args["gate0"][z]
        one["gate1"] = None if args["gate1"] is None else args["gate1"][z]
    if args["res"] is not None:
        if args["res"].data_ptr() == args["out"].data_ptr():
            out.fill(res_v[z])
            one["res"] = out.view()
        else:
            one["res"] = args["res"][z]
    return one


@pytest.mark.parametrize("case", FP8_EXACT_CASES, ids=[c[0] for c in FP8_EXACT_CASES])
def test_fp8_exact(ops, dev, case):
    from bind_your_avatar_implementation_amd._hip import ByaError
    cid, B, M, N, K, opts, expect, kw = case
    args, out, ref, res_v = build_case(dev, B, M, N, K, **kw)
    if B > 1:                        # the batch entries must not be interchangeable: codes, row scales, gates, residual
        assert not torch.equal(args["a8"][0], args["a8"][1]) and not torch.equal(args["a_scale"][:M], args["a_scale"][M:])
        assert not kw.get("batch_gates") or not torch.equal(args["gate0"][0], args["gate0"][1])
        assert res_v is None or not torch.equal(res_v[0], res_v[1])
    with ops.options(**opts):
        if expect.startswith("BYA_ERR"):
            with pytest.raises(ByaError, match=expect):
                _call(ops.gemm_fp8_plan, args)
            with pytest.raises(ByaError, match=expect):
                _call(ops.gemm_fp8, args)
            torch.cuda.synchronize()
            assert out.guard_intact()
            print(f"{cid}: {B}x{M}x{N}x{K} refused with {expect}")
            return
        plan = _call(ops.gemm_fp8_plan, args)
        assert plan["path"] == expect and plan["row_chunks"] == 1 and plan["m0"] == 0 and not plan["split_k"], plan
        _call(ops.gemm_fp8, args)
    torch.cuda.synchronize()
    assert_exact(out.gathered(), ref, plan, f"{cid} {B}x{M}x{N}x{K}")
    assert out.guard_intact(), f"{cid}: a write outside the output view"
    print(f"{cid}: {B}x{M}x{N}x{K} ({K // 128} K-tiles) on {plan['path']} bit-exact")
    if B > 1:                        # ... and entry 1 is what a B = 1 launch makes of entry 1's operands
        alone = GuardedOut(M, N, dev, parts=kw.get("parts", 1), col0=kw.get("col0", 8))
        one = entry_of(args, 1, M, res_v, alone)
        with ops.options(**opts):
            plan1 = _call(ops.gemm_fp8_plan, one)
            _call(ops.gemm_fp8, one)
        torch.cuda.synchronize()
        assert torch.equal(alone.gathered(), out.gathered()[1]), (cid, plan1)
        assert alone.guard_intact()
        print(f"{cid}: entry 1 equals the B = 1 launch of its operands (on {plan1['path']})")


# ---------------------------------------------------------------------------------------------------------------- activations
# bya_gemm_fp8 takes no activation, GELU(tanh) and its A/B twin (include/bya.h: act in {NONE, GELU_TANH(_IEEE)}); the epilogue
# code is csrc/gemm_common.h's, shared with the bf16 kernels, so the bounds are the bf16 suite's ACT_ULPS (worst error in bf16
# ulps; results below 2^-6: in ulps of 2^-6).  gelu_tanh_ieee has no entry there: it is the same function evaluated with expf
# and an IEEE division, a few fp32 ulps (2^-16 bf16 ulps) from the exact value, so all it can do is land on the other side of a
# bf16 rounding boundary -- 1 ulp, GELU(tanh)'s own bound, for the same reason.
FP8_ACTS = ("gelu_tanh", "gelu_tanh_ieee")
FP8_ACTS_REFUSED = ("gelu_erf", "relu", "silu", "leaky_relu")
FP8_ACT_ULPS = {"gelu_tanh": 1, "gelu_tanh_ieee": 1}
FP8_ACT_SHAPES = [(515, 264, 512, "t128x128"), (3621, 3848, 512, "p256")]


def test_activation_bounds_are_the_bf16_suites():
    from test_gemm_exact_gpu import ACT_ULPS
    assert FP8_ACT_ULPS["gelu_tanh"] == ACT_ULPS["gelu_tanh"] and FP8_ACT_ULPS["gelu_tanh_ieee"] == ACT_ULPS["gelu_tanh"]


@pytest.mark.parametrize("M,N,K,expect", FP8_ACT_SHAPES, ids=[s[-1] for s in FP8_ACT_SHAPES])
@pytest.mark.parametrize("act", FP8_ACTS)
def test_fp8_activation_of_the_exact_pre_activation(ops, dev, act, M, N, K, expect):
    """The kernel's act(pre-activation) against the fp64 activation of the EXACT pre-activation (row scales 2^-6 times the
    grid's: pre-activations of order 1, where the curve bends), element by element, within ``FP8_ACT_ULPS`` bf16 ulps."""
    args, out, pre, _ = build_case(dev, 1, M, N, K, bias=True, a_scale_mul=2.0 ** -6)
    plan = _call(ops.gemm_fp8_plan, args, act=act)
    assert plan["path"] == expect, plan
    _call(ops.gemm_fp8, args, act=act)
    torch.cuda.synchronize()
    want = F.gelu(pre, approximate="tanh")
    got = out.gathered()
    ulps, worst = bf16_ulps(got, want)
    print(f"{act} on {expect}: worst {ulps:.3f} bf16 ulp(s) from the activation of the exact pre-activation (at pre-activation "
          f"{float(pre.flatten()[worst]):.6g}: got {float(got.flatten()[worst]):.6g}, want {float(want.flatten()[worst]):.6g}); "
          f"pre-activations span {float(pre.min()):.3g} .. {float(pre.max()):.3g}")
    assert ulps <= FP8_ACT_ULPS[act], (act, ulps)
    assert out.guard_intact()


@pytest.mark.parametrize("M,N,K,expect", FP8_ACT_SHAPES, ids=[s[-1] for s in FP8_ACT_SHAPES])
def test_fp8_refuses_the_activations_it_lacks(ops, dev, M, N, K, expect):
    """Every other activation of the bf16 GEMM: BYA_ERR_UNSUPPORTED from the plan query and from the launch, at a shape of
    either kernel, and nothing written."""
    from bind_your_avatar_implementation_amd._hip import ByaError
    args, out, _, _ = build_case(dev, 1, M, N, K, bias=True)
    assert _call(ops.gemm_fp8_plan, args)["path"] == expect
    for act in FP8_ACTS_REFUSED:
        with pytest.raises(ByaError, match="BYA_ERR_UNSUPPORTED"):
            _call(ops.gemm_fp8_plan, args, act=act)
        with pytest.raises(ByaError, match="BYA_ERR_UNSUPPORTED"):
            _call(ops.gemm_fp8, args, act=act)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.gathered()).all()) and out.guard_intact()


# ----------------------------------------------------------------------------------------------------------------- row chunks
# (id, B, M, N, K, expected path, row_chunks): ``out`` = the first N columns of rows CHUNK_LD elements apart (exact_gemm.py),
# 513 rows = pieces of 256, 256 and 1 rows per batch entry.  "chunk-p256": the smallest shape with three row pieces and 200
# tiles of 256 x 256 (3 x 67; a launch of 769 rows would run as 512 + 257: gemm_chunk_rows halves to whole 256-row blocks)
CHUNK_CASES = [
    ("chunk-t128", 1, 513, 128, 128, "t128x128", 3),
    ("chunk-t128-batch2", 2, 513, 128, 128, "t128x128", 6),
    ("chunk-p256", 1, 513, 17152, 512, "p256", 3),
]
CHUNK_KW = dict(bias=True, gates="two", gate_split=300, res="alias")      # gate_split inside the SECOND piece
CHUNK_PIECES = ((0, 256), (256, 512), (512, 513))


def chunk_meta_case(B, M, N, K):
    """A CHUNK_CASES case on the meta device: the plan (and its row_chunks) needs no GPU."""
    args = meta_case(B, M, N, K, batch_gates=B > 1, **CHUNK_KW)
    _, out = chunk_view(B, M, N, "meta")
    return dict(args, out=out, res=out)


@pytest.mark.parametrize("cid,B,M,N,K,expect,chunks", CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_fp8_row_chunks_past_2gib_on_exact_data(ops, dev, cid, B, M, N, K, expect, chunks):
    """A launch cut into row chunks: every piece must start at ITS rows of the one-byte codes (row0 * lda BYTES), of the row
    scales (a_scale + z * M + m0), of the output and of the residual that aliases it, with gate_split re-based on its first
    row and, batched, its own entry's gates -- a piece fed another piece's rows or scales is wrong in almost every element."""
    plan_meta = _call(ops.gemm_fp8_plan, chunk_meta_case(B, M, N, K))
    assert plan_meta["path"] == expect and plan_meta["row_chunks"] == chunks and plan_meta["m0"] == 0, plan_meta
    seed = _seed(B, M, N, K)
    a8, sa, da = exact_fp8_operand(B * M, K, dev, seed)
    w8, sw, dw = exact_fp8_operand(N, K, dev, seed + 5)
    ep = exact_fp8_epilogue(N, dev, seed + 11, bias=True, gates="two", res_rows=M, batch=B, batch_gates=B > 1)
    a3, s2 = a8.reshape(B, M, K), sa.reshape(B, M)
    # (a one-row piece has one scale: give each its own value, which no other piece's first row has)
    s2[:, 0], s2[:, 256], s2[:, 512] = 1.0, 2.0, torch.tensor([4.0, 0.25], device=dev)[:B]
    da = a8.view(torch.float8_e4m3fn).double() * sa.double()[:, None]
    pieces = [(z, lo, hi) for z in range(B) for lo, hi in CHUNK_PIECES]
    assert len(pieces) == chunks
    for i, (z, lo, hi) in enumerate(pieces):         # codes and scales differ between the pieces
        for z2, lo2, hi2 in pieces[i + 1:]:
            n = min(hi - lo, hi2 - lo2)
            assert not torch.equal(a3[z, lo:lo + n], a3[z2, lo2:lo2 + n]) and not torch.equal(s2[z, lo:lo + n], s2[z2, lo2:lo2 + n])
    buf, out = chunk_view(B, M, N, dev)
    res_v = ep["res"] if B > 1 else ep["res"][0]
    out.copy_(res_v.to(BF))
    args = dict(a8=a3 if B > 1 else a8, a_scale=sa, w8=w8, w_scale=sw, out=out, bias=ep["bias"], res=out, gate0=ep["gate0"],
                gate1=ep["gate1"], gate_split=CHUNK_KW["gate_split"], gate_batch_stride=N if B > 1 else 0)
    plan = _call(ops.gemm_fp8_plan, args)
    assert plan == plan_meta, (plan, plan_meta)
    _call(ops.gemm_fp8, args)
    torch.cuda.synchronize()
    da = da.reshape(B, M, K) if B > 1 else da
    ref = reference(da, dw, ep["bias"], ep["gate0"], ep["gate1"], CHUNK_KW["gate_split"], res_v)
    assert_exact(out, ref, plan, f"{cid} {B}x{M}x{N}x{K}, ldc {CHUNK_LD}")
    rows = torch.tensor(sorted({r for lo, hi in CHUNK_PIECES for r in (lo, hi - 1)}), device=dev)
    assert bool((buf[:, rows, N:N + 64] == SENTINEL).all()), "canary behind the output columns of each piece's first and last row"
    print(f"{cid}: {B}x{M}x{N}x{K} in {plan['row_chunks']} row chunks on {plan['path']} bit-exact")


# ------------------------------------------------------------------------------------------------------------------ quantiser
Q_SENTINEL = 0xA5
# (id, batch, M, K, pad): K = 8 (one vector of one thread), the largest K of the entry point (12288: every thread's six
# vectors), K % 128 != 0, a strided input view (ldx = K + pad), batch 2 (evenly stacked rows, strided too)
QUANT_CASES = [("k8", 1, 37, 8, 0), ("k12288", 1, 33, 12288, 0), ("k3080", 1, 65, 3080, 0), ("strided", 1, 130, 1000, 24),
               ("batch2", 2, 67, 3080, 0), ("batch2-strided", 2, 5, 12288, 8)]


def test_quantize_rows_fp8_refuses_k_past_its_largest(ops, dev):
    """K = 12288 is the largest (QUANT_CASES runs it); the next multiple of 8 and a K % 8 != 0 are BYA_ERR_SHAPE, nothing written."""
    from bind_your_avatar_implementation_amd._hip import ByaError
    for K in (12296, 12):
        x = torch.ones(3, K, dtype=BF, device=dev)
        q = torch.full((3, K), Q_SENTINEL, dtype=torch.uint8, device=dev)
        with pytest.raises(ByaError, match="BYA_ERR_SHAPE"):
            ops.quantize_rows_fp8(x, q)
        torch.cuda.synchronize()
        assert bool((q == Q_SENTINEL).all())


@pytest.mark.parametrize("cid,B,M,K,pad", QUANT_CASES, ids=[c[0] for c in QUANT_CASES])
def test_quantize_rows_fp8_edges_byte_for_byte(ops, dev, cid, B, M, K, pad):
    """bya_quantize_rows_fp8 against its definition (exact_norm.quant_rows_fp8_ref) BYTE FOR BYTE, with sentinel bytes behind
    ``q`` and behind ``scale`` that must survive."""
    g = torch.Generator().manual_seed(K + M)
    x = (torch.randn(B, M, K, generator=g) * 3.0 * torch.exp2(torch.randint(-6, 7, (B, M, 1), generator=g).float())).to(BF)
    x[0, 1] = 0                                                      # an all-zero row: scale 1, zeros
    x[-1, 2, :7] = torch.tensor([448., -448., 1e-3, -0.0, 0.0, 1e4, -3e-5]).to(BF)
    x[0, 3, K - 1] = 3e4                                             # the row maximum in the last element
    if B == 1:
        x = x[0]
    q_ref, s_ref = quant_rows_fp8_ref(x)
    xd = strided(x.to(dev), pad)
    assert xd.stride(-2) == K + pad
    rows = B * M
    qbuf = torch.full((rows * K + 256,), Q_SENTINEL, dtype=torch.uint8, device=dev)
    sbuf = torch.full((rows + 64,), float("nan"), dtype=torch.float32, device=dev)
    sbuf.view(torch.int32).fill_(0x7FA5A5A5)
    q, s = qbuf[:rows * K].view(x.shape), sbuf[:rows].view(x.shape[:-1])
    ops.quantize_rows_fp8(xd, q, s)
    torch.cuda.synchronize()
    assert torch.equal(s.cpu(), s_ref)
    same = q.cpu() == q_ref
    print(f"{cid}: {B}x{M}x{K} (ldx {K + pad}): {int((~same).sum())} of {same.numel()} bytes differ")
    assert bool(same.all())
    assert bool((qbuf[rows * K:] == Q_SENTINEL).all()), "a write behind q"
    assert bool((sbuf.view(torch.int32)[rows:] == 0x7FA5A5A5).all()), "a write behind scale"
