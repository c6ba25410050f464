"""CPU: tests/cond_gemm_bf16.py against itself -- the generators hold the bit patterns they claim, the exactness proofs hold in
integer arithmetic on the generated bits, the conditions that keep the bars from being empty hold on the reference alone, the fp32
restatement and four other correct summations stay inside every bar on every family, each planted fault is rejected by the bar
named beside it, and the case tables of test_gemm_bf16_cond_gpu.py, planned on meta tensors, reach every bf16 GEMM path."""
import functools

import pytest
import torch

import cond_gemm as C
import cond_gemm_bf16 as B
from exact_gemm import BF

FAULT_SHAPE = (300, 264, 512)
QUIET = lambda *x: None


@functools.lru_cache(maxsize=8)
def operands(M, N, K, group="mid", batch=1):
    a, w = B.data(M, N, K, group, batch)
    return a, w, B.values(a), B.values(w)


def checked(name, got, a, w, a64, w64, e=C.NO_EPILOGUE, M=None, exact=None, rms=False, out=QUIET, extra_T=0.0, keep=None):
    """``cond_gemm.check`` exactly as ``cond_gemm_bf16.check_result`` applies it on the GPU, of a result computed here
    (``keep``: a function of y64 -> mask of the elements looked at; the others belong to no family)."""
    K = a64.shape[1]
    y, S = C.reference(a64, w64, e, M)
    fam = B.family_of(a, w, a64, w64)
    if keep is not None:
        fam = torch.where(keep(y), fam, torch.full_like(fam, B.OUTSIDE))
    plain = all(e[k] is None for k in ("bias", "act", "gate0", "res", "rowscale")) and e["alpha"] == 1.0
    orders = B.rms_orders(a64, w64, e, M) if rms else None
    return C.check(name, got, y, S, K, fam, restated=C.restate(a64, w64, e, M), ops=C.epilogue_ops(e),
                   act=e["act"], exact=(B.EXACT if plain else ()) if exact is None else exact,
                   T=B.underflow_term(K, C.epilogue_ops(e)) + extra_T, families=B.FAMILIES, rms_of=orders, out=out)


# ------------------------------------------------------------------------------------------------------------- generators
def test_row_families_hold_the_bit_patterns_they_claim():
    a, w, a64, w64 = operands(300, 264, 512)
    for op, v, side in ((a, a64, "a"), (w, w64, "w")):
        assert set(op["fam"].tolist()) == set(range(5))
        rows = lambda name: op["bits"][op["fam"] == B.FAMILIES.index(name)].long() & 0xFFFF
        vals = lambda name: v[op["fam"] == B.FAMILIES.index(name)]
        assert bool(torch.isfinite(v).all())
        assert len(set((rows("near") & 0x7F).flatten().tolist())) == 128, "near: full 8-bit significands"
        sp = vals("spread")
        nz = sp[sp != 0].abs()
        assert float(nz.min()) >= 2.0 ** -12 and float(nz.max()) < 2.0 ** 13
        assert float(nz.min()) < 2.0 ** -11 and float(nz.max()) >= 2.0 ** 12, "spread: 25 binades"
        blocks = sp.reshape(sp.shape[0], -1, 32)
        zero = (blocks == 0).all(-1).double().mean()
        assert 0.005 < float(zero) < 0.05, "spread: about 2 % of the 32-blocks all zero"
        c = vals("cancel").reshape(-1, 256, 2)
        if side == "a":
            assert torch.equal(c[..., 0], c[..., 1])
            assert bool(((rows("subnormal") & 0x7F80) == 0).all()) and bool(((rows("subnormal") & 0x7F) != 0).all())
            assert set((rows("subnormal") & 0x7F).flatten().tolist()) == set(range(1, 128))
            assert set(rows("extreme").flatten().tolist()) == {B.TOP_BITS, B.TOP_BITS | 0x8000}
            assert float(vals("extreme").abs().max()) == 255 * 2.0 ** 120 == float(torch.finfo(BF).max)
            assert float(vals("subnormal").abs().max()) == 127 * 2.0 ** -133 < float(torch.finfo(BF).tiny)
        else:
            nudged = c[..., 0] != -c[..., 1]
            assert 0.09 < float(nudged.double().mean()) < 0.16, "cancel: one pair in eight nudged"
            step = (c[..., 1].abs() - c[..., 0].abs())[nudged]
            ulp = torch.exp2(torch.floor(torch.log2(c[..., 0].abs()[nudged])) - 7)
            assert bool((step > 0).all()) and bool((step <= 2 * ulp).all()), "... by one bf16 step"
            assert set(torch.ldexp(vals("subnormal"), torch.tensor(-120)).flatten().tolist()) == set(range(-3, 4))
            assert set(torch.ldexp(vals("extreme"), torch.tensor(120)).flatten().tolist()) == set(range(-3, 4))
    # cancel: the sum is a small part of the sum of magnitudes
    y, S = C.reference(a64, w64)
    fam = B.family_of(a, w, a64, w64)
    sel = fam == B.FAMILIES.index("cancel")
    assert float((y[sel].abs() / S[sel]).median()) < 0.02 and float(S[sel].min()) > 0
    # every family of the launch appears among the outputs, and only ``mixed`` elements are outside the domain
    assert set(fam.flatten().tolist()) == set(range(6)) | {B.OUTSIDE}
    named = C.out_family(a, w) != B.MIXED
    assert float((a64.abs() @ w64.abs().T)[named].max()) < B.DOMAIN_S0 / 2 ** 90
    assert bool(torch.isfinite(y.to(BF).float()[fam != B.OUTSIDE]).all())


def test_one_hot_covers_all_65280_finite_codes_and_returns_them():
    M, N, K = B.ONE_HOT_SHAPE
    assert M * K >= B.FINITE_CODES
    a, w, a64, w64 = operands(M, N, K, "one-hot")
    codes = a["bits"].long() & 0xFFFF
    assert set(codes.flatten().tolist()) == set(B.finite_bits().tolist()) and len(B.finite_bits()) == 65280
    assert bool(torch.isfinite(a64).all())
    nz = w64 != 0
    assert bool((nz.sum(1) == 1).all()) and torch.equal(nz.int().argmax(1), torch.arange(N) % K) and bool((w64[nz] == 1.0).all())
    y, S = C.reference(a64, w64)
    want = a["bits"][:, torch.arange(N) % K]
    assert torch.equal(y.to(BF).view(torch.int16)[want != -32768], want[want != -32768]), "the output IS A[m, n mod K]"
    checked("one-hot", C.restate(a64, w64), a, w, a64, w64)
    # the second launch: -0.5 times the element, rounded once (subnormals with an odd j tie to even)
    a2, w2, a64n, w64n = operands(M, N, K, "one-hot-neg")
    assert torch.equal(a2["bits"], a["bits"]) and bool((w64n[w64n != 0] == -0.5).all())
    y2, _ = C.reference(a64n, w64n)
    assert torch.equal(y2.float().double(), y2), "a 9-bit product is exact in fp32: fp64 -> fp32 -> bf16 rounds once"
    checked("one-hot -0.5", C.restate(a64n, w64n), a2, w2, a64n, w64n)


def test_act_range_covers_the_tails():
    M, N, K = B.EPI_SHAPE
    a, w, a64, w64 = operands(M, N, K, "act-range")
    e = B.epilogue_of(M, N, K, "act-range", None, "gelu_tanh")
    pre = a64 @ w64.T + e["bias"].double()[None]
    hist = torch.histc(pre, bins=60, min=-30, max=30)
    assert float(hist.min()) > 0.5 * float(hist.mean()), "the pre-activations cover [-30, 30] evenly"
    assert int(((pre > -13) & (pre < -5)).sum()) > 5000, "... the stretch where 1 + tanh(u) cancels included"
    assert set(B.family_of(a, w, a64, w64).flatten().tolist()) == {B.ACT_RANGE}


@pytest.mark.parametrize("fam", ["subnormal", "extreme"])
def test_exact_families_are_exact_by_integer_arithmetic(fam):
    """``exact_units_bf16`` asserts the proof on the bits; here also that the fp64 reference IS the integer sum, at the longest K."""
    for M, N, K in ((60, 50, 512), (30, 25, 12288)):
        a, w, a64, w64 = operands(M, N, K)
        prod, unit = B.exact_units_bf16(a, w, fam)
        i = B.FAMILIES.index(fam)
        y, _ = C.reference(a64, w64)
        sub = y[a["fam"] == i][:, w["fam"] == i]
        assert torch.equal(sub, torch.ldexp(prod.sum(-1).double(), torch.tensor(float(unit))))
        assert bool((C.out_family(a, w) == i).any()) and float(sub.abs().max()) > 0
    assert 381 * 12288 < 2 ** 24 and 765 * 12288 < 2 ** 24


# ------------------------------------------------------------------------------- conditions that keep the bars from being empty
def test_eps_is_small_on_near_rows_where_the_bars_must_bite():
    for K, share in ((64, 0.90), (192, 0.90), (512, 0.75)):
        a, w, a64, w64 = operands(300, 264, K)
        y, S = C.reference(a64, w64)
        near = B.family_of(a, w, a64, w64) == 0
        got = float((C.eps_of(S, C._ulp(y), K)[near] <= 0.5).double().mean())
        print(f"K = {K}: {got:.3f} of the near elements have eps <= 0.5")
        assert got >= share, (K, got)


def test_every_tiled_case_holds_every_row_family_16_rows_deep():
    """(bya_gemm_skinny_bf16 takes at most 64 rows and its cases as few as one: there W alone holds every family, 54 rows deep.)"""
    for c in B.tiled_cases():
        if c["group"] != "mid":
            continue
        for rows, shift in ((c["batch"] * c["M"], 0), (c["N"], 2)):
            fam = (torch.arange(rows) + shift) % 5
            assert int(torch.bincount(fam, minlength=5).min()) >= 16, c["id"]
    assert B.SKINNY_N // 5 >= 16


def test_res_cancel_results_are_a_few_steps_of_the_value_before_the_residual():
    for K in (64, 512):
        M, N = B.EPI_SHAPE[:2]
        a, w, a64, w64 = operands(M, N, K)
        e = B.epilogue_of(M, N, K, "mid", "res-cancel", None)
        y, S = C.reference(a64, w64, e, M)
        before, _ = C.reference(a64, w64, {**e, "res": None}, M)
        inside = B.family_of(a, w, a64, w64) != B.OUTSIDE
        steps = (y.abs() / C._ulp(before))[inside]
        assert float(steps.max()) < B.RES_CANCEL_STEPS and float(steps.median()) > 0.5, (K, float(steps.max()))
        # the derived eps allows about 2^-17 of S at K = 64: 2 (64 + 4) 2^-24
        if K == 64:
            assert 2 * (K + C.epilogue_ops(e)) * C.U32 < 2.0 ** -16.9


# ----------------------------------------------------------------------------------- the restatement and other correct sums
PLAIN_SHAPES = sorted({(300, 264, K) for K in (64, 192, 256, 512)} | set(B.LONG_K_SHAPES))


@pytest.mark.parametrize("M,N,K", PLAIN_SHAPES)
def test_restatement_orders_and_two_other_sums_pass_every_bar(M, N, K):
    a, w, a64, w64 = operands(M, N, K)
    rms = K >= 1024
    checked(f"restatement {M}x{N}x{K}", C.restate(a64, w64), a, w, a64, w64, rms=rms, out=print)
    checked("reversed K", C.restate(a64, w64, reverse=True), a, w, a64, w64, rms=rms)
    checked("128-step grouping", C.restate(a64, w64, group=128), a, w, a64, w64, rms=rms)
    checked("four K slices", C.epilogue32(B.accumulate_slices(a64, w64)), a, w, a64, w64, rms=rms)
    checked("skinny's 16 K ranges", C.epilogue32(B.accumulate_skinny(a64, w64)), a, w, a64, w64, rms=rms)
    if K <= 3072:
        checked("sequential fp32", C.epilogue32(B.accumulate_sequential(a64, w64)), a, w, a64, w64, rms=rms)


@pytest.mark.parametrize("K", [1024, 3072, 12288])
def test_the_restatement_orders_lie_within_the_rms_factor_of_each_other(K):
    """Bar (e) takes 1.25 x the LARGEST rms of three orders: that is a bar only if the orders themselves agree that well, per
    family of at least 1000 elements, at the K lengths the GPU matrix asserts it (1024: split-K 1 and the row split; 3072:
    split-K 2 and 130 x 128 x 3072; 12288: 130 x 128 x 12288, whose ``mixed`` family alone has 1000 elements) -- here at
    300 x 264, where every family has that many."""
    a, w, a64, w64 = operands(300, 264, K)
    y, S = C.reference(a64, w64)
    fam = B.family_of(a, w, a64, w64)
    figs = [C.figures(r, y, S, K, fam, T=B.underflow_term(K), families=B.FAMILIES) for r in B.rms_orders(a64, w64)]
    seen = 0
    for f in figs[0]:
        if figs[0][f]["n"] >= C.RMS_MIN_N and f not in B.EXACT:
            r = [g[f]["rms"] for g in figs]
            print(f"K = {K} {f}: rms {r}")
            assert max(r) <= C.RMS_FACTOR * min(r), (f, r)
            seen += 1
    assert seen >= 4


def test_restatement_passes_under_every_epilogue_and_activation():
    M, N, K = B.EPI_SHAPE
    for which in B.EPILOGUES:
        batch = 2 if which == "batch2" else 1
        a, w, a64, w64 = operands(M, N, K, "mid", batch)
        e = B.epilogue_of(M, N, K, "mid", which, "gelu_tanh" if which == "gelu" else None, batch)
        checked(which, C.restate(a64, w64, e, M), a, w, a64, w64, e, M, out=print)
    a, w, a64, w64 = operands(M, N, 64)
    e = B.epilogue_of(M, N, 64, "mid", "res-cancel", None)
    checked("res-cancel K = 64", C.restate(a64, w64, e, M), a, w, a64, w64, e, M, out=print)
    a, w, a64, w64 = operands(M, N, K, "act-range")
    for act in B.SKINNY_ACTS:
        e = B.epilogue_of(M, N, K, "act-range", None, act)
        checked(f"act-range {act}", C.restate(a64, w64, e, M), a, w, a64, w64, e, M, out=print)


def test_activation_slopes_are_the_ones_the_docstring_derives():
    x = torch.linspace(-12, 12, 240001, dtype=torch.float64)
    h = x[1] - x[0]
    for act, bound in C.ACT_SLOPE.items():
        f = C.ACT64[act](x)
        d1 = (f[2:] - f[:-2]) / (2 * h)
        d2 = (f[2:] - 2 * f[1:-1] + f[:-2]) / (h * h)
        assert bound - 0.005 < float(d1.abs().max()) <= bound, (act, float(d1.abs().max()))
        assert float(d2.abs().max()) < 1.0, (act, float(d2.abs().max()))


# ------------------------------------------------------------------------------------------------------------ planted faults
def epilogue32_with(acc, e, M, fault):
    """``cond_gemm.epilogue32`` with one planted fault."""
    rows = acc.shape[0]
    r16 = lambda t: t.to(BF).float()
    v = acc
    if e["bias"] is not None:
        rs = 1.0 if e["rowscale"] is None else e["rowscale"].double()[:, None]
        add = rs * e["bias"].double()[None]
        v = (acc.double() + (add.to(BF).double() if fault == "rowscale * bias in bf16" else add)).float()
    if e["act"] is not None:
        if fault == "tanh argument clamped":
            u = (0.7978845608028654 * (v + 0.044715 * v * v * v)).clamp(-5.0, 5.0)
            v = 0.5 * v * (1.0 + torch.tanh(u))
        else:
            v = C.ACT64[e["act"]](v)
    g0, g1 = (e["gate1"], e["gate0"]) if fault == "gates swapped" else (e["gate0"], e["gate1"])
    g = C._gate({**e, "gate0": g0, "gate1": g1}, rows, M or rows, torch.float32)
    if fault == "rounded before the gate":
        v = r16(v)
    if fault == "gate * alpha in bf16":
        v = v * r16(g * e["alpha"])
    else:
        if e["alpha"] != 1.0:
            v = v * e["alpha"]
        if g is not None:
            v = v * g
    if e["res"] is not None:
        v = (r16(v) if fault == "rounded before the residual" else v) + e["res"].float()
    if fault == "truncated":
        return (v.contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF)
    return v.to(BF)


def accumulate_bf16_per_ktile(a64, w64):
    acc = torch.zeros(a64.shape[0], w64.shape[0], dtype=torch.float32)
    for k0 in range(0, a64.shape[1], 64):
        acc = (acc + (a64[:, k0:k0 + 64] @ w64[:, k0:k0 + 64].T).float()).to(BF).float()
    return acc


def rejected(name, bar, got, a, w, a64, w64, e=C.NO_EPILOGUE, M=None, **kw):
    """The fault fails ``check`` as the GPU file applies it, and (``bar`` given) the bar named for it is among those that say so."""
    with pytest.raises(AssertionError) as err:
        checked(name, got, a, w, a64, w64, e, M, **kw)
    msg = str(err.value)
    print(f"{name}: {msg[:260]}")
    for b in ([bar] if isinstance(bar, str) else bar or []):
        assert b in msg, (name, b, msg[:400])


BAR_A, BAR_C, BAR_E, BAR_EXACT = "+ eps =", "mean signed error", "rms error", "exact family"


def test_planted_accumulator_and_input_faults_are_rejected():
    M, N, K = FAULT_SHAPE
    a, w, a64, w64 = operands(M, N, K)
    base = C.accumulate32(a64, w64)
    checked("clean", C.epilogue32(base), a, w, a64, w64)
    # a K-tile of 64 dropped in one 16 x 16 tile
    a2 = a64.clone()
    a2[16:32, 256:320] = 0
    acc = base.clone()
    acc[16:32, 32:48] = C.accumulate32(a2, w64)[16:32, 32:48]
    rejected("a K-tile dropped in one 16 x 16 tile", None, C.epilogue32(acc), a, w, a64, w64)
    # the accumulator rounded to bf16 once per 64-step K-tile: bar (a) at K <= 512 ...
    rejected("bf16 accumulator per K-tile", BAR_A, C.epilogue32(accumulate_bf16_per_ktile(a64, w64)), a, w, a64, w64)
    b, x, b64, x64 = operands(M, N, 192)          # (at K = 64 there is one K-tile: the rounding is the final one)
    rejected("bf16 accumulator per K-tile, K = 192", BAR_A, C.epilogue32(accumulate_bf16_per_ktile(b64, x64)), b, x, b64, x64)
    # ... and bar (e) at K = 3072, where eps has grown past the damage on most elements
    b, x, b64, x64 = operands(300, 264, 3072)
    rejected("bf16 accumulator per K-tile, K = 3072", BAR_E, C.epilogue32(accumulate_bf16_per_ktile(b64, x64)), b, x, b64, x64, rms=True)
    # bf16 subnormal inputs flushed to zero: the subnormal family, and one-hot
    flush = lambda op: {**op, "bits": torch.where((op["bits"] & 0x7F80) == 0, op["bits"] & -32768, op["bits"])}
    rejected("subnormal inputs flushed", BAR_EXACT + ", share 1.0", C.restate(B.values(flush(a)), B.values(flush(w))), a, w, a64, w64)
    oa, ow, oa64, ow64 = operands(*B.ONE_HOT_SHAPE, "one-hot")
    rejected("subnormal inputs flushed, one-hot", "one-hot: " + BAR_EXACT, C.restate(B.values(flush(oa)), ow64), oa, ow, oa64, ow64)
    # the top code decoded as infinity
    top = {**a, "bits": a["bits"].clone()}
    inf = a64.clone()
    inf[a64.abs() == 255 * 2.0 ** 120] = float("inf")
    rejected("the top code decoded as infinity", "extreme: a result is not finite", C.restate(inf, w64), top, w, a64, w64)
    inf1 = oa64.clone()
    inf1[oa64.abs() == 255 * 2.0 ** 120] = float("inf")
    rejected("the top code decoded as infinity, one-hot", "one-hot: a result is not finite", C.restate(inf1, ow64), oa, ow, oa64, ow64)


def test_planted_epilogue_faults_are_rejected():
    M, N, K = FAULT_SHAPE
    a, w, a64, w64 = operands(M, N, K)
    acc = C.accumulate32(a64, w64)
    full = C.make_epilogue(M, N, 11, bias=True, gates=True, res=True, rowscale=True, alpha=0.5)
    odd = C.make_epilogue(M, N, 12, gates=True, alpha=0.3)
    for e in (full, odd):
        checked("clean", epilogue32_with(acc, e, M, None), a, w, a64, w64, e, M)
        assert torch.equal(epilogue32_with(acc, e, M, None).view(torch.int16), C.epilogue32(acc, e, M).view(torch.int16))
    rejected("rounded before the gate", BAR_A, epilogue32_with(acc, odd, M, "rounded before the gate"), a, w, a64, w64, odd, M)
    rejected("gate * alpha in bf16", BAR_A, epilogue32_with(acc, odd, M, "gate * alpha in bf16"), a, w, a64, w64, odd, M)
    rejected("rowscale * bias in bf16", BAR_A, epilogue32_with(acc, full, M, "rowscale * bias in bf16"), a, w, a64, w64, full, M)
    rejected("gates swapped", BAR_A, epilogue32_with(acc, full, M, "gates swapped"), a, w, a64, w64, full, M)
    # truncation instead of round-to-nearest-even at the final conversion: up to one ulp, (a); it is toward zero, so over results
    # of both signs the two halves' signed means cancel and (c) is silent -- over the positive results alone (c) names it too
    trunc = epilogue32_with(acc, C.NO_EPILOGUE, M, "truncated")
    rejected("truncated", BAR_A, trunc, a, w, a64, w64, exact=())
    rejected("truncated, positive results", BAR_C, trunc, a, w, a64, w64, exact=(), keep=lambda y: y > 0)
    checked("clean, positive results", C.epilogue32(acc), a, w, a64, w64, exact=(), keep=lambda y: y > 0)
    # the value rounded to bf16 before the residual add: (a) on res-cancel at K = 64
    b, x, b64, x64 = operands(M, N, 64)
    e = B.epilogue_of(M, N, 64, "mid", "res-cancel", None)
    acc64 = C.accumulate32(b64, x64)
    checked("clean", epilogue32_with(acc64, e, M, None), b, x, b64, x64, e, M)
    rejected("rounded before the residual", BAR_A, epilogue32_with(acc64, e, M, "rounded before the residual"), b, x, b64, x64, e, M)
    # GELU with its tanh argument clamped to [-5, 5]: act-range (pre-activations below -8 come out as -0.5 x 9e-5 x, not 0)
    b, x, b64, x64 = operands(M, N, K, "act-range")
    e = B.epilogue_of(M, N, K, "act-range", None, "gelu_tanh")
    accr = C.accumulate32(b64, x64)
    checked("clean", epilogue32_with(accr, e, M, None), b, x, b64, x64, e, M)
    rejected("tanh argument clamped", "act-range: e ", epilogue32_with(accr, e, M, "tanh argument clamped"), b, x, b64, x64, e, M)


# --------------------------------------------------------------------------------------------------------------- plan coverage
@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import build
    build.build_hip_library()
    from bind_your_avatar_implementation_amd import ops
    return ops


def test_the_gpu_matrix_reaches_every_bf16_path_on_meta_tensors(ops):
    """Each case of the GPU tables gets the plan key it asserts (split-K needs a device's workspace: without one its cases plan
    the unsplit P256, and the key they assert on the GPU is "p256+splitk"); together they reach every key of ops.GEMM_PATHS,
    split-K, and a row split with m0 > 0."""
    seen = set()
    for c in B.tiled_cases():
        A, W, out, kw = B.launch_args("meta", c)
        with ops.options(**c["opts"]):
            plan = ops.gemm_plan(A, W, out.view(), **kw)
        want = "p256" if c["key"] == "p256+splitk" else c["key"]
        assert ops.plan_key(plan) == want and plan["row_chunks"] == 1, (c["id"], plan)
        if c["key"] == B.ROW_SPLIT_KEY:
            assert 0 < plan["m0"] < c["M"] and (c["M"] - plan["m0"]) > 128 and plan["m0"] > 128
        seen.add(c["key"])
    assert seen == set(ops.GEMM_PATHS.values()) | {"p256+splitk", B.ROW_SPLIT_KEY}, sorted(seen)
    for p in B.PATHS:                       # every path: every K length, one-hot, every epilogue, GELU on act-range
        mine = [c for c in B.tiled_cases() if c["key"] == p]
        assert {c["K"] for c in mine if c["group"] == "mid" and not c["which"]} >= set(B.PATHS[p][4])
        assert {c["group"] for c in mine} >= {"mid", "one-hot", "one-hot-neg", "act-range"}
        assert {c["which"] for c in mine} >= set(B.EPILOGUES)
    assert {c["act"] for c in B.activation_cases() if c["key"] == "t128x128"} == {"gelu_tanh", *B.ACTS_T128}
    for c in B.skinny_cases():
        cc = dict(M=c["M"], N=B.SKINNY_N, K=c["K"], batch=c["B"], parts=1, col0=8, alias=False, which=None, act=c["act"])
        A, W, out, kw = B.launch_args("meta", cc)
        with ops.weight_streaming():
            assert ops.gemm_plan(A, W, out.view(), **kw)["path"] == "skinny", c["id"]
    assert {c["act"] for c in B.skinny_cases()} == {None, *B.SKINNY_ACTS}
    for M, N, form in B.ROWGEMM:
        for mode in B.ROWGEMM_MODES:
            plan = ops.rowgemm512_plan(M, N, ln=False, res=True if mode == "res" else None, act="gelu_erf" if mode == "gelu_erf" else None)
            assert plan["form"] == form and not plan["ln"], (M, N, mode, plan)
    assert {f for _, _, f in B.ROWGEMM} == set(ops._hip.ROWGEMM_FORMS.values())


def test_the_row_split_shape_is_the_smallest_the_plan_query_splits(ops):
    """Under the default options, over 256 x 256 tile grids of up to 520 tiles (M one past a multiple of 256, N eight past one),
    at K = 512 and 1024: no launch with fewer output elements than ROW_SPLIT_SHAPE has m0 > 0."""
    m = lambda *s: torch.empty(*s, dtype=BF, device="meta")
    M0, N0, K0 = B.ROW_SPLIT_SHAPE
    assert ops.gemm_plan(m(M0, K0), m(N0, K0), m(M0, N0))["m0"] > 0
    for K in (512, 1024):
        for tn in range(1, 261):
            for tm in range(2, 521 // tn + 1):
                M, N = (tm - 1) * 256 + 1, (tn - 1) * 256 + 8
                if tm * tn <= 256 or M * N >= M0 * N0:
                    continue
                assert ops.gemm_plan(m(M, K), m(N, K), m(M, N))["m0"] == 0, (M, N, K)
