"""CPU: the exact-data norm tests' own conditions (tests/exact_norm.py; the GPU file imports the same case lists): the exact
mean / variance identities, y != 0 and at most 8 significant bits on every element, the kernels' fp32 expressions with rstd +- 2
ulps, the fp8 / MX exactness conditions; that the case lists reach every template instance and branch of csrc/norm.hip, asserted
from the host-side plan queries and the wave models; and planted faults on the fp64 reference that the exact check must catch --
with, for the scale faults, what the old relative-Frobenius bar scores on the old random data."""
import pytest
import torch
import torch.nn.functional as F

import exact_norm as xn
from conftest import rel_fro
from exact_norm import BF, GuardedOut


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    from bind_your_avatar_implementation_amd import ops
    return ops


def test_mean_and_variance_identities_hold_in_fp32():
    xn.assert_mean_var_identities()
    # sums of D small integers are exact in fp32 in any order: the largest partial sum is below 2^24
    assert max(xn.WIDTHS) * 12 ** 2 < 2 ** 24


@pytest.mark.parametrize("c", xn.LN_CASES, ids=lambda c: c["name"])
def test_layernorm_case_data_conditions(c):
    xn.assert_ln_conditions(c, xn.ln_data(c))


@pytest.mark.parametrize("c", xn.QK_CASES, ids=lambda c: c["name"])
def test_qknorm_case_data_conditions(c):
    xn.assert_qk_conditions(c, xn.qk_data(c))


def test_modulation_sets_differ_on_every_element():
    """The sets of one batch entry and of different batch entries: the wrong one changes every element."""
    c = next(c for c in xn.ROWS_CASES if c["batch"] == 2 and c["form"] == "wbmod" and c["rows"] == 5)
    dat = xn.ln_data(c)
    rows = torch.arange(c["rows"] * c["batch"])
    own = xn.row_sets(c)
    for shift in (1, 2, 3):
        other = xn.closed_form(c, dat, sets=(own + shift) % 4, rows=rows)
        assert bool((other.to(BF) != xn.closed_form(c, dat).to(BF)).all())


def _ln_plan(ops, c):
    x = xn.strided(torch.empty(c["batch"], c["rows"], c["D"], dtype=BF, device="meta"), 40)
    x = x if c["batch"] > 1 else x[0]
    p = lambda present: True if present else None
    kw = dict(weight=p(c["form"] in ("w", "wb", "wbmod", "quant")), bias=p(c["form"] in ("wb", "wbmod", "quant")))
    if xn.modulated(c):
        kw.update(shift0=True, scale0=True, shift1=True, scale1=True, mod_batch_stride=2 * c["D"])
    if c["out"] == "bf16":
        out = GuardedOut(c["rows"], c["D"], "meta", batch=c["batch"]).view()
    else:
        rb = c["D"] * (6 if c["out"] == "mxfp6" else 8) // 8
        out = torch.empty(c["batch"], c["rows"] + 8, rb + 64, dtype=torch.uint8, device="meta")[:, 3:3 + c["rows"], 8:8 + rb]
    with ops.options(reference_forms="ln_generic" if c["generic_form"] else []):
        return ops.layernorm_plan(x, out, split=c["split"], out_kind=c["out"], **kw)


def test_layernorm_cases_reach_every_instance_branch_and_event(ops):
    instances, forms, rpws, events = set(), set(), set(), set()
    for c in xn.LN_CASES:
        plan = _ln_plan(ops, c)
        vec, nv = xn.VEC_NV[c["D"]]
        assert (plan["kernel"], plan["rows_per_wave"], plan["vec"], plan["nv"], plan["modulated"]) == \
            (c["kernel"], c["rpw"], vec, nv, xn.modulated(c)), (c["name"], plan)
        total = c["rows"] * c["batch"]
        assert plan["waves"] == -(-total // c["rpw"]) and plan["grid"] == -(-plan["waves"] // 4)
        instances.add(xn.ln_instance(c))
        if plan["kernel"] == "generic" and c["out"] == "bf16":
            forms.add((c["form"], c["D"]))
        else:
            rpws.add(plan["rows_per_wave"])
        got = xn.ln_events(c, plan)
        assert c["events"] <= got, (c["name"], c["events"], got)
        events |= got
    assert instances == xn.LN_INSTANCES, instances ^ xn.LN_INSTANCES
    # every parameter-form branch of layernorm_kernel at every width: none, w without b, w + b, modulation without affine, the
    # A / B fma; <8, 6> with w + b through the reference form
    assert {(f, D) for f in xn.FORMS for D in xn.WIDTHS} <= forms
    assert any(c["generic_form"] and c["form"] == "wb" for c in xn.GENERIC_CASES)
    assert {2, 3, 4} <= rpws
    assert {"crosses_split", "crosses_batch", "crosses_batch_same_side", "clipped"} <= events
    # the workload's case meets all three in one launch, and the partial last workgroup is reached
    big = next(c for c in xn.ROWS_CASES if c["rows"] == 4099 and c["form"] == "wbmod")
    assert {"crosses_split", "crosses_batch", "clipped"} <= xn.ln_events(big, _ln_plan(ops, big))
    assert any((c["rows"] * c["batch"]) % 4 for c in xn.GENERIC_CASES)
    assert {c["rows"] for c in xn.GENERIC_CASES} >= set(xn.ROW_COUNTS)
    assert all(any(c["eps"] and c["D"] == D for c in xn.GENERIC_CASES) for D in xn.WIDTHS)


def test_rows_wave_model():
    """4099 rows x 2, split 226, three rows per wave: wave 75 crosses the split of entry 0 (rows 225 .. 227), wave 1366 the batch
    boundary (4098, then rows 0, 1 of entry 1), the last wave is clipped."""
    w = xn.rows_waves(4099, 2, 226, 3)
    assert len(w) == 2733 and w[75] == (225, 228, True, False, False) and w[1366] == (4098, 4101, False, True, False)
    assert w[-1] == (8196, 8198, False, False, True)
    assert sum(1 for t in w if t[2]) == 2                               # the split of each batch entry
    assert w[(4099 + 226) // 3][2]                                      # rows 4323 .. 4325 hold row 226 of entry 1
    # all rows on one side: the batch boundary is crossed, the side is not
    for split in (0, 5):
        w = xn.rows_waves(5, 2, split, 2)
        assert [t[2] for t in w] == [False] * 5 and [t[3] for t in w] == [False, False, True, False, False]


def test_qknorm_cases_reach_both_instances_every_only_and_the_straddles(ops):
    onlys, stats = set(), set()
    for c in xn.QK_CASES:
        W = c["heads"] * 64
        buf = torch.empty(c["batch"], c["S"] + 3, 3 * W, dtype=BF, device="meta")
        q, k = buf[:, :c["S"], :W], buf[:, :c["S"], W:2 * W]
        plan = ops.qknorm_rope_plan(None if c["only"] == 2 else q, None if c["only"] == 1 else k, c["heads"], c["text_rows"],
                                    cos=None if c["text_rows"] == c["S"] else True, stats=c["slots"] or None)
        pairs = c["batch"] * c["S"] * c["heads"] * (1 if c["only"] else 2)
        assert plan == {"stats": bool(c["slots"]), "only": c["only"], "slots": c["slots"], "pairs": pairs, "waves": -(-pairs // 8),
                        "grid": -(-pairs // 32)}, (c["name"], plan)
        assert c["events"] <= xn.qk_waves(c), (c["name"], c["events"], xn.qk_waves(c))
        onlys.add(c["only"])
        stats.add(plan["stats"])
    assert onlys == {0, 1, 2} and stats == {False, True}
    assert {c["heads"] for c in xn.QK_CASES} == {1, 3, 6, 8, 48} and {c["batch"] for c in xn.QK_CASES} == {1, 2}
    assert {c["slots"] for c in xn.QK_CASES} >= {1, 8, 64}
    for H in (3, 6):                                                     # not a multiple of 8: every straddle, in a joint call
        assert any(c["heads"] == H and not c["only"] and {"straddles_row", "straddles_batch", "straddles_qk"} <= xn.qk_waves(c)
                   for c in xn.QK_CASES)
        assert {c["only"] for c in xn.QK_CASES if c["heads"] == H} == {0, 1, 2}
    kinds = {("0" if c["text_rows"] == 0 else "S" if c["text_rows"] == c["S"] else "inside") for c in xn.QK_CASES}
    assert kinds == {"0", "inside", "S"}
    assert any(c["slots"] and -(-c["batch"] * c["S"] * c["heads"] * 2 // 32) < c["slots"] for c in xn.QK_CASES)     # slots never reached


def test_plan_queries_validate_like_the_launchers(ops):
    from bind_your_avatar_implementation_amd import _hip
    x = torch.empty(300, 3072, dtype=BF, device="meta")
    assert ops.layernorm_plan(x, x, True, True)["kernel"] == "rows" and ops.layernorm_plan(x, x, True)["kernel"] == "generic"
    with ops.options(reference_forms="ln_generic"):
        assert ops.layernorm_plan(x, x, True, True)["kernel"] == "generic"
    assert ops.layernorm_plan(torch.empty(2, 8193, 3072, dtype=BF, device="meta"), torch.empty(2, 8193, 3072, dtype=BF, device="meta"),
                              True, True)["rows_per_wave"] == 5
    with pytest.raises(_hip.ByaError, match="UNSUPPORTED"):
        ops.layernorm_plan(x[:, :640], x[:, :640])
    with pytest.raises(_hip.ByaError, match="ALIGN"):
        ops.layernorm_plan(x, x[:, 4:][:, :3064].as_strided((300, 3072), (3072, 1), 4))
    with pytest.raises(_hip.ByaError, match="UNSUPPORTED"):             # the quantised forms exist at the DiT width only
        ops.layernorm_plan(x[:, :512], torch.empty(300, 512, dtype=torch.uint8, device="meta"), out_kind="fp8")
    with pytest.raises(_hip.ByaError, match="SHAPE"):                   # an MX row must hold its code bytes
        ops.layernorm_plan(x, torch.empty(300, 2296, dtype=torch.uint8, device="meta"), out_kind="mxfp6")
    q = torch.empty(2, 7, 3 * 384, dtype=BF, device="meta")
    with pytest.raises(_hip.ByaError, match="SHAPE"):
        ops.qknorm_rope_plan(q[..., :384], q[..., 384:768], 6, 3, cos=None)     # rows to rotate, no tables
    with pytest.raises(_hip.ByaError, match="SHAPE"):
        ops.qknorm_rope_plan(q[..., :384], None, 6, 3, stats=65)


# ------------------------------------------------------------------------------------------------------------ planted faults
def _caught(ref_fault, ref):
    return bool(xn.bad_elements(ref_fault.to(BF), ref.to(BF)).any())


def _old_ln_scores():
    """The data of test_kernels_gpu.test_layernorm_affine at D = 3072 and what its bar (relative Frobenius error against the
    fp32 reference rounded to bf16, <= 1e-3) scores for the three scale faults."""
    D = 3072

    def rnd(shape, seed, std=1.0):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(shape, generator=g) * std).to(BF)

    x = rnd((333, D), 60, 2.0) + 0.5
    w, b = rnd((D,), 61, 0.2) + 1, rnd((D,), 62, 0.2)
    ref = F.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-5).to(BF).float()

    def score(eps, var_div=D):
        xf = x.float()
        mean = xf.mean(-1, keepdim=True)
        var = ((xf - mean) ** 2).sum(-1, keepdim=True) / var_div
        y = (xf - mean) * torch.rsqrt(var + eps) * w.float() + b.float()
        return rel_fro(y.to(BF).float(), ref)

    return {"exact": score(1e-5), "var_div": score(1e-5, D - 1), "eps_dropped": score(0.0), "eps_x100": score(1e-3)}


def test_planted_scale_faults_pass_the_old_bar_and_fail_the_exact_check():
    old = _old_ln_scores()
    print("old bar (1e-3) on the data of test_layernorm_affine, D = 3072:", {k: f"{v:.2e}" for k, v in old.items()})
    assert old["exact"] < 1e-4
    # variance / (D - 1): the variance-sensitive rows of every width catch it; the grid rows alone do not at D = 3072
    for c in (c for c in xn.GENERIC_CASES if c["form"] == "sens"):
        dat = xn.ln_data(c)
        assert _caught(xn.ln_reference_case(c, dat, var_div=c["D"] - 1), xn.ln_reference_case(c, dat)), c["name"]
    assert old["var_div"] <= 1e-3, old
    # eps dropped, a hundred times too large, 1e-5 or 1e-6 in place of the caller's: wrong by a factor on the eps = 3 rows
    eps_cases = [c for c in xn.LN_CASES if c["eps"]]
    assert {c["D"] for c in eps_cases} == set(xn.WIDTHS) and {c["kernel"] for c in eps_cases} == {"generic", "rows"}
    for c in eps_cases:
        dat = xn.ln_data(c)
        ref = xn.ln_reference_case(c, dat)
        for eps in (0.0, 300.0, 1e-5, 1e-6):
            bad = xn.bad_elements(xn.ln_reference_case(c, dat, eps=eps).to(BF), ref.to(BF))
            assert float(bad.double().mean()) > 0.5, (c["name"], eps)   # every element whose pattern value is not 0
    assert old["eps_dropped"] <= 1e-3 and old["eps_x100"] <= 1e-3, old


def test_planted_qknorm_scale_faults():
    """The 64-wide q/k norm: eps dropped and the LayerNorm's 1e-5 in place of 1e-6 pass the old bar on random data and fail the
    exact check on the eps = 3 rows; variance / 63 fails it on every case (a cancelling b makes 1 / 126 visible)."""
    g = torch.Generator().manual_seed(70)
    x = torch.randn(2, 56, 48 * 64, generator=g).to(BF)
    w = (torch.randn(64, generator=g) * 0.3 + 1).to(BF)
    b = (torch.randn(64, generator=g) * 0.3).to(BF)
    old = lambda eps: xn.qk_reference64(x, w, b, None, None, 56, eps).float().to(BF).float()
    scores = {"eps_dropped": rel_fro(old(0.0), old(1e-6)), "eps_1e-5": rel_fro(old(1e-5), old(1e-6))}
    print("old bar (1e-3) on random q/k rows:", {k: f"{v:.2e}" for k, v in scores.items()})
    assert max(scores.values()) <= 1e-3
    for c in xn.QK_CASES:
        dat = xn.qk_data(c)
        q, k = xn.qk_reference_case(c, dat)
        for which, r in enumerate(xn.qk_reference_case(c, dat, var_div=63)):
            if not c["only"] or c["only"] - 1 == which:
                assert _caught(r, (q, k)[which]), c["name"]
        if c["eps"]:
            for eps in (0.0, 1e-5, 1e-6):
                for r, good in zip(xn.qk_reference_case(c, dat, eps=eps), (q, k)):
                    assert float(xn.bad_elements(r.to(BF), good.to(BF)).double().mean()) > 0.9, (c["name"], eps)
    assert any(c["eps"] for c in xn.QK_CASES)


def test_planted_index_faults_fail_the_exact_check():
    # the parameter set keyed by the side alone (batch entry 1 reads entry 0's vectors): every element of entry 1
    for c in (c for c in xn.LN_CASES if c["batch"] == 2 and xn.modulated(c) and c["form"] != "sens"):
        dat = xn.ln_data(c)
        rows = xn.distinct_rows(c, dat)
        bad = xn.bad_elements(xn.ln_reference_case(c, dat, rows=rows, side_only=True).to(BF), xn.ln_reference_case(c, dat, rows=rows).to(BF))
        z1 = rows >= c["rows"]
        assert bool(z1.any()) and not bool(bad[~z1].any()), c["name"]
        assert bool(bad[z1].all()) if c["form"] != "quant" else float(bad[z1].double().mean()) > 0.5, c["name"]
    # the last row of a clipped range skipped: its elements keep the poison, which equals no reference value
    for c in (c for c in xn.ROWS_CASES if "clipped" in c["events"]):
        total = c["rows"] * c["batch"]
        r0, r1, _, _, clipped = xn.rows_waves(c["rows"], c["batch"], c["split"], c["rpw"])[-1]
        assert clipped and r1 == total
        dat = xn.ln_data(c)
        ref = xn.ln_reference_case(c, dat, rows=torch.tensor([total - 1])).to(BF)
        got = torch.full_like(ref.view(torch.int16), xn.POISON).view(BF)
        assert bool(xn.bad_elements(got, ref).all())
    # cos[e] read for element e + 1; k_scale applied to q
    rotated = [c for c in xn.QK_CASES if c["text_rows"] < c["S"]]
    for c in rotated:
        dat = xn.qk_data(c)
        good = xn.qk_reference_case(c, dat)
        for r, g in zip(xn.qk_reference_case(c, dat, cos_shift=True), good):
            assert _caught(r, g), c["name"]
    scaled = [c for c in xn.QK_CASES if c["k_scale"] != 1.0 and c["only"] != 2]
    assert scaled
    for c in scaled:
        dat = xn.qk_data(c)
        q_bad, _ = xn.qk_reference_case(c, dat, q_scale=c["k_scale"])
        assert bool(xn.bad_elements(q_bad.to(BF), xn.qk_reference_case(c, dat)[0].to(BF)).all()), c["name"]


def test_fp8_definition_moved_here_is_the_one_the_quantiser_test_uses():
    import test_fp8_gpu
    assert test_fp8_gpu.quant_ref is xn.quant_rows_fp8_ref
