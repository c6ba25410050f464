"""CPU side of the attention conditioning tests (tests/cond_attn.py): (1) every case of the GPU matrix holds every family its path
admits, and the rows are what they claim: the realised score ranges, the static kinds inside their bound; (2) the fp32 terms eps of
the per-element bar stay <= 0.5 at every case; (3) the restatement and two correct variants of it (tiled online softmax with the
lazy-rescale threshold and the two-term bf16 reference point; no offset at all on the static kinds) pass the per-element bar and
carry no bias at the suite's own shapes; (4) planted faults in plain torch fail one of the two bars on the families they touch,
most of them under the relative-Frobenius bar of the random-data tests; (5) the GPU matrix reaches every attention plan the exact
suite reaches, the 17776-row shapes apart."""
import functools

import pytest
import torch

import cond_attn as C
import exact_attn as X
from cond_attn import BF, FAMILIES
from conftest import rel_fro

ATTN_TOL = 3e-3            # the bar of tests/test_kernels_gpu.py
CORRECT_BIAS, PLANTED_BIAS = 0.1, 0.5
ALL_CASES = ([("attn", c) for c in C.ATTN_CASES] + [("mix", c) for c in C.MIX_CASES] + [("tiny", c) for c in C.TINY_CASES])
IDS = [f"{p}-{c['name']}" for p, c in ALL_CASES]


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    ops._hip.load()
    return ops


def _path(p, c):
    return c["kind"] if p == "attn" else p


def _data(p, c):
    if p == "attn":
        return C.attn_case_data(c)
    return C.mix_case_data(c) if p == "mix" else C.tiny_case_data(c)[0]


def _sample(d, max_scores=3e7):
    """(q, k, v, fam, factor) per key/value variant; where the case has more than ``max_scores`` scores: 8 (batch, head)s -- even
    and odd ones, i.e. both row layouts -- with 8 consecutive 32-row blocks each, 2048 rows."""
    q, k, v, fam = C.per_variant(d)
    nkv = d["k"].shape[1]
    factor = d["factor"].repeat_interleave(nkv)
    n, Sq, _ = q.shape
    if n * Sq * k.shape[1] <= max_scores:
        return q, k, v, fam, factor
    heads = torch.arange(0, n, max(1, n // 8))[:8]
    nblk = -(-Sq // 32)
    r0 = torch.tensor([(int(h) * 3 % max(1, nblk - 8)) * 32 for h in heads])
    rows = r0[:, None] + torch.arange(256)[None]
    pick = lambda t: torch.stack([t[h, rows[i]] for i, h in enumerate(heads)])
    return pick(q), k[heads], v[heads], pick(fam), factor[heads]


@functools.lru_cache(maxsize=None)
def _extremes(p, name):
    """(S_abs, max |s|) over ALL pairs of the case, in fp32."""
    c = next(c for pp, c in ALL_CASES if pp == p and c["name"] == name)
    q, k, _, _ = C.per_variant(_data(p, c))
    worst = 0.0
    for a, b, r0, r1 in C._row_chunks(q.shape[0], q.shape[1], k.shape[1]):
        worst = max(worst, float((q[a:b, r0:r1] @ k[a:b].transpose(1, 2)).abs().max()))
    return C.s_abs(q, k), worst


# ------------------------------------------------------------------------------------------------ (1) families and ranges
@pytest.mark.parametrize("p,c", ALL_CASES, ids=IDS)
def test_every_case_holds_every_family_and_the_rows_are_what_they_claim(p, c):
    d = _data(p, c)
    fams = C.families_of(_path(p, c))
    Sq, Skv, D = d["q"].shape[1], d["k"].shape[2], d["q"].shape[2]
    present = {FAMILIES[i] for i in d["fam"].unique().tolist()}
    assert present == set(fams) == set(d["fams"]), (sorted(present), fams)
    if Sq >= len(fams):                                             # every (batch, head) then holds every family
        for bh in range(d["q"].shape[0]):
            assert len(d["fam"][bh].unique()) == len(fams), bh
    assert bool(d["blocked"].any()) == (Sq >= 32 * len(fams) and d["q"].shape[0] > 1)
    for t in (d["q"], d["k"], d["v"]):
        assert torch.equal(t.to(BF).float(), t)
    assert bool((d["v"][..., :D // 2] >= 1).all())
    static = _path(p, c) in C.STATIC_KINDS
    assert d["static"] == static
    if p == "attn" and c["kind"] == "w4":
        assert _extremes(p, c["name"])[1] <= 85.0 < X.BOUND
    if p == "attn" and c["kind"] == "dev":
        stats, B = C.device_bound_stats(d, c["B"], c["H"], "cpu")
        assert bool((stats[:, :, :2] == 0).all()) and stats.shape[2] == B.numel() + 5
        high = (torch.arange(B.numel()) % c["H"]) % 2 == 1
        assert c["Sq"] == 1 or bool((B > 0).all())                   # (a head whose only row is the flat one has q = 0 and B = 0)
        high, B = high[B > 0], B[B > 0]
        assert bool((B[~high] <= 85.5).all()) and bool((B[~high] >= 75).all()) and bool((B[high] >= 99.5).all()) and bool((B[high] <= 115).all()), B
        assert bool(high.any()) and not bool(high.all()) and _extremes(p, c["name"])[1] <= float(B.max())

    q, k, v, fam, factor = _sample(d)
    s = (q.double() @ k.double().transpose(1, 2)) / factor[:, None, None]          # the device bound's scaling of q taken out
    nt = -(-Skv // 64)
    tmax = torch.stack([s[..., t0:t0 + 64].amax(-1) for t0 in range(0, Skv, 64)], -1)     # [n, rows, nt]
    lo, hi = s.amin(-1), s.amax(-1)
    sel = lambda name: fam == FAMILIES.index(name)
    tol = 6 * C.STRUCT_SD + 1.0                                    # six sd of the noise, and the bf16 rounding of q, k (<= 2^-8 * 300)
    if static:                                                      # (dev: before q is scaled; its peak is 120 there, 40 after)
        assert float(s[~sel("peaked")].abs().max()) <= 85.0 and float((s * factor[:, None, None]).abs().max()) <= 85.0 * 100 / 85
    m = sel("friendly")
    assert 1.5 <= float(s[m].std()) <= 4.5 and float(s[m].abs().max()) <= 25
    assert bool((s[sel("flat")] == 0).all())
    m = sel("peaked")
    top2 = (s * factor[:, None, None])[m].topk(min(2, Skv), -1).values       # (as the kernel sees them: cond_attn.DEV_PEAK)
    if Skv > 1:
        assert float((top2[:, 0] - top2[:, 1]).min()) >= 30.0
    for name, sign in (("shift-low", -1), ("shift-high", 1)):
        m = sel(name)
        assert float((sign * s[m]).min()) >= C.SHIFT - C.SPREAD - tol and float((sign * s[m]).max()) <= C.SHIFT + C.SPREAD + tol
        if Skv > 1:
            assert float((sign * hi[m] if sign > 0 else -lo[m]).min()) >= C.SHIFT + C.SPREAD - tol     # the +-1 keys are there
    m = sel("wide")
    if Skv > 1:
        assert float(hi[m].min()) >= C.WIDE - tol and float(lo[m].max()) <= -C.WIDE + tol
    assert float(s[m].abs().max()) <= C.WIDE + tol
    if "large" in fams and Skv > 1:
        m = sel("large")
        assert float(hi[m].min()) >= C.LARGE[D] - tol and float(lo[m].max()) <= -C.LARGE[D] + tol
    if "rising-3" in fams and nt > 1:
        base, cap = (-80.0, 80.0) if static else (0.0, C.CAP[D])
        for name, step in (("rising-3", 3.0), ("rising-7", 7.0)):
            tm = tmax[sel(name)]
            want = torch.clamp(base + step * torch.arange(nt), max=cap).double()
            # the tile maximum: the structured value plus the largest of 64 noise terms, the coordinate rounded to bf16
            assert float((tm - want).min()) >= -1.0 and float((tm - want).max()) <= tol, (name, (tm - want).aminmax())
        fm = tmax[sel("falling")]
        top = 80.0 if static else 0.0
        assert bool((fm.argmax(-1) == 0).all())
        floor = max(top - C.fall_rate(nt) * (nt - 1), top - 160.0)
        assert float(lo[sel("falling")].max()) <= floor + 1.0 and (static or floor <= -150.0)


def test_a_peaked_row_selects_the_first_tile_the_interior_and_the_last_key():
    c = next(c for c in C.ATTN_CASES if c["name"] == "run-1350x1350")
    d = C.attn_case_data(c)
    s = d["q"].double() @ d["k"][:, 0].double().transpose(1, 2)
    m = d["fam"] == FAMILIES.index("peaked")
    assert torch.equal(s.argmax(-1)[m], torch.tensor(d["peaks"])[d["peak"][m]])
    assert d["peaks"][0] < 64 and 64 <= d["peaks"][1] < 1344 and d["peaks"][2] == 1349
    for bh in range(d["q"].shape[0]):
        assert set(d["peak"][bh][m[bh]].tolist()) == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ (2) eps
@pytest.mark.parametrize("p,c", ALL_CASES, ids=IDS)
def test_the_fp32_terms_leave_the_per_element_bar_its_meaning(p, c):
    sabs = _extremes(p, c["name"])[0]
    eps = C.eps_of(c["Skv"] if p != "tiny" else c["L"], c.get("D", 64), sabs, n_id=c.get("n_id", 0), tiny=p == "tiny")
    print(f"{IDS[ALL_CASES.index((p, c))]}: S_abs {sabs:.1f}, eps {eps:.3f}")
    assert eps <= C.EPS_MAX, (c["name"], sabs, eps)
    assert max(c["Skv"] if p != "tiny" else c["L"], 1) <= 5056


# ------------------------------------------------------------------------------------------------ (3) the restatement and its variants
@pytest.mark.parametrize("p,c", ALL_CASES, ids=IDS)
def test_restatement_and_its_correct_variants_pass_both_bars(p, c):
    d = _data(p, c)
    fams = C.families_of(_path(p, c))
    q, k, v, fam, _ = _sample(d)
    o64, A = C.reference64(q, k, v)
    eps = C.eps_of(k.shape[1], q.shape[2], C.s_abs(q, k))
    forms = ["rowmax", "tiled"] + (["static"] if _path(p, c) in C.STATIC_KINDS else [])
    for form in forms:
        fig = C.figures(C.restate(q, k, v, form), o64, A, fam)
        assert set(fig) == set(fams)
        for f, (w, b, finite) in fig.items():
            print(f"{c['name']} {form:6s} {f:10s} worst e {w:.3f} b {b:+.3f}")
            assert finite and w <= 1 + eps, (form, f, w, eps)
            assert f == "flat" or abs(b) <= CORRECT_BIAS, (form, f, b)
        assert fig["flat"][1] == 0.0 or abs(fig["flat"][1]) <= CORRECT_BIAS


# ------------------------------------------------------------------------------------------------ (4) planted faults
def test_planted_faults_fail_a_bar(capsys):
    """On the data of two cases (200 and 1350 keys), in plain torch.  Truncations: the bias bar on every family but flat and peaked
    (P of a peaked row is 1 and 0: nothing to truncate; O truncation shows there too).  A lost last key on 32 of every 128 rows: the
    per-element bar on the rising rows (the last key carries the row) and on the gaussian rows, which at 1350 keys pass the
    Frobenius bar.  One padding key at score 0: the per-element bar on the shift-low rows, invisible on the friendly ones."""
    lines = []
    for name in ("pre-200x200", "pre-1350x1350", "w4-1350x1350"):
        c = next(c for c in C.ATTN_CASES if c["name"] == name)
        d = C.attn_case_data(c)
        q, k, v, fam = C.per_variant(d)
        o64, A = C.reference64(q, k, v)
        eps = C.eps_of(c["Skv"], c["D"], C.s_abs(q, k))
        base = C.figures(C.restate(q, k, v), o64, A, fam)
        friendly = fam == FAMILIES.index("friendly")
        some = (torch.arange(q.shape[1]) % 128 < 32)[None].expand(q.shape[0], -1)
        form = "static" if c["kind"] == "w4" else "tiled"
        for fault, rows in (("p_trunc", None), ("o_trunc", None), ("drop_last", some), ("pad_zero", some)):
            got = C.restate(q, k, v, form, fault, rows)
            fig = C.figures(got, o64, A, fam)
            fro = rel_fro(got[friendly].float(), o64[friendly])
            fails_a = [f for f, (w, b, _) in fig.items() if w > 1 + eps]
            fails_b = [f for f, (w, b, _) in fig.items() if f != "flat" and abs(b) > abs(base[f][1]) + C.BIAS_MARGIN]
            lines.append(f"{name} {form} {fault:9s}: fails (a) on {fails_a or '-'}, (b) on {fails_b or '-'}; worst e "
                         f"{max(w for w, _, _ in fig.values()):.1f}; friendly rows rel_fro {fro:.1e}: "
                         f"{'PASSES' if fro <= ATTN_TOL else 'fails'} the old bar")
            if fault == "p_trunc":
                hit = [f for f in fig if f not in ("flat", "peaked")]
                assert all(fig[f][1] <= -PLANTED_BIAS for f in hit), (name, fault, {f: fig[f][1] for f in hit})
                assert set(hit) <= set(fails_b)
            elif fault == "o_trunc":
                hit = [f for f in fig if f != "flat"]
                assert all(fig[f][1] <= -PLANTED_BIAS for f in hit), (name, fault, {f: fig[f][1] for f in hit})
                assert set(hit) <= set(fails_b)
            elif fault == "drop_last":
                assert {"rising-3", "rising-7"} <= set(fails_a) and (c["Skv"] < 1350 or "friendly" in fails_a), (name, fails_a)
                assert fig["rising-7"][0] >= 20
            else:
                assert "shift-low" in fails_a and fig["shift-low"][0] >= 100, (name, fig["shift-low"])
                assert "friendly" not in fails_a and "shift-high" not in fails_a
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ------------------------------------------------------------------------------------------------ (5) coverage
def _meta_case(c):
    nbh = c["B"] * c["H"]
    e = lambda *s: torch.empty(*s, device="meta")
    return dict(q=e(nbh, c["Sq"], c["D"]), k=e(nbh, c["L2"], c["Skv"], c["D"]), v=e(nbh, c["L2"], c["Skv"], c["D"]),
                want=e(nbh, c["L2"], c["Sq"], c["D"]))


def _attn_keys(ops, cases):
    import test_attn_exact_gpu as G
    keys = {}
    for c in cases:
        q, k, v, g, o, want, kw, _ = G.attn_layout(c, _meta_case(c), "meta")
        with ops.options(attn_streamk=c["sk_opt"], reference_forms=["attn_narrow_store"] if c["narrow"] else []):
            key = ops.attention_plan_key(ops.attention_plan(o, workspace=True, **kw))
        assert key == X.attn_case_key(c), (c["name"], key)
        keys.setdefault(key, c["name"])
    return keys


def _mix_key(ops, c):
    with ops.options(reference_forms=["kv_mix_generic"] if c["generic"] else []):
        g = X.GuardedOut(c["Sq"], c["H"] * c["D"], "meta", batch=c["grp"], col0=c["col0"])
        z = g.bf[:, g.r0:g.r0 + c["Sq"], g.c0:g.c0 + c["H"] * c["D"]]
        W = c["H"] * c["D"] + c["pad"]
        p = ops.attn_kv_mix_plan(z, None, head_dim=c["D"], heads=c["H"], n_id=c["n_id"], n_grp=c["grp"], Sq=c["Sq"], Skv=c["Skv"],
                                 q_strides=(c["Sq"] * W, W), k_strides=(c["grp"] * c["Skv"] * W, c["Skv"] * W, W),
                                 v_strides=(c["grp"] * c["Skv"] * W, c["Skv"] * W, W), z_strides=(z.stride(0), z.stride(1)))
    return f"{p['form']}_d{p['head_dim']}" + ("+big_lds" if p["big_lds"] else "")


def test_the_matrix_reaches_every_plan_the_exact_suite_reaches(ops, capsys):
    from test_attn_exact_cpu import _tiny_plan
    exact = _attn_keys(ops, [c for c in X.ATTN_CASES if c["Sq"] != 17776])
    mine = _attn_keys(ops, C.ATTN_CASES)
    assert set(mine) == set(exact), (sorted(set(exact) - set(mine)), sorted(set(mine) - set(exact)))
    mix_exact, mix_mine = {_mix_key(ops, c) for c in X.MIX_CASES}, {_mix_key(ops, c) for c in C.MIX_CASES}
    assert mix_mine == mix_exact == {"mix32_d64", "mix32_d128", "mix32_d128+big_lds", "one_tile_d64", "one_tile_d128"}
    assert any(c["generic"] for c in C.MIX_CASES) and any(c["col0"] % 8 for c in C.MIX_CASES)
    for c in C.MIX_CASES:
        assert _mix_key(ops, c) == X.mix_case_key(c)
    tiny_exact = {_tiny_plan(ops, c)["instance"] for c in X.TINY_CASES}
    tiny_mine = {_tiny_plan(ops, c)["instance"] for c in C.TINY_CASES}
    assert tiny_mine == tiny_exact == set(ops.TINY_INSTANCES.values()) and any(c["unaligned"] for c in C.TINY_CASES)
    with capsys.disabled():
        print("\n" + "\n".join(f"{k:48s} <- {v}" for k, v in sorted(mine.items())))
