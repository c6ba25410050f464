"""The batch forms of the four per-sample launches of a guided step (include/bya.h: bya_attn_kv_mix_batch, bya_attn_kv_mix_mx_batch,
bya_router_scores_batch, bya_router_head_batch; ops.attn_kv_mix_batch, ops.router_scores_batch, ops.router_head_batch): ONE
launch writes, byte for byte, what the n single-sample launches write.  Every sample has operands of its own (a sample that read
its neighbour's K, V, r or af would change bytes), outputs start as canary bytes and are padded (rows behind Sq, columns behind
the heads, a gap between the samples), every comparison is torch.equal on raw bytes, and the plan (form, grid) is asserted before
each launch."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H = 2
CANARY = 0xA5
FORMATS = ("mxfp8", "mxfp6")


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def raw(t):
    return t.contiguous().view(torch.uint8)


def canary(dev, shape, dtype):
    n = torch.empty((), dtype=dtype).element_size()
    return torch.full((*shape[:-1], shape[-1] * n), CANARY, dtype=torch.uint8, device=dev).view(dtype)


def first_diff(a, b):
    bad = (a != b).flatten().nonzero()
    return f"{bad.numel()} bytes differ, first at {int(bad[0])} of {a.numel()}" if bad.numel() else "equal"


def assert_same(got, want, what):
    assert got.shape == want.shape
    assert torch.equal(raw(got), raw(want)), f"{what}: " + first_diff(raw(got), raw(want))


# head_dim 64: the audio form (af present, two K / V groups); head_dim 128: the face form (af absent, one group)
def geometry(D, Sq):
    return dict(n_grp=2 if D == 64 else 1, audio=D == 64, E=H * D, Sq=Sq)


@functools.lru_cache(maxsize=None)
def inputs(dev, n, n_id, D, Sq, Skv, shared_r):
    """q [n, n_grp * Sq, E], k / v [n, n_id, n_grp, Skv, E], r [n or 1, n_grp * Sq, n_id] of mixed sign, af [n, n_id, n_id] or None:
    distinct per sample.  Cached: every test of a case reads the same tensors and leaves them alone."""
    geo = geometry(D, Sq)
    g = torch.Generator().manual_seed(11 + 1000 * n + 100 * n_id + D + 7 * Sq + Skv + shared_r)
    rnd = lambda *s: torch.randn(*s, generator=g).to(BF).to(dev)
    rows = geo["n_grp"] * Sq
    return (rnd(n, rows, geo["E"]), rnd(n, n_id, geo["n_grp"], Skv, geo["E"]), rnd(n, n_id, geo["n_grp"], Skv, geo["E"]) * 2.0,
            rnd(1 if shared_r else n, rows, n_id), rnd(n, n_id, n_id) if geo["audio"] else None)


def outputs(ops, dev, n, D, Sq, fmt, wsum, pad):
    """Canary-filled outputs of n samples: z [n, rows + pad rows, E + pad columns] or the MX pair likewise, wsum [n, rows + pad]."""
    geo = geometry(D, Sq)
    rows, E = geo["n_grp"] * Sq, geo["E"]
    extra_r, extra_c = (3, 8) if pad else (0, 0)
    ws = canary(dev, (n, rows + extra_r), torch.float32) if wsum else None
    if fmt is None:
        return canary(dev, (n, rows + extra_r, E + extra_c), BF), ws
    return (canary(dev, (n, rows + extra_r, ops.mx_code_bytes(E, fmt) + 4 * bool(pad)), torch.uint8),
            canary(dev, (n, rows + extra_r, E // 32 + 5 * bool(pad)), torch.uint8)), ws


def mix_kw(D, Sq, Skv, n_id):
    geo = geometry(D, Sq)
    E, G = geo["E"], geo["n_grp"]
    kvs = (G * Skv * E, Skv * E, E)
    return dict(head_dim=D, heads=H, n_id=n_id, n_grp=G, Sq=Sq, Skv=Skv, q_strides=(Sq * E, E), k_strides=kvs, v_strides=kvs,
                scale=D ** -0.5)


def out_views(out, fmt, D, Sq):
    """The [n, n_grp, Sq, width] views of the outputs the launches write through, and z's strides within a sample."""
    geo = geometry(D, Sq)
    rows = geo["n_grp"] * Sq
    if fmt is None:
        return out[:, :rows], (Sq * out.stride(1), out.stride(1))
    return tuple(t[:, :rows].unflatten(1, (geo["n_grp"], Sq)) for t in out), None


def per_sample(ops, dev, n, n_id, D, Sq, Skv, fmt, wsum, pad, shared_r):
    q, k, v, r, af = inputs(dev, n, n_id, D, Sq, Skv, shared_r)
    out, ws = outputs(ops, dev, n, D, Sq, fmt, wsum, pad)
    view, zs = out_views(out, fmt, D, Sq)
    kw = mix_kw(D, Sq, Skv, n_id)
    for b in range(n):
        to = dict(z_strides=zs) if fmt is None else dict(mx_out=(view[0][b], view[1][b], fmt))
        plan = ops.attn_kv_mix_plan(view[b] if fmt is None else None, None if af is None else af[b], **dict(kw, **to))
        assert plan["form"] == "mix32", plan
        got = ops.attn_kv_mix(q[b], k[b], v[b], r[0 if shared_r else b], None if af is None else af[b],
                              view[b] if fmt is None else None, None if ws is None else ws[b], **kw, **to)
        assert got is not False
    torch.cuda.synchronize()
    return out, ws


@functools.lru_cache(maxsize=None)
def reference(dev, n, n_id, D, Sq, Skv, fmt=None, wsum=True, pad=True, shared_r=False):
    from bind_your_avatar_implementation_amd import ops
    return per_sample(ops, dev, n, n_id, D, Sq, Skv, fmt, wsum, pad, shared_r)


def one_launch(ops, dev, n, n_id, D, Sq, Skv, fmt=None, wsum=True, pad=True, shared_r=False):
    q, k, v, r, af = inputs(dev, n, n_id, D, Sq, Skv, shared_r)
    out, ws = outputs(ops, dev, n, D, Sq, fmt, wsum, pad)
    view, zs = out_views(out, fmt, D, Sq)
    kw = mix_kw(D, Sq, Skv, n_id)
    to = dict(z_strides=zs) if fmt is None else dict(mx_out=(*view, fmt))
    z = view if fmt is None else None
    one = ops.attn_kv_mix_plan(view[0] if fmt is None else None, None if af is None else af[0],
                               **dict(kw, **(to if fmt is None else dict(mx_out=(view[0][0], view[1][0], fmt)))))
    strides = dict(q=q.stride(0), k=k.stride(0), v=v.stride(0), r=0 if shared_r else r.stride(0), wsum=ws.stride(0) if wsum else 0)
    plan = ops.attn_kv_mix_batch_plan(z, af, n=n, sample_strides=strides, **dict(kw, **to))
    assert plan == dict(one, grid=one["grid"] * n) and plan["form"] == "mix32", (plan, one)
    got = ops.attn_kv_mix_batch(q, k, v, r, af, z, ws, **kw, **to)
    assert got is not False
    torch.cuda.synchronize()
    return out, ws


CASES = [(n, n_id, D, Sq, Skv) for n, n_id in ((2, 2), (3, 3), (2, 3), (3, 2)) for D in (64, 128)
         for Sq, Skv in ((33, 32), (65, 5), (33, 5), (65, 32))]


@pytest.mark.parametrize("n,n_id,D,Sq,Skv", CASES)
def test_bf16_output_equals_the_launches_per_sample(ops, dev, n, n_id, D, Sq, Skv):
    want, want_ws = reference(dev, n, n_id, D, Sq, Skv)
    z, ws = one_launch(ops, dev, n, n_id, D, Sq, Skv)
    assert_same(z, want, "z")
    assert_same(ws, want_ws, "wsum")
    rows, E = geometry(D, Sq)["n_grp"] * Sq, H * D
    # the padding -- rows behind the sample's, columns behind the heads' -- is canary still, and every row was written
    assert bool((raw(z[:, rows:]) == CANARY).all()) and bool((raw(z[:, :, E:]) == CANARY).all())
    assert bool((raw(ws[:, rows:]) == CANARY).all())
    assert not bool((raw(z[:, :rows, :E]) == CANARY).all(-1).any())
    # the samples differ from one another: a sample that had read its neighbour's operands would show above
    assert not torch.equal(z[0], z[1])


@pytest.mark.parametrize("D", [64, 128])
def test_a_zero_stride_shares_r_and_no_wsum_is_fine(ops, dev, D):
    want, _ = reference(dev, 2, 2, D, 65, 32, None, False, False, True)
    z, ws = one_launch(ops, dev, 2, 2, D, 65, 32, None, False, False, True)
    assert ws is None
    assert_same(z, want, "z")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n,n_id,D,Sq,Skv", [(2, 2, 64, 33, 32), (3, 3, 64, 65, 5), (2, 3, 128, 65, 32), (3, 2, 128, 33, 5)])
def test_mx_output_equals_the_launches_per_sample(ops, dev, fmt, n, n_id, D, Sq, Skv):
    (want_c, want_s), want_ws = reference(dev, n, n_id, D, Sq, Skv, fmt)
    (codes, scales), ws = one_launch(ops, dev, n, n_id, D, Sq, Skv, fmt)
    assert_same(scales, want_s, f"{fmt} scales")
    assert_same(codes, want_c, f"{fmt} codes")
    assert_same(ws, want_ws, "wsum")
    assert_same(ws, reference(dev, n, n_id, D, Sq, Skv)[1], "wsum of the bf16 launches")
    rows, cb, sb = geometry(D, Sq)["n_grp"] * Sq, ops.mx_code_bytes(H * D, fmt), H * D // 32
    assert bool((codes[:, rows:] == CANARY).all()) and bool((codes[:, :, cb:] == CANARY).all())
    assert bool((scales[:, rows:] == CANARY).all()) and bool((scales[:, :, sb:] == CANARY).all())


def test_declined_launch_writes_and_counts_nothing(ops, dev):
    """More than 32 keys, or the generic reference form: False, no launch, no timer entry, the outputs untouched."""
    n, n_id, D, Sq = 2, 2, 64, 33
    q, k, v, r, af = inputs(dev, n, n_id, D, Sq, 32, False)
    g = torch.Generator().manual_seed(40)
    k40 = torch.randn(n, n_id, 2, 40, H * D, generator=g).to(BF).to(dev)
    z, ws = outputs(ops, dev, n, D, Sq, None, True, False)
    view, zs = out_views(z, None, D, Sq)
    ops.enable_kernel_timers()
    try:
        assert ops.attn_kv_mix_batch(q, k40, k40, r, af, view, ws, **mix_kw(D, Sq, 40, n_id), z_strides=zs) is False
        with ops.options(reference_forms="kv_mix_generic"):
            assert ops.attn_kv_mix_batch(q, k, v, r, af, view, ws, **mix_kw(D, Sq, 32, n_id), z_strides=zs) is False
        torch.cuda.synchronize()
        assert bool((raw(z) == CANARY).all()) and bool((raw(ws) == CANARY).all())
        assert ops.attn_kv_mix_batch(q, k, v, r, af, view, ws, **mix_kw(D, Sq, 32, n_id), z_strides=zs) is view
    finally:
        times = ops.collect_kernel_timers()
    assert len(times.get("bya_attn_kv_mix_batch", ())) == 1 and set(times) == {"bya_attn_kv_mix_batch"}


# ------------------------------------------------------------------------------------------ the router's scores and head
@functools.lru_cache(maxsize=None)
def router_inputs(dev, n, n_id, N):
    g = torch.Generator().manual_seed(5 + 10 * n_id + N)
    rnd = lambda *s: torch.randn(*s, generator=g).to(BF).to(dev)
    return (rnd(n, N, 2048), rnd(n, n_id, 32, 2048), 1 + 0.1 * rnd(512), 0.1 * rnd(512), rnd(N, 512), rnd(n, n_id, N, 512),
            rnd(512) * 0.05, rnd(1))


# (4099 rows: the form that keeps an identity's keys in LDS, from 4096 rows on; the others: one wave per 16-row tile)
@pytest.mark.parametrize("n_id,N", [(2, 70), (3, 70), (2, 257), (3, 257), (2, 4099)])
def test_router_scores_batch_equals_the_launches_per_sample(ops, dev, n_id, N):
    n = 2
    qr, kr, ln_w, ln_b, pos, _, _, _ = router_inputs(dev, n, n_id, N)
    want, got = canary(dev, (n, n_id * N + 2, 512), BF), canary(dev, (n, n_id * N + 2, 512), BF)      # two spare rows per sample
    view = lambda t: t[:, :n_id * N].unflatten(1, (n_id, N))
    for b in range(n):
        ops.router_scores(qr[b], kr[b], ln_w, ln_b, pos, view(want)[b], n_id, N)
    one = ops.router_scores_plan(qr[0], kr[0], ln_w, ln_b, pos, view(got)[0], n_id, N)
    plan = ops.router_scores_batch_plan(qr, kr, ln_w, ln_b, pos, view(got), n_id, N)
    assert plan == dict(one, grid=one["grid"] * n) and plan["kernel"] == ("lds" if N >= 4096 else "wave"), (plan, one)
    assert ops.router_scores_batch(qr, kr, ln_w, ln_b, pos, view(got), n_id, N) is not False
    torch.cuda.synchronize()
    assert_same(got, want, "router scores")
    assert bool((raw(got[:, n_id * N:]) == CANARY).all()) and not bool((raw(got[:, :n_id * N]) == CANARY).all(-1).any())
    assert not torch.equal(got[0], got[1])


@pytest.mark.parametrize("n_id,N", [(2, 70), (3, 70), (2, 257), (3, 257)])
def test_router_head_batch_equals_the_launches_per_sample(ops, dev, n_id, N):
    n = 2
    _, _, _, _, _, x, w, b = router_inputs(dev, n, n_id, N)
    want, got = canary(dev, (n, N + 1, n_id), BF), canary(dev, (n, N + 1, n_id), BF)                  # a spare row per sample
    for s in range(n):
        ops.router_head(x[s], w, b, want[s, :N], n_id, N)
    plan = ops.router_head_batch_plan(x, w, b, got[:, :N], n_id, N)
    assert (plan["grid"], plan["items"]) == (-(-N * n_id // 4) * n, N * n_id), plan
    assert ops.router_head_batch(x, w, b, got[:, :N], n_id, N) is not False
    torch.cuda.synchronize()
    assert_same(got, want, "routing logits")
    assert bool((raw(got[:, N:]) == CANARY).all()) and not bool((raw(got[:, :N]) == CANARY).all(-1).any())
    assert not torch.equal(got[0], got[1])
