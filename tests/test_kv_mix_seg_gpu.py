"""The kv-mix over a segment table (include/bya.h, bya_attn_kv_mix_seg / bya_attn_kv_mix_mx_seg; ops.attn_kv_mix_segments): ONE
launch writes, byte for byte, what the launches per segment write that the sharded engine issued before -- a partial head, a
whole frame, a tail shorter than a tile; 2 and 3 identities; 32 keys and 20 (masked); with and without wsum; the face weights;
two row chunks with an empty range; a gap; the grouped launch as a special case; both MX formats against the per-segment MX
launches AND the standalone quantiser.  Outputs start as canary bytes, every comparison is torch.equal on raw bytes, and
the plan (form, grid) is asserted before each launch."""
import functools

import pytest
import torch

from test_mx_attn_out_gpu import first_diff, two_launch_ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
H, D = 3, 64
E = H * D
FORMATS = ("mxfp8", "mxfp6")
CANARY = 0xA5

# name -> (K / V frames, rows of the buffers, segments)
TABLES = {
    "frames": (4, 160, ((1, 0, 45), (2, 45, 70), (3, 115, 7))),      # partial head, whole frame (per_frame 70), short tail
    "chunks": (2, 440, ((0, 0, 400), (1, 400, 33))),                 # two row chunks; the short segment's second one is empty
    "gap": (2, 110, ((0, 0, 40), (1, 64, 40))),                      # rows 40 .. 63 belong to nobody
}


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import ops
    return ops


def raw(t):
    return t.contiguous().view(torch.uint8)


def canary(dev, rows, cols, dtype):
    return torch.full((rows, cols * torch.empty((), dtype=dtype).element_size()), CANARY, dtype=torch.uint8, device=dev).view(dtype)


@functools.lru_cache(maxsize=None)
def inputs(dev, table, n_id, Skv, face):
    """q [rows, E], k / v [n_id, frames, Skv, E], routing logits r [rows, n_id] of mixed sign, af a random [n_id, n_id] (None:
    the face weights).  Cached: every test of a case reads the same tensors and leaves them alone."""
    frames, rows, _ = TABLES[table]
    g = torch.Generator().manual_seed(7 + 1000 * n_id + 10 * Skv + len(table) + face)
    torch.manual_seed(7 + 1000 * n_id + 10 * Skv + len(table) + face)
    rnd = lambda *s: torch.randn(*s, generator=g).to(BF).to(dev)
    return rnd(rows, E), rnd(n_id, frames, Skv, E), rnd(n_id, frames, Skv, E) * 2.0, rnd(rows, n_id), None if face else rnd(n_id, n_id)


def chunks_of(segs):
    return -(-(-(-max(s[2] for s in segs) // 32)) // 12)


def per_segment(ops, dev, table, n_id, Skv, face, wsum, fmt=None):
    """The launches the sharded engine issued: one ops.attn_kv_mix(n_grp=1, Sq=length) per segment on sliced views.
    -> (z or the MX pair, wsum or None), canaries wherever no launch wrote."""
    frames, rows, segs = TABLES[table]
    q, k, v, r, af = inputs(dev, table, n_id, Skv, face)
    kvs = (frames * Skv * E, 0, E)
    ws = canary(dev, rows, 1, torch.float32).view(-1) if wsum else None
    if fmt is None:
        out = canary(dev, rows, E, BF)
    else:
        out = (canary(dev, rows, ops.mx_code_bytes(E, fmt) + 12, torch.uint8), canary(dev, rows, E // 32 + 5, torch.uint8))
    for f, start, length in segs:
        to = dict(z_strides=(0, E)) if fmt is None else dict(mx_out=(out[0][start:], out[1][start:], fmt))
        got = ops.attn_kv_mix(q[start:], k[:, f], v[:, f], r[start:start + length], af, out[start:] if fmt is None else None,
                              None if ws is None else ws[start:], head_dim=D, heads=H, n_id=n_id, n_grp=1, Sq=length, Skv=Skv,
                              q_strides=(0, E), k_strides=kvs, v_strides=kvs, scale=D ** -0.5, **to)
        assert got is not False
    return out, ws


@functools.lru_cache(maxsize=None)
def reference(dev, table, n_id, Skv, face, wsum, fmt=None):
    from bind_your_avatar_implementation_amd import ops
    return per_segment(ops, dev, table, n_id, Skv, face, wsum, fmt)


def one_launch(ops, dev, table, n_id, Skv, face, wsum, fmt=None, segs=None):
    """ops.attn_kv_mix_segments into canary-filled outputs, the plan pinned first.  -> (z or the MX pair, wsum or None)."""
    frames, rows, table_segs = TABLES[table]
    segs = list(table_segs if segs is None else segs)
    q, k, v, r, af = inputs(dev, table, n_id, Skv, face)
    kvs = (frames * Skv * E, Skv * E, E)
    ws = canary(dev, rows, 1, torch.float32).view(-1) if wsum else None
    if fmt is None:
        out, to = canary(dev, rows, E, BF), dict(z_row=E)
    else:
        out = (canary(dev, rows, ops.mx_code_bytes(E, fmt) + 12, torch.uint8), canary(dev, rows, E // 32 + 5, torch.uint8))
        to = dict(mx_out=(*out, fmt))
    kw = dict(segments=segs, head_dim=D, heads=H, n_id=n_id, n_grp=frames, Sq=rows, Skv=Skv, q_row=E, k_strides=kvs, v_strides=kvs, **to)
    plan = ops.attn_kv_mix_segments_plan(out if fmt is None else None, af, **kw)
    assert plan is not None and plan["form"] == "mix32" and plan.get("mx_out") == fmt, plan
    assert (plan["row_chunks"], plan["grid"]) == (chunks_of(segs), chunks_of(segs) * H * len(segs)), plan
    assert plan["lds_bytes"] == (2 * n_id + 4) * 32 * D * 2 and not plan["big_lds"]
    got = ops.attn_kv_mix_segments(q, k, v, r, af, out if fmt is None else None, ws, scale=D ** -0.5, **kw)
    assert got is not False
    assert got is out if fmt is None else (got[0] is out[0] and got[1] is out[1])
    torch.cuda.synchronize()
    return out, ws


def written(table, rows):
    m = torch.zeros(rows, dtype=torch.bool)
    for _, start, length in TABLES[table][2]:
        m[start:start + length] = True
    return m


def assert_same(got, want, what):
    assert torch.equal(raw(got), raw(want)), f"{what}: " + first_diff(raw(got), raw(want))


# ------------------------------------------------------------------------------------------ 1. the launches it replaces
@pytest.mark.parametrize("wsum", [True, False], ids=["wsum", "nowsum"])
@pytest.mark.parametrize("Skv", [32, 20])
@pytest.mark.parametrize("n_id", [2, 3])
def test_equal_to_the_launches_per_segment(ops, dev, n_id, Skv, wsum):
    want, want_ws = reference(dev, "frames", n_id, Skv, False, wsum)
    z, ws = one_launch(ops, dev, "frames", n_id, Skv, False, wsum)
    assert_same(z, want, "z")
    assert bool((raw(z[122:]) == CANARY).all()) and not bool((raw(z[:122]) == CANARY).all(-1).any())
    if wsum:
        assert_same(ws, want_ws, "wsum")
        assert bool((raw(ws[122:]) == CANARY).all())


def test_equal_to_the_launches_per_segment_face_weights(ops, dev):
    want, want_ws = reference(dev, "frames", 2, 32, True, True)
    z, ws = one_launch(ops, dev, "frames", 2, 32, True, True)
    assert_same(z, want, "z")
    assert_same(ws, want_ws, "wsum")
    assert bool((raw(z[122:]) == CANARY).all()) and bool((raw(ws[122:]) == CANARY).all())


# ------------------------------------------------------------------------------------------ 2. row chunks, empty ranges
def test_two_row_chunks_and_an_empty_range(ops, dev):
    assert chunks_of(TABLES["chunks"][2]) == 2                      # 13 tiles of the long segment; the short one has 2 tiles
    want, want_ws = reference(dev, "chunks", 2, 32, False, True)
    z, ws = one_launch(ops, dev, "chunks", 2, 32, False, True)
    assert_same(z, want, "z")
    assert_same(ws, want_ws, "wsum")
    assert bool((raw(z[433:]) == CANARY).all()) and bool((raw(ws[433:]) == CANARY).all())
    # a one-tile segment beside it: chunk 0 of 2 is the empty one (tiles [0, 0)), chunk 1 computes
    segs = [(0, 0, 400), (1, 400, 20)]
    z2, ws2 = one_launch(ops, dev, "chunks", 2, 32, False, True, segs=segs)
    assert_same(z2[:420], want[:420], "z, one-tile segment")
    assert_same(ws2[:420], want_ws[:420], "wsum, one-tile segment")
    assert bool((raw(z2[420:]) == CANARY).all()) and bool((raw(ws2[420:]) == CANARY).all())


# ------------------------------------------------------------------------------------------ 3. a gap
def test_rows_in_a_gap_are_left_alone(ops, dev):
    want, want_ws = reference(dev, "gap", 2, 32, False, True)
    z, ws = one_launch(ops, dev, "gap", 2, 32, False, True)
    assert_same(z, want, "z")
    assert_same(ws, want_ws, "wsum")
    for lo, hi in ((40, 64), (104, 110)):
        assert bool((raw(z[lo:hi]) == CANARY).all()) and bool((raw(ws[lo:hi]) == CANARY).all())
    assert not bool((raw(z[64:104]) == CANARY).all(-1).any())


# ------------------------------------------------------------------------------------------ 4. the grouped launch
@pytest.mark.parametrize("Skv", [32, 20])
def test_uniform_segments_equal_the_grouped_launch(ops, dev, Skv):
    g = torch.Generator().manual_seed(96 + Skv)
    rnd = lambda *s: torch.randn(*s, generator=g).to(BF).to(dev)
    n_id, grp, Sq = 2, 4, 96
    q, k, v, r, af = rnd(grp * Sq, E), rnd(n_id, grp, Skv, E), rnd(n_id, grp, Skv, E), rnd(grp * Sq, n_id), rnd(n_id, n_id)
    kvs = (grp * Skv * E, Skv * E, E)
    common = dict(head_dim=D, heads=H, n_id=n_id, n_grp=grp, Skv=Skv, k_strides=kvs, v_strides=kvs, scale=D ** -0.5)
    want, want_ws = canary(dev, grp * Sq, E, BF), canary(dev, grp * Sq, 1, torch.float32).view(-1)
    assert ops.attn_kv_mix_plan(want, af, Sq=Sq, q_strides=(Sq * E, E), z_strides=(Sq * E, E), **common)["form"] == "mix32"
    ops.attn_kv_mix(q, k, v, r, af, want, want_ws, Sq=Sq, q_strides=(Sq * E, E), z_strides=(Sq * E, E), **common)
    z, ws = canary(dev, grp * Sq, E, BF), canary(dev, grp * Sq, 1, torch.float32).view(-1)
    segs = [(gi, gi * Sq, Sq) for gi in range(grp)]
    plan = ops.attn_kv_mix_segments_plan(z, af, segments=segs, Sq=grp * Sq, q_row=E, z_row=E, **common)
    assert (plan["form"], plan["row_chunks"], plan["grid"]) == ("mix32", 1, H * grp)
    assert ops.attn_kv_mix_segments(q, k, v, r, af, z, ws, segments=segs, Sq=grp * Sq, q_row=E, z_row=E, **common) is z
    assert_same(z, want, "z")
    assert_same(ws, want_ws, "wsum")


# ------------------------------------------------------------------------------------------ 5. the MX output
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("table,n_id,Skv", [("frames", 2, 32), ("frames", 3, 20), ("frames", 3, 32), ("frames", 2, 20), ("chunks", 2, 32),
                                            ("gap", 2, 32)])
def test_mx_output_equals_the_per_segment_launches_and_the_quantiser(ops, dev, fmt, table, n_id, Skv):
    rows = TABLES[table][1]
    (want_c, want_s), want_ws = reference(dev, table, n_id, Skv, False, True, fmt)
    (codes, scales), ws = one_launch(ops, dev, table, n_id, Skv, False, True, fmt)
    assert_same(scales, want_s, f"{fmt} scales")
    assert_same(codes, want_c, f"{fmt} codes")
    assert_same(ws, want_ws, "wsum")
    assert_same(ws, reference(dev, table, n_id, Skv, False, True)[1], "wsum of the bf16 launches")
    # ... and the standalone quantiser on the bf16 rows; canaries in the rows of no segment and behind the heads' bytes
    zc, zs = two_launch_ref(ops, reference(dev, table, n_id, Skv, False, True)[0], fmt)
    cb, sb = ops.mx_code_bytes(E, fmt), E // 32
    m = written(table, rows).to(dev)
    full_c, full_s = torch.full_like(codes, CANARY), torch.full_like(scales, CANARY)
    full_c[:, :cb] = torch.where(m[:, None], zc, full_c[:, :cb])
    full_s[:, :sb] = torch.where(m[:, None], zs, full_s[:, :sb])
    assert_same(scales, full_s, f"{fmt} scales against quantize_mx")
    assert_same(codes, full_c, f"{fmt} codes against quantize_mx")


def test_mx_output_without_wsum_and_with_face_weights(ops, dev):
    for fmt in FORMATS:
        (want_c, want_s), _ = reference(dev, "frames", 2, 32, True, False, fmt)
        (codes, scales), ws = one_launch(ops, dev, "frames", 2, 32, True, False, fmt)
        assert ws is None
        assert_same(scales, want_s, f"{fmt} scales")
        assert_same(codes, want_c, f"{fmt} codes")


# ------------------------------------------------------------------------------------------ 6. declined, timers
def test_declined_launch_writes_and_counts_nothing(ops, dev):
    """More than 32 keys: False from both outputs, no launch, no timer entry; the generic reference form likewise."""
    n_id, rows, Skv = 2, 64, 40
    g = torch.Generator().manual_seed(40)
    rnd = lambda *s: torch.randn(*s, generator=g).to(BF).to(dev)
    q, k, v, r, af = rnd(rows, E), rnd(n_id, 1, Skv, E), rnd(n_id, 1, Skv, E), rnd(rows, n_id), rnd(n_id, n_id)
    kw = dict(segments=[(0, 0, 30), (0, 30, 34)], head_dim=D, heads=H, n_id=n_id, n_grp=1, Sq=rows, Skv=Skv, q_row=E,
              k_strides=(Skv * E, Skv * E, E), v_strides=(Skv * E, Skv * E, E), scale=D ** -0.5)
    z = canary(dev, rows, E, BF)
    pair = (canary(dev, rows, ops.mx_code_bytes(E, "mxfp8"), torch.uint8), canary(dev, rows, E // 32, torch.uint8))
    ops.enable_kernel_timers()
    try:
        assert ops.attn_kv_mix_segments(q, k, v, r, af, z, None, z_row=E, **kw) is False
        assert ops.attn_kv_mix_segments(q, k, v, r, af, None, None, mx_out=(*pair, "mxfp8"), **kw) is False
        with ops.options(reference_forms="kv_mix_generic"):
            assert ops.attn_kv_mix_segments(q, k[:, :, :32], v[:, :, :32], r, af, z, None, z_row=E, **dict(kw, Skv=32)) is False
        good = ops.attn_kv_mix_segments(q, k[:, :, :32], v[:, :, :32], r, af, z, None, z_row=E, **dict(kw, Skv=32))
        assert good is z
    finally:
        times = ops.collect_kernel_timers()
    assert len(times.get("bya_attn_kv_mix_seg", ())) == 1 and "bya_attn_kv_mix_mx_seg" not in times
    assert ops.kernel_timer_flops()["bya_attn_kv_mix_seg"] == 4.0 * n_id * H * 32 * D * 64
    assert bool((raw(pair[0]) == CANARY).all()) and not bool((raw(z) == CANARY).all(-1).any())
