"""CPU: the C ABI of the kv-mix over a segment table (include/bya.h: bya_attn_kv_mix_seg, bya_attn_kv_mix_mx_seg and their plan
queries) -- every refusal with its code before any launch and the plan left alone, the plan of accepted tables -- and the
ops front end on meta tensors."""
import ctypes
import os

import pytest
import torch

OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
E4M3, E2M3 = 0, 2
BASE = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from bind_your_avatar_implementation_amd import _hip
    from bind_your_avatar_implementation_amd.build import build_hip_library
    build_hip_library()
    return _hip.load()


def desc(D=64, H=3, n_id=2, n_grp=4, Sq=500, Skv=32, mx=False):
    from bind_your_avatar_implementation_amd import _hip
    d = _hip.AttnMixDesc()
    d.head_dim, d.heads, d.n_id, d.n_grp, d.Sq, d.Skv = D, H, n_id, n_grp, Sq, Skv
    d.q_row = d.k_row = d.v_row = H * D
    d.z_row = 0 if mx else H * D
    d.k_grp = d.v_grp = Skv * H * D
    d.k_id = d.v_id = n_grp * Skv * H * D
    d.scale = D ** -0.5
    return d


def table(segs):
    from bind_your_avatar_implementation_amd import _hip
    s = _hip.AttnMixSegments()
    s.n = len(segs)
    for i, (g, a, n) in enumerate(segs[:16]):
        s.grp[i], s.start[i], s.len[i] = g, a, n
    return s


def mx_strides(d, fmt):
    return [0, d.heads * d.head_dim * (8 if fmt == E4M3 else 6) // 8, 0, d.heads * d.head_dim // 32]


class Entry:
    """One of the four entry points behind one signature: call(desc, table or None, **what differs from a good call)."""

    def __init__(self, lib, mx, plan):
        self.lib, self.mx, self.plan = lib, mx, plan
        self.name = "bya_attn_kv_mix" + ("_mx" if mx else "") + "_seg" + ("_plan" if plan else "")

    def __call__(self, d, seg, out=BASE, af=None, st=None, fmt=E2M3, q=BASE):
        from bind_your_avatar_implementation_amd import _hip
        self.filled = _hip.AttnMixPlan(-9, -9, -9, -9, -9, -9)
        segp = None if seg is None else ctypes.byref(seg)
        dp = None if d is None else ctypes.byref(d)
        outs = (out, out) if self.mx else (out,)
        tail = (dp, segp) + ((fmt, *(st or (mx_strides(d, fmt) if d is not None else [0, 144, 0, 6]))) if self.mx else ())
        fn = getattr(self.lib, self.name)
        if self.plan:
            return fn(*outs, af, *tail, ctypes.byref(self.filled))
        return fn(q, BASE, BASE, BASE, af, *outs, None, *tail, None)

    def untouched(self):
        p = self.filled
        return (p.form, p.head_dim, p.grid, p.row_chunks, p.lds_bytes, p.big_lds) == (-9,) * 6


ENTRIES = [(mx, plan) for mx in (False, True) for plan in (False, True)]
GOOD = [(1, 0, 45), (2, 45, 70), (3, 115, 7)]


def test_binding_table_has_the_four_entry_points(lib):
    from bind_your_avatar_implementation_amd import _hip
    for name, nargs in (("bya_attn_kv_mix_seg", 10), ("bya_attn_kv_mix_seg_plan", 5), ("bya_attn_kv_mix_mx_seg", 16),
                        ("bya_attn_kv_mix_mx_seg_plan", 11)):
        assert len(_hip.SIGNATURES[name]) == nargs and hasattr(lib, name)
    assert _hip.MIX_MAX_SEGMENTS == 16 and ctypes.sizeof(_hip.AttnMixSegments) == 4 * (1 + 3 * 16)
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bya.h")).read()
    assert "#define BYA_MIX_MAX_SEGMENTS 16" in src
    body = src.split("typedef struct bya_attn_mix_segments {")[1].split("}")[0]
    assert [w for w in ("n;", "grp[", "start[", "len[") if w in body] == ["n;", "grp[", "start[", "len["]
    assert body.index("n;") < body.index("grp[") < body.index("start[") < body.index("len[")


@pytest.mark.parametrize("mx,plan", ENTRIES)
def test_every_refusal_has_its_code_and_leaves_the_plan_alone(lib, mx, plan):
    from bind_your_avatar_implementation_amd import _hip
    e, query = Entry(lib, mx, plan), Entry(lib, mx, True)

    def refused(code, d, seg, **kw):
        # (the addresses are made up: a launch entry is only ever called with what its query, the same checks, has refused)
        assert "q" in kw or query(d, seg, **kw) == code, (query.name, code, kw)
        assert e(d, seg, **kw) == code, (e.name, code, kw)
        assert e.untouched()

    def accepted(d, seg):
        assert query(d, seg) == OK

    d = desc(mx=mx)
    accepted(d, table(GOOD))                                             # the good call every refusal below departs from
    # ---- BYA_ERR_SHAPE
    refused(ERR_SHAPE, d, None)                                          # seg is NULL
    refused(ERR_SHAPE, d, table([]))                                     # n outside 1 .. 16
    t17 = table([(0, 8 * i, 8) for i in range(16)])
    t17.n = 17
    refused(ERR_SHAPE, d, t17)
    t17.n = -1
    refused(ERR_SHAPE, d, t17)
    refused(ERR_SHAPE, d, table([(1, 0, 45), (2, 45, 0)]))               # a len <= 0
    refused(ERR_SHAPE, d, table([(1, 0, 45), (2, 45, -3)]))
    refused(ERR_SHAPE, d, table([(1, 0, 45), (4, 45, 70)]))              # a grp out of range: n_grp = 4
    refused(ERR_SHAPE, d, table([(-1, 0, 45)]))
    refused(ERR_SHAPE, d, table([(1, 0, 45), (2, 45, 456)]))             # rows past Sq = 500
    refused(ERR_SHAPE, d, table([(1, 500, 1)]))
    refused(ERR_SHAPE, d, table([(1, -1, 45)]))
    refused(ERR_SHAPE, d, table([(1, 0, 45), (2, 44, 70)]))              # overlapping
    refused(ERR_SHAPE, d, table([(2, 45, 70), (1, 0, 45)]))              # descending
    accepted(d, table([(1, 0, 45), (2, 45, 455)]))                       # ... up to Sq, touching, is fine
    accepted(d, table([(0, 8 * i, 8) for i in range(16)]))               # ... and so are 16
    dq = desc(mx=mx)
    dq.q_grp = 8
    refused(ERR_SHAPE, dq, table(GOOD))                                  # a group stride on q
    dz = desc(mx=mx)
    dz.z_grp = 8
    refused(ERR_SHAPE, dz, table(GOOD))                                  # ... on z
    if mx:
        st = mx_strides(d, E2M3)
        refused(ERR_SHAPE, d, table(GOOD), st=[4, st[1], 0, st[3]])      # ... on codes
        refused(ERR_SHAPE, d, table(GOOD), st=[0, st[1], 4, st[3]])      # ... on scales
        # what bya_attn_kv_mix_mx refuses
        dzr = desc(mx=True)
        dzr.z_row = 192
        refused(ERR_SHAPE, dzr, table(GOOD))                             # there is no bf16 output
        refused(ERR_SHAPE, d, table(GOOD), st=[0, st[1] - 4, 0, st[3]])  # c_row too short for the heads
        refused(ERR_SHAPE, d, table(GOOD), st=[0, st[1], 0, st[3] - 1])
        refused(ERR_ALIGN, d, table(GOOD), st=[0, st[1] + 2, 0, st[3]])
        refused(ERR_ALIGN, d, table(GOOD), out=BASE + 2)
        refused(ERR_UNSUPPORTED, d, table(GOOD), fmt=4)                  # e2m1 is never an activation format
    # what bya_attn_kv_mix refuses
    refused(ERR_SHAPE, None, table(GOOD))
    refused(ERR_SHAPE, d, table(GOOD), out=None)
    refused(ERR_SHAPE, desc(Skv=65, mx=mx), table(GOOD))
    refused(ERR_SHAPE, desc(n_id=5, mx=mx), table(GOOD))
    refused(ERR_SHAPE, desc(n_id=1, mx=mx), table(GOOD), af=BASE)        # audio weights need >= 2 streams
    refused(ERR_UNSUPPORTED, desc(D=96, mx=mx), table(GOOD))
    dr = desc(mx=mx)
    dr.k_row = 196
    refused(ERR_ALIGN, dr, table(GOOD))
    if not mx:
        refused(ERR_ALIGN, d, table(GOOD), out=BASE + 4)                 # z not 8-byte aligned
    if not plan:
        refused(ERR_SHAPE, d, table(GOOD), q=None)
        refused(ERR_ALIGN, d, table(GOOD), q=BASE + 8)
    # ---- BYA_ERR_UNSUPPORTED: the segment form exists on the mix32 form with head_dim 64 alone
    refused(ERR_UNSUPPORTED, desc(Skv=40, mx=mx), table(GOOD))           # Skv > 32
    refused(ERR_UNSUPPORTED, desc(D=128, mx=mx), table(GOOD))            # head_dim 128
    _hip.set_option("reference_forms", _hip.REFERENCE_FORMS["kv_mix_generic"])
    try:
        refused(ERR_UNSUPPORTED, d, table(GOOD))                         # BYA_REF_KV_MIX_GENERIC is set
    finally:
        _hip.set_option("reference_forms", 0)
    if not mx:
        refused(ERR_UNSUPPORTED, d, table(GOOD), out=BASE + 8)           # z not 16-byte aligned
        dodd = desc()
        dodd.z_row = 196
        refused(ERR_UNSUPPORTED, dodd, table(GOOD))                      # odd z stride (a multiple of 4, not of 8)
    accepted(d, table(GOOD))


def test_a_null_plan_is_refused(lib):
    d, s = desc(), table(GOOD)
    assert lib.bya_attn_kv_mix_seg_plan(BASE, None, ctypes.byref(d), ctypes.byref(s), None) == ERR_SHAPE
    dm = desc(mx=True)
    assert lib.bya_attn_kv_mix_mx_seg_plan(BASE, BASE, None, ctypes.byref(dm), ctypes.byref(s), E2M3, *mx_strides(dm, E2M3),
                                           None) == ERR_SHAPE


@pytest.mark.parametrize("mx", [False, True])
@pytest.mark.parametrize("segs,heads,n_id,chunks", [([(0, 0, 45)], 3, 2, 1), ([(1, 0, 400), (2, 400, 33)], 3, 2, 2),
                                                     ([(0, 0, 384)], 3, 3, 1), ([(0, 0, 385), (0, 385, 1), (3, 386, 9)], 48, 4, 2)])
def test_plan_of_accepted_tables(lib, mx, segs, heads, n_id, chunks):
    """form mix32, row_chunks = ceil(ceil(L / 32) / 12) of the LONGEST segment, grid = row_chunks * heads * n, and the LDS of
    the grouped launch with the same identities."""
    from bind_your_avatar_implementation_amd import _hip
    e = Entry(lib, mx, True)
    d = desc(H=heads, n_id=n_id, mx=mx)
    assert e(d, table(segs)) == OK
    p = e.filled
    longest = max(s[2] for s in segs)
    assert chunks == -(-(-(-longest // 32)) // 12)
    assert (p.form, p.head_dim, p.row_chunks, p.grid, p.big_lds) == (0, 64, chunks, chunks * heads * len(segs), 0)
    g = _hip.AttnMixPlan()
    d.z_row = heads * 64
    assert lib.bya_attn_kv_mix_plan(BASE, None, ctypes.byref(d), ctypes.byref(g)) == OK
    assert p.lds_bytes == g.lds_bytes == (2 * n_id + 4) * 32 * 64 * 2


def test_plan_grids_named_in_the_header_comment(lib):
    e = Entry(lib, False, True)
    assert e(desc(), table([(0, 0, 45)])) == OK and (e.filled.row_chunks, e.filled.grid) == (1, 3)
    assert e(desc(), table([(1, 0, 400), (2, 400, 33)])) == OK and (e.filled.row_chunks, e.filled.grid) == (2, 2 * 3 * 2)


def test_ops_front_end_on_meta_tensors(lib):
    from bind_your_avatar_implementation_amd import _hip, ops
    H, D = 3, 64
    kw = dict(head_dim=D, heads=H, n_id=2, n_grp=4, Sq=160, Skv=32, q_row=H * D, k_strides=(4 * 32 * H * D, 32 * H * D, H * D),
              v_strides=(4 * 32 * H * D, 32 * H * D, H * D))
    z = torch.empty(160, H * D, dtype=torch.bfloat16, device="meta")
    af = torch.empty(2, 2, dtype=torch.bfloat16, device="meta")
    p = ops.attn_kv_mix_segments_plan(z, af, segments=GOOD, z_row=H * D, **kw)
    assert p == {"form": "mix32", "head_dim": 64, "grid": 1 * H * 3, "row_chunks": 1, "lds_bytes": 8 * 4096, "big_lds": 0}
    grouped = {k: v for k, v in kw.items() if k != "q_row"}
    assert p.keys() == ops.attn_kv_mix_plan(z, af, z_strides=(0, H * D), q_strides=(0, H * D), **dict(grouped, n_grp=1)).keys()
    p2 = ops.attn_kv_mix_segments_plan(z, None, segments=[(1, 0, 400 - 300), (2, 100, 33)], z_row=H * D, **kw)
    assert (p2["row_chunks"], p2["grid"]) == (1, 6)
    big = dict(kw, Sq=433)
    zb = torch.empty(433, H * D, dtype=torch.bfloat16, device="meta")
    p3 = ops.attn_kv_mix_segments_plan(zb, None, segments=[(1, 0, 400), (2, 400, 33)], z_row=H * D, **big)
    assert (p3["form"], p3["row_chunks"], p3["grid"]) == ("mix32", 2, 2 * H * 2)
    # a view that starts 8 bytes into its buffer: no segment form (the grouped launch would take its one-tile form)
    off = torch.empty(160 * H * D + 4, dtype=torch.bfloat16, device="meta")[4:].view(160, H * D)
    assert ops.attn_kv_mix_segments_plan(off, af, segments=GOOD, z_row=H * D, **kw) is None
    # declined: None, not an error
    assert ops.attn_kv_mix_segments_plan(z, af, segments=GOOD, z_row=H * D, **dict(kw, Skv=40)) is None
    # the MX output: the pair holds Sq rows, no group stride
    c = torch.empty(160, H * D * 6 // 8, dtype=torch.uint8, device="meta")
    s = torch.empty(160, H * D // 32, dtype=torch.uint8, device="meta")
    pm = ops.attn_kv_mix_segments_plan(None, af, segments=GOOD, mx_out=(c, s, "mxfp6"), **kw)
    assert pm == dict(p, mx_out="mxfp6")
    assert ops.attn_kv_mix_segments_plan(None, af, segments=GOOD, mx_out=(c, s, "mxfp6"), **dict(kw, Skv=40)) is None
    with pytest.raises(ValueError, match="no bf16 output"):
        ops.attn_kv_mix_segments_plan(z, af, segments=GOOD, mx_out=(c, s, "mxfp6"), **kw)
    with pytest.raises(ValueError):
        ops.attn_kv_mix_segments_plan(None, af, segments=GOOD, mx_out=(c[:150], s, "mxfp6"), **kw)      # fewer rows than Sq
    # a malformed table is an error, not a decline
    with pytest.raises(_hip.ByaError, match="BYA_ERR_SHAPE"):
        ops.attn_kv_mix_segments_plan(z, af, segments=[(1, 0, 45), (2, 40, 70)], z_row=H * D, **kw)
    # more than 16 segments: the caller splits
    seventeen = [(0, 8 * i, 8) for i in range(17)]
    with pytest.raises(ValueError, match="at most 16"):
        ops.attn_kv_mix_segments_plan(z, af, segments=seventeen, z_row=H * D, **kw)
    with pytest.raises(ValueError, match="at most 16"):
        ops.attn_kv_mix_segments(z, z, z, z, af, z, segments=seventeen, z_row=H * D, scale=0.125, **kw)
    assert ops.MIX_MAX_SEGMENTS == 16
    # a launch never takes meta tensors
    with pytest.raises((ValueError, AssertionError)):
        ops.attn_kv_mix_segments(z, z, z, torch.empty(160, 2, dtype=torch.bfloat16, device="meta"), af, z, segments=GOOD,
                                 z_row=H * D, scale=0.125, **kw)


def test_engine_switch_reads_its_variable():
    import inspect
    from bind_your_avatar_implementation_amd import engine
    src = inspect.getsource(engine.DenoiseEngine.__init__)
    assert 'self.sp_segment_mix = os.environ.get("BYA_SP_SEGMENT_MIX"' in src
