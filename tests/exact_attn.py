"""Exact-data attention checking (a plain helper module for the attention tests; it defines no tests and no fixtures; the
sibling of ``exact_gemm.py``, whose ``GuardedOut`` / ``bad_elements`` / ``describe`` it reuses).

"Selected-set" data: softmax attention whose answer has a closed form that is exactly representable in bf16, so the check is
``torch.equal`` and a failure names the element.

Construction (``build``), per (batch, head) index bh and key/value variant (the level-2 batch of the perceiver pattern, the
identities of ``attn_kv_mix``):
  * the Skv keys are cut into T sets by a seeded permutation, so the members of a set lie in different 64-key tiles, different
    stream-K pieces, some in the ragged last tile.  Query row i selects set (i + shift[bh]) % T: with Sq >= T every key is
    selected by some row of every (batch, head) -- every K row and every V row is load-bearing.  (T >= Skv / max_set; a case
    with fewer rows than that cannot cover its keys, ``covers`` says so.)
  * inside a set the scores, in exp2 units, are small integers at or below the set's top score whose weights 2^level sum to a
    power of two (``pattern``): (0), (0,0), (0,-1,-1), (0,-1,-2,-2), ..., and for 9..32 members x keys at 0 and y at -1 with
    x + y / 2 a power of two.  P / l of a selected key is 2^-k, k <= 5.
  * q and k carry the set as a positional code of ``m`` digits in base B (one coordinate per digit value: q has ``a`` there, k has
    ``b``; a, b small integers), so q . k = a b * (digits on which the two sets agree): a b m for the row's own set, at most
    a b (m - 1) for every other key -- GAP = a b = 32 (m = 2, up to B^2 sets) or 28 (m = 3).  (+-1 Hadamard codes give the same
    with one gap for at most D sets; random +-1 codes beyond that spread the other keys over more than the 176 units a bound of
    88 leaves.  Digits keep the whole score range at m GAP + 5 for up to 8000 (D = 64) sets.)  One coordinate carries the key's
    level (q: 1), one a constant offset (q: 1, k: the offset) that places the top score; the last two coordinates cancel
    (2 * 1 - 1 * 2) so that they are read too.  All entries are integers of magnitude <= 256: exact in bf16, every score an exact
    integer in fp32 in any order.
  * V holds integers 1..vmax times a sign that depends on the column only, rotated by bh and by the variant, so a head / batch /
    identity mix-up shows.  The expected output sum_j w_j v_j is a multiple of 1/32 of magnitude in [1, 7]: never zero (all terms
    of a column share the sign), 8 significant bits at most: exact in bf16.
  * three placements of the top score: 1 -- top 0 (a padding key counted at score 0 doubles a row sum); 2 -- top at +88 (static
    bound) or +200 (running maximum: the rescale branch runs whenever the set's keys arrive after the first tile, and a level
    -1 / -2 key followed by its level-0 key steps under the lazy-rescale threshold of 6); 3 -- top at -21 with everything else
    down to -88 (static bound, m = 2 only) or -150 (running maximum): every real score far below 0.

Why equality is the bar: the expected value e is a bf16 number, the nearest rounding boundary is >= 2^-9 |e| away.  The keys
outside the set add at most (keys that share a digit) * 2^-GAP relative, ``scale * log2 e`` != 1 and v_rcp / v_exp a few fp32 ulps.
The data condition checked in test_attn_exact_cpu.py: the fp64 softmax of the same q, k, v is within 2^-16 |e| of the closed form,
which leaves a factor 128 for a correct kernel's fp32 arithmetic.

``scale``: the kernels that scale themselves compute float(scale) * 1.4426950408889634f; ``UNIT_SCALE`` is the float for which
that product is exactly 1.0f (found by search at import; asserted).  attn_tiny uses exp(s * scale): ``LN2`` = float(ln 2), the
error (L <= 32 members, |s - max| <= 70) stays below 1e-5 relative, inside the margin above.

``mix_weights``: routing weights on an exact grid.  Face: r in {0, 1/4, 1/2, 1}, w = r.  Audio: af a permutation matrix and r in
{0, 1/2, 1} with at most one 1 and at most two 1/2 per token: av = af r is a copy of r, 1 - av in {1, 1/2, 0}, the products of
csrc/routing_weights.h stay in {0, 1/4, 1/2, 1} and every bf16 rounding of that chain is exact.  With sets of at most 3 keys
(P / l >= 1/4) and |v| <= 3, z = sum_id w_id O_id is a multiple of 1/16 of magnitude <= 12 (8 bits) and wsum a multiple of 1/4.
"""
import math

import numpy as np
import torch

from exact_gemm import BF, GuardedOut, bad_elements, describe, strided  # noqa: F401  (re-exported for the tests)

LOG2E_F = np.float32(1.4426950408889634)
LN2 = float(np.float32(math.log(2.0)))
BOUND = 88.0


def _unit_scale():
    s0 = np.float32(1.0) / LOG2E_F
    for step in range(-8, 9):
        s = s0
        for _ in range(abs(step)):
            s = np.nextafter(s, np.float32(2.0 if step > 0 else 0.0), dtype=np.float32)
        if np.float32(s) * LOG2E_F == np.float32(1.0):
            return float(s)
    return None


UNIT_SCALE = _unit_scale()
assert UNIT_SCALE is not None, "no float scale with scale * log2(e) == 1.0f: use 1 / log2(e) and the margin argument"

_SMALL = {1: [(0,)], 2: [(0, 0)], 3: [(0, -1, -1)], 4: [(0, -1, -2, -2), (0, 0, 0, 0)], 5: [(0, -1, -2, -3, -3)],
          6: [(0, 0, -1, -1, -1, -1)], 7: [(0, 0, -1, -1, -1, -2, -2)], 8: [(0,) * 8, (0, 0, -1, -1, -2, -2, -2, -2)]}


def pattern(n, pick=0):
    """Levels (<= 0) of an n-member set whose weights 2^level sum to a power of two; every P / l >= 1/32."""
    if n in _SMALL:
        return _SMALL[n][pick % len(_SMALL[n])]
    assert n <= 32
    p = 1 << (n.bit_length() - 1)
    return (0,) * (2 * p - n) + (-1,) * (2 * (n - p))


for _n in range(1, 33):
    for _pick in (0, 1):
        _w = [2.0 ** lv for lv in pattern(_n, _pick)]
        assert len(_w) == _n and math.log2(sum(_w)).is_integer() and min(_w) / sum(_w) >= 1 / 32 and max(_w) == 1


def n_sets(Sq, Skv, max_set):
    lo = -(-Skv // max_set)
    want = Skv if Skv <= 2 else -(-Skv // 3)
    return max(lo, min(want, Sq))


def build(Sq, Skv, D, nbh, dev, seed=0, nkv=1, placement=1, running=False, max_set=None, vmax=7, heads=None):
    """-> dict: q [nbh, Sq, D], k, v [nbh, nkv, Skv, D], want [nbh, nkv, Sq, D] (fp32 holding bf16-exact values), top, lo (the
    smallest score any pair can have), T, covers.  ``heads``: bh = b * heads + h shifts the row -> set map by 5 h + 11 b."""
    rng = np.random.RandomState(seed)
    ncode = D - 4
    two_digit = (ncode // 2) ** 2
    need_two = placement == 3 and not running            # the whole score range must fit between -88 and the top
    if max_set is None:
        max_set = 8 if Skv <= 8 * two_digit and not (need_two and Skv > 3 * two_digit) else 32
        if Sq < -(-Skv // max_set):                      # fewer rows than 8-key sets: larger sets keep every key selected
            max_set = 32
    T = n_sets(Sq, Skv, max_set)
    if need_two:
        T = min(T, two_digit)
    m = 2 if T <= two_digit else 3
    B = ncode // m
    assert -(-Skv // max_set) <= T <= B ** m, (T, B, m)
    a, b = (4, 8) if m == 2 else (4, 7)
    gap = a * b
    if running:
        top = {1: 0, 2: 200, 3: -150}[placement]
    else:
        # levels reach -3: the lowest score any pair can have is top - m a b - 3
        top = {1: 0, 2: int(BOUND) if m == 2 else 87, 3: -int(BOUND) + m * a * b + 3}[placement]
    offset = top - m * a * b
    assert abs(offset) <= 256
    code_of = torch.from_numpy(rng.permutation(B ** m)[:T].copy())
    digits = torch.stack([(code_of // B ** j) % B + j * B for j in range(m)], 1)          # [T, m] coordinates
    heads = heads or nbh
    shift = torch.tensor([(5 * (bh % heads) + 11 * (bh // heads)) % T for bh in range(nbh)])
    sel = (torch.arange(Sq)[None, :] + shift[:, None]) % T                                  # [nbh, Sq]
    q = torch.zeros(nbh, Sq, D)
    q.scatter_(2, digits[sel].reshape(nbh, Sq, m), float(a))
    q[..., D - 4], q[..., D - 3], q[..., D - 2], q[..., D - 1] = 1.0, 1.0, 2.0, -1.0
    sgn = torch.from_numpy(rng.choice([-1.0, 1.0], D)).float()
    rv = torch.from_numpy(rng.randint(0, vmax, (Skv, D)))
    k = torch.zeros(nbh, nkv, Skv, D)
    v = torch.zeros(nbh, nkv, Skv, D)
    want = torch.zeros(nbh, nkv, Sq, D)
    min_level = 0
    for bh in range(nbh):
        for c in range(nkv):
            sizes = np.full(T, Skv // T)
            sizes[:Skv % T] += 1
            half = T // 2
            delta = rng.randint(-1, 2, half)
            lo_, hi_ = sizes[:half] + delta, sizes[half:2 * half] - delta
            ok = (lo_ >= 1) & (lo_ <= max_set) & (hi_ >= 1) & (hi_ <= max_set)
            sizes[:half][ok], sizes[half:2 * half][ok] = lo_[ok], hi_[ok]
            sizes = sizes[rng.permutation(T)]
            assert sizes.sum() == Skv and sizes.min() >= 1 and sizes.max() <= max_set
            perm = rng.permutation(Skv)
            set_of = np.repeat(np.arange(T), sizes)                                        # set of perm[p]
            level = np.concatenate([pattern(int(n), int(rng.randint(2))) for n in sizes]).astype(np.float32)
            min_level = min(min_level, int(level.min()))
            keys = torch.from_numpy(perm)
            kk = torch.zeros(Skv, D)
            kk.scatter_(1, digits[torch.from_numpy(set_of)], float(b))
            kk[:, D - 4] = torch.from_numpy(level)
            kk[:, D - 3], kk[:, D - 2], kk[:, D - 1] = float(offset), 1.0, 2.0
            k[bh, c, keys] = kk
            v[bh, c] = sgn * (1 + (rv + bh + 3 * c) % vmax).float()
            # closed form: want[i] = sum over the members of the row's set of 2^level / (sum of the set's 2^level) * v
            wt = np.exp2(level)
            tot = np.zeros(T, np.float32)
            np.add.at(tot, set_of, wt)
            wkey = torch.zeros(Skv)
            wkey[keys] = torch.from_numpy(wt / tot[set_of])
            starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
            for j in range(int(sizes.max())):
                has = torch.from_numpy(sizes > j)
                member = torch.from_numpy(perm[np.minimum(starts + j, Skv - 1)])           # [T] key j of every set
                mj, hj = member[sel[bh]], has[sel[bh]]
                want[bh, c] += torch.where(hj[:, None], wkey[mj][:, None] * v[bh, c, mj], torch.zeros(()))
    out = dict(q=q, k=k, v=v, want=want)
    out = {n: t.to(dev) for n, t in out.items()}
    out.update(top=top, lo=top - m * a * b + min_level, T=T, covers=Sq >= T, gap=gap, m=m)
    return out


def reference(q, k, v, rows=None, chunk=1024):
    """fp64 softmax attention of ONE (batch, head), scores in exp2 units: q [Sq, D], k, v [Skv, D] -> (o [rows, D] fp64, min
    score, max score), chunked over the query rows so that 17776 keys fit."""
    qd, kd, vd = q.double(), k.double(), v.double()
    rows = torch.arange(q.shape[0], device=q.device) if rows is None else rows
    outs, smin, smax = [], math.inf, -math.inf
    for r0 in range(0, len(rows), chunk):
        s = qd[rows[r0:r0 + chunk]] @ kd.T
        smin, smax = min(smin, float(s.min())), max(smax, float(s.max()))
        p = torch.exp2(s - s.max(-1, keepdim=True).values)
        outs.append((p @ vd) / p.sum(-1, keepdim=True))
    return torch.cat(outs), smin, smax


def assert_exact(got, want, what=""):
    """``got`` (bf16) must equal ``want`` (fp32 holding bf16-exact values) bit for bit; the message names the first bad element,
    the bounding box and ``what`` (case and plan)."""
    ref = want.to(BF)
    assert torch.equal(ref.float(), want.float()), f"{what}: the closed form is not representable in bf16"
    bad = bad_elements(got, ref)
    assert not bool(bad.any()), f"{what}: {describe(bad, got, ref)}"


# ---------------------------------------------------------------------------------------------- attn_kv_mix weights
def mix_weights(rows, n_id, audio, dev, seed=0):
    """-> (r bf16 [rows, n_id], af bf16 [n_id, n_id] or None, w fp32 [rows, n_id]) on the exact grid of the module docstring;
    every row has at least one non-zero weight."""
    rng = np.random.RandomState(seed)
    if not audio:
        r = rng.choice([0.0, 0.25, 0.5, 1.0], (rows, n_id))
        r[np.arange(rows), rng.randint(n_id, size=rows)] = rng.choice([0.25, 0.5, 1.0], rows)
        r = torch.from_numpy(r).float()
        return r.to(BF).to(dev), None, r.to(dev)
    base = [(1.0, 0.0, 0.0, 0.0), (0.5, 0.0, 0.0, 0.0), (0.5, 0.5, 0.0, 0.0), (1.0, 0.5, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0),
            (1.0, 0.5, 0.5, 0.0)]
    r = np.array([rng.permutation(base[rng.randint(6 if n_id > 2 else 5)][:n_id]) for _ in range(rows)])
    af = np.eye(n_id)[rng.permutation(n_id)]
    r, af = torch.from_numpy(r).float(), torch.from_numpy(af).float()
    # csrc/routing_weights.h: av = af r, om = 1 - av, w[a] = prod over b != a of om[b], every step rounded to bf16
    om = (1.0 - (r @ af.T).to(BF).float()).to(BF).float()
    w = torch.ones(rows, n_id)
    for a_ in range(n_id):
        for b_ in range(n_id):
            if b_ != a_:
                w[:, a_] = (w[:, a_] * om[:, b_]).to(BF).float()
    assert set(w.unique().tolist()) <= {0.0, 0.25, 0.5, 1.0} and bool((w.sum(1) > 0).all())
    return r.to(BF).to(dev), af.to(BF).to(dev), w.to(dev)


# ---------------------------------------------------------------------------------------------- the GPU matrix
# bya_attn_fwd.  kind: run (d64_running_max), pre (d64_prescaled_running_max), d128, w4 (static bound), dev (device bound).
# B = nb1, L2 = nb2 (q shared over it: stride 0), pad = extra elements per q/k/v row, col0 = first column of o in its buffer
# (8: 16-byte aligned, 4: only 8-byte aligned -> narrow stores), narrow = reference form attn_narrow_store, sk = the stream-K
# grid is expected (a workspace is registered), sk_opt = option attn_streamk.
def _a(name, kind, Sq, Skv, H, p=1, B=1, L2=1, pad=0, col0=8, narrow=False, sk=False, sk_opt=1):
    return dict(name=name, kind=kind, Sq=Sq, Skv=Skv, H=H, placement=p, B=B, L2=L2, pad=pad, col0=col0, narrow=narrow, sk=sk,
                sk_opt=sk_opt, D=128 if kind == "d128" else 64)


def _family(kind):
    w4 = kind in ("w4", "dev")
    return [
        _a(f"{kind}-kv40", kind, 40, 40, 8, p=1),
        _a(f"{kind}-one-tile", kind, 64, 64, 8, p=2),
        _a(f"{kind}-kv200", kind, 200, 200, 4, p=3, B=2),
        _a(f"{kind}-kv1350", kind, 1350, 1350, 8 if not w4 else 4, p=1, pad=24, col0=8),
        _a(f"{kind}-kv4133-q513", kind, 513, 4133, 4, p=2),
        _a(f"{kind}-kv4133-q1031-narrow", kind, 1031, 4133, 3, p=3, col0=4),
        _a(f"{kind}-cross-kv32-q127", kind, 127, 32, 6, p=1, B=2, L2=2, narrow=True),
        _a(f"{kind}-cross-kv32-q129", kind, 129, 32, 8, p=3, L2=3, pad=8),
        _a(f"{kind}-q1", kind, 1, 8, 8, p=2),
    ]


ATTN_CASES = sum((_family(kd) for kd in ("run", "pre", "d128", "w4", "dev")), []) + [
    # stream-K: the 4-rank shard's 12 heads at 17776 tokens (8 does not divide the 420 items: an XCD owns a contiguous eighth),
    # 5056 keys x 32 heads (320 items, whole heads per XCD), each also with the option off; 160 items: declined
    _a("w4-streamk-17776x12", "w4", 17776, 17776, 12, p=1, sk=True),
    _a("w4-streamk-off-17776x12", "w4", 17776, 17776, 12, p=1, sk_opt=0),
    _a("w4-streamk-5056x32", "w4", 5056, 5056, 32, p=3, sk=True),
    _a("w4-streamk-off-5056x32", "w4", 5056, 5056, 32, p=3, sk_opt=0),
    _a("w4-streamk-5056x32-narrow", "w4", 5056, 5056, 32, p=2, sk=True, col0=4),
    _a("dev-streamk-5056x32", "dev", 5056, 5056, 32, p=2, sk=True),
    _a("w4-160-items-declined", "w4", 5000, 5000, 16, p=2),
]
ATTN_KIND_VARIANT = {"run": "d64_running_max", "pre": "d64_prescaled_running_max", "d128": "d128_running_max",
                     "w4": "d64_static_bound_w4", "dev": "d64_device_bound_w4"}


def attn_case_key(c):
    """The plan key (ops.attention_plan_key) the case is meant to reach."""
    wide = c["col0"] % 8 == 0 and not c["narrow"]
    return ATTN_KIND_VARIANT[c["kind"]] + ("+streamk" if c["sk"] else "") + ("/wide" if wide else "/narrow")


def attn_case_data(c, dev, seed=0):
    running = c["kind"] in ("run", "pre", "d128")
    return build(c["Sq"], c["Skv"], c["D"], c["B"] * c["H"], dev, seed=seed + len(c["name"]), nkv=c["L2"], placement=c["placement"],
                 running=running, heads=c["H"])


# bya_attn_kv_mix: form = the expected plan; generic = reference form kv_mix_generic; col0 = 4: z only 8-byte aligned
def _m(name, D, H, n_id, grp, Sq, Skv, audio, form, generic=False, col0=8, pad=0):
    return dict(name=name, D=D, H=H, n_id=n_id, grp=grp, Sq=Sq, Skv=Skv, audio=audio, form=form, generic=generic, col0=col0, pad=pad)


MIX_CASES = [
    _m("audio-d64-2id", 64, 48, 2, 3, 150, 32, True, "mix32"),
    _m("audio-d64-3id-kv20", 64, 6, 3, 2, 333, 20, True, "mix32", pad=8),
    _m("audio-d64-4id", 64, 8, 4, 1, 97, 32, True, "mix32"),
    _m("face-d128-1id", 128, 16, 1, 2, 131, 32, False, "mix32"),
    _m("face-d128-2id", 128, 16, 2, 1, 300, 32, False, "mix32", pad=16),
    _m("face-d128-4id-big-lds", 128, 4, 4, 2, 77, 32, False, "mix32"),
    _m("face-d64-kv33", 64, 8, 2, 2, 200, 33, False, "one_tile"),
    _m("audio-d64-kv64", 64, 6, 3, 1, 129, 64, True, "one_tile"),
    _m("audio-d64-generic", 64, 8, 2, 2, 150, 32, True, "one_tile", generic=True),
    _m("face-d128-misaligned-z", 128, 4, 3, 2, 140, 32, False, "one_tile", col0=4),
    _m("face-d128-kv64", 128, 4, 2, 1, 257, 64, False, "one_tile"),
    _m("audio-d128-generic-4id", 128, 2, 4, 1, 65, 20, True, "one_tile", generic=True),
]


def mix_case_key(c):
    big = c["form"] == "mix32" and (c["n_id"] * 2 + 4) * 32 * c["D"] * 2 > 65536
    return f"{c['form']}_d{c['D']}" + ("+big_lds" if big else "")


def mix_case_data(c, dev, seed=0):
    """q [grp * H, Sq, D], k / v [grp * H, n_id, Skv, D], per-identity want, r, af, w, z_want [grp * H, Sq, D], wsum [grp * Sq]."""
    d = build(c["Sq"], c["Skv"], c["D"], c["grp"] * c["H"], dev, seed=seed + len(c["name"]), nkv=c["n_id"], placement=1 + len(c["name"]) % 3,
              running=True, max_set=3, vmax=3, heads=c["H"])
    r, af, w = mix_weights(c["grp"] * c["Sq"], c["n_id"], c["audio"], dev, seed=seed + 1)
    wg = w.view(c["grp"], 1, c["Sq"], c["n_id"]).expand(c["grp"], c["H"], c["Sq"], c["n_id"]).reshape(-1, c["Sq"], c["n_id"])
    d["z_want"] = torch.einsum("bisd,bsi->bsd", d["want"], wg)
    d.update(r=r, af=af, w=w, wsum=w.sum(1))
    return d


# bya_attn_tiny: temporal = rows (outer, member, inner) with outer_stride = L * n_inner, else multi-ID (outer_stride 0, n_outer 1);
# unaligned = the q / k / v views start 4 elements into their rows' 16-byte grid (generic kernel although L and heads would fit)
def _t(L, H, n_outer, n_inner, instance, temporal=True, unaligned=False):
    return dict(name=f"L{L}-h{H}-{n_outer}x{n_inner}" + ("-unaligned" if unaligned else "") + ("" if temporal else "-multi-id"),
                L=L, H=H, n_outer=n_outer, n_inner=n_inner, instance=instance, temporal=temporal, unaligned=unaligned)


TINY_CASES = [
    _t(2, 8, 1, 203, "tiny8<2>", temporal=False), _t(2, 16, 3, 7, "tiny8<2>"),
    _t(3, 8, 1, 150, "tiny8<3>", temporal=False), _t(3, 16, 2, 9, "tiny8<3>"),
    _t(13, 8, 2, 45, "tiny8<13>"), _t(13, 16, 1, 13, "tiny8<13>"),
    _t(25, 8, 2, 15, "tiny8<25>"), _t(25, 16, 1, 5, "tiny8<25>"),
    _t(1, 6, 1, 9, "generic<2>"), _t(2, 6, 1, 11, "generic<2>", temporal=False),
    _t(4, 6, 2, 5, "generic<4>"), _t(5, 6, 1, 7, "generic<16>"), _t(16, 6, 1, 3, "generic<16>"),
    _t(17, 6, 1, 3, "generic<32>"), _t(32, 6, 1, 2, "generic<32>"),
    _t(13, 8, 1, 9, "generic<16>", unaligned=True),
]


def tiny_case_data(c, dev, seed=0):
    """-> (qkv [rows + 2, 3 H 64 + 8] bf16 with q | k | v side by side, row ids [groups, L], want [rows, H * 64] fp32, touched mask)."""
    L, H, no, ni = c["L"], c["H"], c["n_outer"], c["n_inner"]
    groups = no * ni
    d = build(L, L, 64, groups * H, dev, seed=seed + len(c["name"]), placement=1 + (L % 3), running=True, heads=H)
    rows = no * L * ni if c["temporal"] else L * ni
    idx = (torch.arange(no)[:, None, None] * (L * ni if c["temporal"] else 0) + torch.arange(L)[None, None, :] * ni
           + torch.arange(ni)[None, :, None]).reshape(groups, L).to(dev)
    return d, rows, idx
