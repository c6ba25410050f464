"""Conditioning of the bf16 GEMMs (a plain helper module: no tests, no fixtures; the sibling of ``cond_gemm.py``, whose measure,
bars, restatement and ``check`` it uses as they stand).  The exact-data suite (tests/exact_gemm.py) draws A and W from integers
in [-3, 3] times 2^{-1, 0, 1} and every epilogue operand from a grid on which each product is a shift; here the operands are
built as bf16 BIT PATTERNS over the whole domain of include/bya.h ("Domain of the bf16 GEMMs") -- every finite bf16 value,
subnormals included -- the epilogue operands are off every grid, and each output element is held to the fp64 value of the
definition on those very bits.

DATA.  An operand is a dict: ``bits`` (int16 [rows, K], the bf16 bit patterns) and ``fam`` (index into FAMILIES per row);
``values`` gives the fp64 values.  The family changes every row (A: m mod 5, W: (n + 2) mod 5) and an output element belongs to
a family when its A row and its W row do, else to ``mixed`` (``cond_gemm.out_family``):
    near       A: N(0, 1) rounded to bf16; W: N(0, 1) / sqrt(K) rounded to bf16                       the control, 8-bit significands
    spread     sign * (128 + U[0, 127]) / 128 * 2^e, e uniform in [-12, 12] per element, 2 % of the 32-blocks all zero (both
               sides)                                                                                  sums ruled by a few products
    cancel     pairs (2j, 2j + 1): A holds one ``near`` value twice, W holds w and -w, one pair in eight nudged by one bf16 step:
               sum p is a few nudges while sum |p| is the whole row                                    fp32 accumulation exposed
    subnormal  A: only bf16 subnormals j * 2^-133, 1 <= |j| <= 127;  W: w * 2^120, w an integer in [-3, 3]
    extreme    A: only +- the largest finite bf16, 255 * 2^120;       W: w * 2^-120, w an integer in [-3, 3]
    one-hot    (launches of their own, N >= K) W row n holds ONE non-zero, at k = n mod K: 1.0 in the first launch, -0.5 in the
               second; A is dense, element (m, k) the finite bf16 bit pattern number (m K + k) * 251 mod 65280 (251 is coprime
               to 65280), so with M K >= 65280 every one of the 65280 finite patterns occurs.
    act-range  (only under an activation) A and W ``near``, the bias of column n = -30 + 60 n / (N - 1): the pre-activations
               cover [-30, 30] evenly, -13 .. -5 included, where 1 + tanh(u) cancels.
EXACT FAMILIES (the result must EQUAL bf16(fp64) bit for bit; ``exact_units_bf16`` restates the proofs on the generated bits):
    subnormal  a product is (j w) * 2^-13 with |j w| <= 127 * 3 = 381: an integer of at most 381 units of 2^-13; every partial
               sum of K of them is below 381 K <= 381 * 12288 < 2^24 units: exact in fp32 in any order.  A kernel or matrix
               instruction that flushes bf16 subnormal inputs changes every element.
    extreme    a product is (+-255 w) units of 1, |255 w| <= 765, and 765 * 12288 < 2^24.
    one-hot    the output is A[m, n mod K] itself (bit for bit, subnormals and the largest values included), or -0.5 times it:
               one product of at most 9 significant bits, exact in fp32, so fp64 -> fp32 -> bf16 rounds once.
OUTSIDE THE DOMAIN.  The domain asks that every partial sum, in any K order, stay within fp32's finite range; S0 = sum_k |a_k w_k|
bounds every such partial sum.  An ``extreme`` A row (3.4e38) under a ``near`` W row, or a ``near`` A row under a ``subnormal`` W row
(3 * 2^120), leaves it, so an element with S0 >= 2^126 (a factor 4 below overflow: the epilogue multiplies by at most 1.5 and adds
operands of order 1) belongs to NO family (index OUTSIDE = -1, which ``cond_gemm.figures`` does not look at): its value is not
specified.  Only ``mixed`` elements are ever taken out; tests/test_gemm_bf16_cond_cpu.py asserts that no element of the five row
families reaches the limit (a one-hot element IS one product, finite whatever its size).
UNDERFLOW.  ``cond_gemm``'s eps is relative to S.  A ``subnormal`` A row under a ``near`` W row gives products and sums below 2^-126,
where an fp32 operation rounds to a multiple of 2^-149 whatever its operands' size: the bar gets the absolute term
T_under = 2 (2 K + ops) 2^-149 (K products, K additions and the epilogue's operations, each allowed to truncate; the factor 2
covers gates of at most 1.5 times an activation slope of at most 1.13).  At an ulp of 2^-133, the smallest ``cond_gemm._ulp``
gives, that is 2 * 1028 * 2^-16 = 0.03 ulp at K = 512; 0.75 ulp at K = 12288; nothing where results are normal numbers.

EPILOGUES.  The seven of ``cond_gemm.EPILOGUES`` on ``cond_gemm.make_epilogue``'s operands (``batch2`` with a residual that
aliases the output), ``gate-alpha`` (two gates and alpha 0.3: under the issue's alpha of 0.5 a gate multiplied with alpha in bf16
is exact and would not show) and ``res-cancel``: bias, two gates, alpha 0.5 and a residual equal to the bf16 rounding of MINUS the
fp64 value before the residual, its magnitude nudged up by 0 .. 3 bf16 steps.  The result is a few steps of the large value:
a rounding of that value to bf16 before the residual add is an error of hundreds of ulps of the result.

BARS.  (a), (b), (c), (d) of ``cond_gemm``; under gelu_erf / silu / relu / leaky_relu with the slopes ``cond_gemm.reference``
derives.  (e), because (a) grows linearly in K (median eps on ``near``: 0.01 at K = 64, 0.23 at 512, 3.3 at 3072, 26 at 12288):
per family of at least 1000 elements, at K >= 1024 and without an activation, the rms of (got - y64) / ulp is at most 1.25 times
the largest rms among the restatement's orders (``rms_orders``: forward, reversed K, 128-step grouping).
The restatement: ``cond_gemm.accumulate32(group=32)`` (one v_mfma_f32_16x16x32_bf16 per 32 of K, its sum taken as exact) then
``cond_gemm.epilogue32``; for bya_gemm_skinny_bf16 ``accumulate_skinny`` (16 waves over the K ranges ksteps * w / 16, partials
added in wave order).

FIGURES of the first run on an MI355X: DESIGN.md, section 17.
"""
import functools

import torch

import cond_gemm as C
from exact_gemm import BF, GuardedOut

FAMILIES = C.ROW_FAMILIES + ("mixed", "one-hot", "act-range")
MIXED, ONE_HOT, ACT_RANGE, OUTSIDE = FAMILIES.index("mixed"), FAMILIES.index("one-hot"), FAMILIES.index("act-range"), -1
assert MIXED == C.MIXED                       # (cond_gemm.out_family writes that index)
EXACT = ("subnormal", "extreme", "one-hot")
SUB_LOG2, W_SUB_LOG2, W_TOP_LOG2 = -133, 120, -120       # subnormal A = j 2^-133; W = w 2^120 (subnormal) / w 2^-120 (extreme)
TOP_BITS = 0x7F7F                                         # the largest finite bf16, 255 * 2^120
DOMAIN_S0 = 2.0 ** 126
FINITE_CODES = 65280


def to_int16(x):
    """Bit patterns 0 .. 65535 (long) as int16."""
    x = x & 0xFFFF
    return torch.where(x >= 0x8000, x - 0x10000, x).to(torch.int16)


def bits_of(x):
    """The bf16 bit patterns (long, 0 .. 65535) of a float tensor rounded to bf16."""
    return x.to(BF).view(torch.int16).long() & 0xFFFF


def values(op):
    """fp64 of the operand's BITS."""
    return op["bits"].view(BF).double()


def finite_bits():
    c = torch.arange(0x10000)
    return c[((c >> 7) & 0xFF) != 0xFF]


def _bits_of_family(fam, side, rows, K, gen):
    """long [rows, K]: bf16 bit patterns of one row family (module docstring)."""
    sign = lambda: torch.randint(0, 2, (rows, K), generator=gen) << 15
    near = lambda n: torch.randn(rows, n, generator=gen) * (1.0 if side == "a" else K ** -0.5)
    if fam == "near":
        return bits_of(near(K))
    if fam == "spread":
        mant = 128 + torch.randint(0, 128, (rows, K), generator=gen)
        e = torch.randint(-12, 13, (rows, K), generator=gen)
        b = bits_of(torch.ldexp(mant.float() / 128.0, e)) | sign()
        zero = torch.rand(rows, K // 32, generator=gen) < 0.02
        return torch.where(zero[..., None].expand(rows, K // 32, 32).reshape(rows, K), torch.zeros_like(b), b)
    if fam == "cancel":
        b = bits_of(near(K // 2))[..., None].expand(rows, K // 2, 2).clone()
        if side == "w":
            b[..., 1] ^= 0x8000
            nudge = torch.rand(rows, K // 2, generator=gen) < 0.125
            b[..., 1] = torch.where(nudge, b[..., 1] + 1, b[..., 1])             # one bf16 step up in magnitude
        return b.reshape(rows, K)
    small = lambda log2: bits_of(torch.ldexp(torch.randint(-3, 4, (rows, K), generator=gen).float(), torch.tensor(log2)))
    if fam == "subnormal":
        return (torch.randint(1, 128, (rows, K), generator=gen) | sign()) if side == "a" else small(W_SUB_LOG2)
    assert fam == "extreme"
    return (TOP_BITS | sign()) if side == "a" else small(W_TOP_LOG2)


def build_operand_bf16(rows, K, side, seed, family=None):
    """One operand (A: side "a", W: side "w") as bf16 bit patterns, on the CPU from a seed: rows interleaved over
    ``cond_gemm.ROW_FAMILIES`` (A: m mod 5, W: (n + 2) mod 5), or every row of ``family`` ("near" for the act-range launches)."""
    gen = torch.Generator().manual_seed(seed)
    if family is not None:
        return dict(bits=to_int16(_bits_of_family("near", side, rows, K, gen)), fam=torch.full((rows,), FAMILIES.index(family)))
    fam = (torch.arange(rows) + (0 if side == "a" else 2)) % len(C.ROW_FAMILIES)
    bits = torch.zeros(rows, K, dtype=torch.long)
    for i, name in enumerate(C.ROW_FAMILIES):
        sel = fam == i
        if int(sel.sum()):
            bits[sel] = _bits_of_family(name, side, int(sel.sum()), K, gen)
    return dict(bits=to_int16(bits), fam=fam)


def build_one_hot_bf16(M, N, K, w_value=1.0):
    """-> (A, W) of the one-hot family: needs N >= K; with M K >= 65280 every finite bf16 bit pattern occurs in A."""
    assert N >= K
    fin = finite_bits()
    assert len(fin) == FINITE_CODES
    m, k = torch.arange(M)[:, None], torch.arange(K)[None]
    a = dict(bits=to_int16(fin[((m * K + k) * 251) % FINITE_CODES]), fam=torch.full((M,), ONE_HOT))
    n = torch.arange(N)
    w = torch.zeros(N, K)
    w[n, n % K] = w_value
    return a, dict(bits=to_int16(bits_of(w)), fam=torch.full((N,), ONE_HOT))


def act_range_bias(N):
    return torch.linspace(-30.0, 30.0, N, dtype=torch.float64).to(BF)


def exact_units_bf16(a, w, fam):
    """The integer proof of an exact family on the generated bits: -> (long [Ma, Nw, K] products in units of 2^log2, log2).  Asserts
    what the module docstring states: A and W are the integers they should be and the sum of the products' magnitudes -- so
    every partial sum in every order -- is below 2^24 units."""
    i = FAMILIES.index(fam)
    ra, rw = a["bits"][a["fam"] == i].long() & 0xFFFF, values(dict(bits=w["bits"][w["fam"] == i]))
    if fam == "subnormal":
        assert bool(((ra & 0x7F80) == 0).all()) and bool(((ra & 0x7F) >= 1).all()), "A: subnormal patterns only"
        ia = torch.where(ra >= 0x8000, -(ra & 0x7F), ra & 0x7F)                     # j: the value is j * 2^-133
        iw, unit, per = torch.ldexp(rw, torch.tensor(-W_SUB_LOG2)), SUB_LOG2 + W_SUB_LOG2, 127 * 3
    else:
        assert bool(((ra & 0x7FFF) == TOP_BITS).all()), "A: +- the largest finite bf16 only"
        ia = torch.where(ra >= 0x8000, -255, 255)                                   # the value is +-255 * 2^120
        iw, unit, per = torch.ldexp(rw, torch.tensor(-W_TOP_LOG2)), 120 + W_TOP_LOG2, 255 * 3
    assert torch.equal(iw, iw.round()) and float(iw.abs().max()) <= 3
    K = ra.shape[1]
    prod = ia[:, None, :] * iw.long()[None, :, :]
    assert int(prod.abs().max()) <= per and int(prod.abs().sum(-1).max()) <= per * K < 2 ** 24
    return prod, unit


def family_of(a, w, a64, w64):
    """[rows, N] index into FAMILIES, OUTSIDE (-1) where S0 = sum_k |a_k w_k| >= 2^126 (module docstring).  On a64's device."""
    fam = C.out_family(a, w).to(a64.device)
    return torch.where((fam == MIXED) & (a64.abs() @ w64.abs().T >= DOMAIN_S0), torch.full_like(fam, OUTSIDE), fam)


def underflow_term(K, ops=0):
    return 2.0 * (2 * K + ops) * 2.0 ** -149


# ------------------------------------------------------------------------------------------------------------- epilogues
EPILOGUES = dict(C.EPILOGUES)
EPILOGUES["batch2"] = dict(bias=True, res=True)                      # (the residual aliases the output)
EPILOGUES["gate-alpha"] = dict(gates=True, alpha=0.3)               # alpha no power of two: gate * alpha has no exact bf16 product
EPILOGUES["res-cancel"] = dict(bias=True, gates=True, alpha=0.5)
RES_CANCEL_STEPS = 8


def make_epilogue_bf16(which, M, N, seed, a64=None, w64=None, batch=1, act=None, act_range=False):
    """``cond_gemm.make_epilogue`` of EPILOGUES[which] (None: no epilogue but ``act``); ``act_range``: the bias of
    ``act_range_bias``; "res-cancel" (needs the operands' values): the residual of the module docstring, zero where the element
    is outside the domain."""
    kw = dict(EPILOGUES[which]) if which else {}
    if act is not None:
        kw.update(bias=True, act=act)
    e = C.make_epilogue(M, N, seed, batch=batch, **kw)
    if act_range:
        e["bias"] = act_range_bias(N)
    if which == "res-cancel":
        y, _ = C.reference(a64, w64, e, M)
        steps = torch.randint(0, 4, y.shape, generator=torch.Generator().manual_seed(seed + 1))
        inside = (a64.abs() @ w64.abs().T < DOMAIN_S0) & torch.isfinite((-y).to(BF).float())
        res = to_int16(bits_of(-y) + steps).view(BF)
        e["res"] = torch.where(inside, res, torch.zeros_like(res))
    return e


# ------------------------------------------------------------------------------------------------------------ restatements
def rms_orders(a64, w64, e=C.NO_EPILOGUE, M=None):
    """The three restatement orders bar (e) takes its maximum over: forward, reversed K, 128-step grouping."""
    return [C.restate(a64, w64, e, M), C.restate(a64, w64, e, M, reverse=True), C.restate(a64, w64, e, M, group=128)]


def accumulate_sequential(a64, w64):
    """fp32, one product at a time in K order, no blocks (each product is exact in fp32 or rounded once)."""
    acc = torch.zeros(a64.shape[0], w64.shape[0], dtype=torch.float32, device=a64.device)
    for k in range(a64.shape[1]):
        acc = acc + (a64[:, k, None] * w64[None, :, k]).float()
    return acc


def accumulate_slices(a64, w64, n=4):
    """``n`` accumulators over contiguous K slices (each ``cond_gemm.accumulate32``), added pairwise at the end."""
    K = a64.shape[1]
    cut = [((K // 32) * i // n) * 32 for i in range(n + 1)]
    parts = [C.accumulate32(a64[:, lo:hi], w64[:, lo:hi]) for lo, hi in zip(cut[:-1], cut[1:]) if hi > lo]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def accumulate_skinny(a64, w64):
    """bya_gemm_skinny_bf16's order (csrc/gemm.hip gemm_skinny_kernel): wave w of 16 sums the 32-steps [ksteps w / 16,
    ksteps (w + 1) / 16) into its own fp32 accumulator, the 16 partials are added in wave order to 0."""
    ksteps = a64.shape[1] // 32
    v = torch.zeros(a64.shape[0], w64.shape[0], dtype=torch.float32, device=a64.device)
    for wave in range(16):
        lo, hi = ksteps * wave // 16 * 32, ksteps * (wave + 1) // 16 * 32
        v = v + (C.accumulate32(a64[:, lo:hi], w64[:, lo:hi]) if hi > lo else torch.zeros_like(v))
    return v


# --------------------------------------------------------------------------------------------------------- the GPU matrix
# path -> (options that force it, first column of the output view, M one off a multiple of the tile height, N, the K lengths).
# N = 260 where the path admits N % 8 != 0; the persistent kernels decline fewer than 3 (p256) / 4 (p128, p128s) K-tiles -- such
# a launch runs on w8_256, which has its own row -- so they take the nearest lengths their plan query accepts.
PATHS = {
    "t128x64": (dict(gemm_tile=0), 8, 257, 260, (64, 192, 512)),
    "t128x128": (dict(gemm_tile=1), 8, 129, 260, (64, 192, 512)),
    "t256x128": (dict(gemm_tile=2), 8, 255, 260, (64, 192, 512)),
    "t256x256": (dict(gemm_tile=3), 8, 511, 260, (64, 192, 512)),
    "p256": (dict(gemm_tile=4), 8, 257, 264, (192, 512)),
    "w8_256": (dict(gemm_tile=4), 4, 255, 264, (64, 192, 512)),
    "p128": (dict(gemm_tile=5), 8, 129, 264, (256, 512)),
    "p128s": (dict(gemm_tile=6), 8, 129, 264, (256, 512)),
}
LONG_K_PATHS, LONG_K_SHAPES = ("t128x128", "p256", "p128s"), ((130, 128, 3072), (130, 128, 12288))
ONE_HOT_SHAPE = (300, 512, 512)
EPI_SHAPE = (300, 264, 512)
ACTS_T128 = ("gelu_erf", "silu", "relu", "leaky_relu")
SKINNY_ACTS = ("gelu_tanh", "gelu_erf", "relu", "silu", "leaky_relu", "gelu_tanh_ieee")
SKINNY_ROWS = ((1, 1), (1, 15), (1, 17), (1, 64), (2, 15), (2, 64))      # (B, M) of test_gemm_exact_gpu.SKINNY_CASES
SKINNY_N, SKINNY_KS = 272, (256, 512, 3072)
SPLITK = {"splitk1": (4000, 1536, 1024, dict(gemm_splitk=1, gemm_splitk_min=8, gemm_tile=4)),
          "splitk2": (2222, 3072, 3072, dict(gemm_splitk=2, gemm_splitk_min=8, gemm_tile=4))}
# the smallest launch (fewest output elements) whose plan, under the library's default options, has a row split (m0 > 0): 103 x 3
# tiles of 256 x 256 = one full round of 256 + 53, m0 = 85 row tiles = 21760; K < 1024 stays on the 128 x 128 kernel.
# test_gemm_bf16_cond_cpu.py searches the plan query on meta tensors and asserts this.  2^23.7 output elements: checked whole.
ROW_SPLIT_SHAPE = (26113, 520, 1024)
ROW_SPLIT_KEY = "p256|p128s"
ROWGEMM = ((2049, 512, "w_stationary"), (1000, 512, "chunk_balanced"), (127, 1536, "chunk_balanced"))
ROWGEMM_MODES = ("plain", "res", "gelu_erf")
GELU_ERF_F_ERROR = 1.5e-7                      # rowk::gelu_erf_f (csrc/rowgemm_common.h): |erf error| <= 1.5e-7


def case(path, M, N, K, group="mid", which=None, act=None, batch=1, parts=1, alias=False, opts=None, key=None, col0=None):
    """One launch of the matrix.  ``group``: "mid" (the five row families), "one-hot", "one-hot-neg", "act-range"."""
    o, c0 = PATHS[path][:2]
    return dict(path=path, key=key or path, opts=dict(o if opts is None else opts), col0=c0 if col0 is None else col0, M=M, N=N, K=K,
                group=group, which=which, act=act, batch=batch, parts=parts, alias=alias,
                id=f"{key or path}-{batch}x{M}x{N}x{K}-{group}" + (f"-{which}" if which else "") + (f"-{act}" if act else ""))


def smallest_k(path):
    return PATHS[path][4][0]


def plain_cases():
    out = [case(p, M, N, K) for p, (_, _, M, N, Ks) in PATHS.items() for K in Ks]
    return out + [case(p, *s) for p in LONG_K_PATHS for s in LONG_K_SHAPES]


def one_hot_cases():
    return [case(p, *ONE_HOT_SHAPE, group=g) for p in PATHS for g in ("one-hot", "one-hot-neg")]


def epilogue_cases():
    M, N, K = EPI_SHAPE
    out = []
    for p in PATHS:
        for which in EPILOGUES:
            out.append(case(p, M, N, K, which=which, batch=2 if which == "batch2" else 1, parts=3 if which == "split3" else 1,
                            alias=which == "batch2", act="gelu_tanh" if which == "gelu" else None))
        out.append(case(p, M, N, smallest_k(p), which="res-cancel"))
    return out


def activation_cases():
    M, N, K = EPI_SHAPE
    return ([case(p, M, N, K, group="act-range", act="gelu_tanh") for p in PATHS]
            + [case("t128x128", M, N, K, group="act-range", act=a) for a in ACTS_T128])


def splitk_cases():
    return [case("p256", M, N, K, which="gate_res", alias=True, opts=o, key="p256+splitk") for M, N, K, o in SPLITK.values()]


def row_split_cases():
    return [case("p256", *ROW_SPLIT_SHAPE, which="gate_res", opts={}, key=ROW_SPLIT_KEY)]


def skinny_cases():
    out = [dict(B=B, M=M, K=K, act=None, group="mid") for B, M in SKINNY_ROWS for K in SKINNY_KS]
    out += [dict(B=2, M=15, K=512, act=a, group="act-range") for a in SKINNY_ACTS]
    out += [dict(B=1, M=64, K=SKINNY_N - SKINNY_N % 32, act=None, group=g) for g in ("one-hot", "one-hot-neg")]   # (N >= K)
    for c in out:
        c["id"] = f"skinny-{c['B']}x{c['M']}x{SKINNY_N}x{c['K']}-{c['group']}" + (f"-{c['act']}" if c["act"] else "")
    return out


def tiled_cases():
    return plain_cases() + one_hot_cases() + epilogue_cases() + activation_cases() + splitk_cases() + row_split_cases()


@functools.lru_cache(maxsize=4)
def data(M, N, K, group, batch=1):
    """(A, W) of a case on the CPU (cached: read-only)."""
    if group.startswith("one-hot"):
        return build_one_hot_bf16(batch * M, N, K, -0.5 if group.endswith("neg") else 1.0)
    seed = C.seed_of(f"bf16-{M}x{N}x{K}-{group}")
    family = "act-range" if group == "act-range" else None
    return build_operand_bf16(batch * M, K, "a", seed, family), build_operand_bf16(N, K, "w", seed + 1, family)


@functools.lru_cache(maxsize=4)
def epilogue_of(M, N, K, group, which, act, batch=1):
    """The case's epilogue operands on the CPU (cached: ``res-cancel`` costs an fp64 product)."""
    if not which and not act:
        return C.NO_EPILOGUE
    a, w = data(M, N, K, group, batch)
    return make_epilogue_bf16(which, M, N, C.seed_of(f"bf16-{M}x{N}-{which}"), values(a) if which == "res-cancel" else None,
                              values(w) if which == "res-cancel" else None, batch, None if which == "gelu" else act,
                              act_range=group == "act-range")


def launch_args(dev, c, a=None, w=None, e=None):
    """-> (A, W, GuardedOut, keyword arguments) of ``ops.gemm`` / ``ops.gemm_plan`` for case ``c``.  On the meta device (the plan
    queries of the CPU file) only shapes, strides and view offsets: no data is built."""
    meta = str(dev) == "meta"
    M, N, K, B = c["M"], c["N"], c["K"], c["batch"]
    put = (lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")) if meta else (lambda t: t.to(dev))
    A = torch.empty(B * M, K, dtype=BF, device="meta") if meta else a["bits"].view(BF).to(dev)
    W = torch.empty(N, K, dtype=BF, device="meta") if meta else w["bits"].view(BF).to(dev)
    A = A.reshape(B, M, K) if B > 1 else A
    if e is None:                                             # (meta: stand-ins with the same pointers set)
        kw = dict(EPILOGUES[c["which"]]) if c["which"] else {}
        if c["act"]:
            kw.update(bias=True, act=c["act"])
        e = C.make_epilogue(M, N, 0, batch=B, **kw)
    out = GuardedOut(M, N, dev, batch=B, parts=c["parts"], col0=c["col0"])
    kw = {k: put(e[k]) for k in ("bias", "gate0", "gate1") if e[k] is not None}
    if e["act"] is not None:
        kw["act"] = e["act"]
    if e["gate0"] is not None:
        kw["gate_split"] = e["gate_split"]
    if e["alpha"] != 1.0:
        kw["alpha"] = e["alpha"]
    if e["rowscale"] is not None:
        kw["bias_rowscale"] = put(e["rowscale"])
    if e["res"] is not None:
        res = put(e["res"])
        res = res.reshape(B, M, N) if B > 1 else res
        if c["alias"]:
            if not meta:
                out.fill(res)
            kw["res"] = out.view()
        else:
            kw["res"] = res
    if c["parts"] > 1:
        kw["split"] = out.split
    return A, W, out, kw


def check_result(name, got, a, w, e, M, K, dev, plan=None, restated=None, exact=None, extra_T=0.0, out=print):
    """``cond_gemm.check`` of one launch's result ``got`` [rows, N] against fp64 on ``dev``: the reference, the family table with
    the elements outside the domain taken out, the restatement (``restated``: a function (a64, w64, e, M) -> bf16; default
    ``cond_gemm.restate``), the underflow term, and at K >= 1024 without an activation the orders of bar (e)."""
    a64, w64 = values(a).to(dev), values(w).to(dev)
    e = C.epilogue_to(e, dev)
    y64, S = C.reference(a64, w64, e, M)
    fam = family_of(a, w, a64, w64)
    ops_n = C.epilogue_ops(e)
    orders = rms_orders(a64, w64, e, M) if K >= 1024 and e["act"] is None else None
    rest = orders[0] if orders and restated is None else (restated or C.restate)(a64, w64, e, M)
    plain = e is C.NO_EPILOGUE or all(e[k] is None for k in ("bias", "act", "gate0", "res", "rowscale")) and e["alpha"] == 1.0
    return C.check(name, got, y64, S, K, fam, restated=rest, ops=ops_n, act=e["act"], plan=plan,
                   exact=(EXACT if plain else ()) if exact is None else exact, T=underflow_term(K, ops_n) + extra_T,
                   families=FAMILIES, rms_of=orders, out=out)


def run_gemm(ops, dev, c, out=print):
    """One launch of ``ops.gemm`` for case ``c``: the plan asserted BEFORE the launch, under the case's options; then the guard
    band, the workspace status and ``check_result``."""
    M, N, K, B = c["M"], c["N"], c["K"], c["batch"]
    a, w = data(M, N, K, c["group"], B)
    e = epilogue_of(M, N, K, c["group"], c["which"], c["act"], B)
    A, W, guard, kw = launch_args(dev, c, a, w, C.epilogue_to(e, dev))
    with ops.options(**c["opts"]):
        plan = ops.gemm_plan(A, W, guard.view(), **kw)
        assert ops.plan_key(plan) == c["key"], (c["id"], plan)
        if c["key"] == ROW_SPLIT_KEY:
            assert plan["m0"] > 0, plan
        ops.gemm(A, W, guard.view(), **kw)
    torch.cuda.synchronize()
    assert guard.guard_intact(), f"{c['id']}: a write outside the output view"
    assert ops.gemm_workspace_status() == 0
    return check_result(c["id"], guard.gathered().reshape(B * M, N), a, w, e, M, K, dev, plan=plan, out=out)


def run_skinny(ops, dev, c, out=print):
    B, M, K, N = c["B"], c["M"], c["K"], SKINNY_N
    cc = dict(M=M, N=N, K=K, batch=B, parts=1, col0=8, alias=False, which=None, act=c["act"])
    a, w = data(M, N, K, c["group"], B)
    e = epilogue_of(M, N, K, c["group"], None, c["act"], B)
    A, W, guard, kw = launch_args(dev, cc, a, w, C.epilogue_to(e, dev))
    with ops.weight_streaming():
        plan = ops.gemm_plan(A, W, guard.view(), **kw)
        assert plan["path"] == "skinny", (c["id"], plan)
        ops.gemm(A, W, guard.view(), **kw)
    torch.cuda.synchronize()
    assert guard.guard_intact(), f"{c['id']}: a write outside the output view"
    restated = lambda a64, w64, e, M: C.epilogue32(accumulate_skinny(a64, w64), e, M)
    return check_result(c["id"], guard.gathered().reshape(B * M, N), a, w, e, M, K, dev, plan=plan, restated=restated, out=out)


def run_rowgemm(ops, dev, M, N, form, mode, out=print):
    """bya_rowgemm512 without LayerNorm (out = res + act(x @ W.T + b), K = 512) on the five row families: the kernel ``form``
    asserted through its plan query; ``mode``: "plain", "res" (the residual aliasing the output) or "gelu_erf", whose bar adds
    the absolute error rowk::gelu_erf_f states for its erf, 1.5e-7 |v| / ulp with v the pre-activation."""
    K = 512
    a, w = data(M, N, K, "mid")
    e = C.make_epilogue(M, N, C.seed_of(f"rowgemm-{M}x{N}"), bias=True, res=mode == "res", act="gelu_erf" if mode == "gelu_erf" else None)
    ed = C.epilogue_to(e, dev)
    x, wt = a["bits"].view(BF).to(dev), w["bits"].view(BF).to(dev)
    guard = GuardedOut(M, N, dev, col0=8)
    res = None
    if mode == "res":
        guard.fill(ed["res"])
        res = guard.view()
    pack = ops.pack_rowgemm512(wt, ed["bias"])
    with ops.options(reference_forms=["rowgemm_chunked"] if form == "chunk_balanced" and M >= 2048 and N == 512 else []):
        plan = ops.rowgemm512_plan(x, N, guard.view(), ln=False, res=res, act=e["act"])
        assert plan["form"] == form and not plan["ln"] and plan["res"] == (mode == "res") and plan["gelu"] == (mode == "gelu_erf"), plan
        ops.rowgemm512(x, pack, guard.view(), res=res, act=e["act"])
    torch.cuda.synchronize()
    assert guard.guard_intact(), "rowgemm512: a write outside the output view"
    extra = 0.0
    if mode == "gelu_erf":
        extra = GELU_ERF_F_ERROR * (values(a).to(dev) @ values(w).to(dev).T + ed["bias"].double()[None]).abs()
    return check_result(f"rowgemm512 {form} {M}x{N} {mode}", guard.gathered(), a, w, e, M, K, dev, plan=plan, exact=(),
                        extra_T=extra, out=out)
