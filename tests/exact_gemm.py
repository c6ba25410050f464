"""Exact-data GEMM checking (a plain helper module for the GEMM tests; it defines no tests and no fixtures).

Operands whose every product and every fp32 partial sum is exact make a GEMM kernel's result a function of the data alone:
whatever the tile shape, K order, split or wave layout, a correct kernel returns the exact product rounded once to bf16, BIT FOR
BIT.  A fragment that lost a K-tile, a wave tile written twice or an element never written then fails outright, where a
relative-Frobenius bar of 1e-3 lets it pass (``test_gemm_exact_cpu.py`` plants both faults).

bf16 operands (``exact_operands``):
    A[m, k] = a * 2^ra[m],  W[n, k] = w * 2^rw[n],   a, w integers in [-3, 3],  ra, rw in {-1, 0, 1}
So every product of output (m, n) is an integer multiple of 2^(ra[m] + rw[n]) >= 2^-2 of magnitude <= 9 * 4, and any partial
sum of K <= 12288 of them is a multiple of 2^-2 below 12288 * 36 < 2^19, i.e. below 2^21 units: exact in fp32 (24-bit
significand) in every order.  Epilogue operands keep it so (``exact_epilogue``):
    bias[n] = b * 2^-2, b in [-16, 16];  bias_rowscale in {1/2, 1, 2};  alpha: any power of two;  gates in {1/2, 1};
    res[m, n] = r * 2^-3 * alpha * min(gate0[n], gate1[n]), r in [-64, 64]
acc + rowscale * bias (the fmaf of csrc/gemm_common.h) is a multiple of u = 2^-3 below 2^19 + 32 < 2^22 u; * alpha * gate
scales value and unit alike; + res is a multiple of u' = u * alpha * min gate >= u * alpha * gate / 2 below 2^23 u' + 64 u':
every value before the final rounding is exact in fp32, for K up to 12288.  The reference is the
same arithmetic in fp64 on the device, rounded to bf16 at the end (fp64 -> fp32 is exact here, so torch's two-step conversion
rounds once).

fp8 (``exact_fp8_operand``): e4m3 codes of {0, +-0.5, ..., +-3} with power-of-two row scales in [1/4, 4]: the kernel sums code
products (multiples of 1/4, at most 9) and applies the scales after, so the sum is a multiple of 1/4 below K * 9 (exact in fp32
up to K = 12288) and the scales only move its exponent; MX: ``exact_operand`` of test_mx_gpu.py and ``dequant_mx`` of
test_mx_cpu.py.

The fp8 product through the whole epilogue of bya_gemm_fp8 (``exact_fp8_epilogue``; tests/test_fp8_exact_*.py).  Write
S = a_scale[m] * w_scale[n] = 2^s, s in [-4, 4], and K <= 12288:
    acc          a multiple of 2^-2, |acc| <= 9 K <= 110592 < 2^17 (below 2^19 units): exact in every K order;
    acc * S      a power of two times acc: exact, a multiple of 2^(s - 2), at most 110592 * 2^s;
    + bias       bias[n] = b * 2^-2, |b| <= 16 (no bias_rowscale: bya_gemm_fp8's callers have none): a multiple of
                 u = 2^(min(s, 0) - 2), at most 110592 * 2^s + 4 -- (1769472 + 4) * 4 < 2^23 units at s = 4, below 2^19 units
                 for s < 0;
    * alpha * gate   alpha any power of two, gates in {1/2, 1}: value and unit scale alike;
    + res        res[m, n] = r * 2^-2 * alpha * max(gate0[n], gate1[n]), |r| <= 64 (one gate: that gate; none: 1): a multiple
                 of U = u * alpha * gate, whichever of the two gates row m takes (max gate >= gate, min(s, 0) <= 0), and at most
                 32 alpha * gate in magnitude.
So every value up to the final rounding is a multiple of U = 2^(min(s, 0) - 2) * alpha * gate[row type(m)][n] and at most
(110592 * 2^s + 36) * 2^(2 - min(s, 0)) <= 7078032 < 2^23 units of U in magnitude: exact in fp32, in every order, on every
kernel.  (The bf16 residual grid above, r * 2^-3 * alpha * MIN gate, is too fine for these scales: at s = 4 under the larger of two
different gates its unit is 2^-4 alpha * gate, and 110592 * 2^4 is 2^24.75 of those.  Random data stays far below that bound --
|acc| is of order 3 sqrt(K) -- so the four older fp8 cases of test_gemm_exact_gpu.py, which use it, are exact all the same; the
bound here holds for ANY codes of the set, which is what test_fp8_exact_cpu.py checks with a planted row and channel of all
3 x 3 at scale 4 x 4.)

Outputs are checked inside a guard band (``GuardedOut``): the view is poisoned with NaN before the launch, the rest of the buffer
(rows and columns around it, gaps between n_split outputs) holds a sentinel that must survive.
"""
import torch

BF = torch.bfloat16
POISON = 0x7FC0            # bf16 quiet NaN: what an element no kernel wrote still holds
SENTINEL = 0x7FA5          # bf16 NaN with a payload no arithmetic produces: the guard band
UNITS = (16, 64, 128, 256)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def pow2(shape, dev, seed, lo=-1, hi=1):
    """Powers of two 2^e, e uniform in [lo, hi], fp32."""
    e = torch.randint(lo, hi + 1, shape, generator=_gen(dev, seed), device=dev)
    return torch.ldexp(torch.ones(shape, device=dev), e)


def exact_operands(M, N, K, dev, seed=0, batch=1):
    """-> (A [batch, M, K] or [M, K], W [N, K]) bf16 on the exact grid of the module docstring."""
    shape_a = (batch, M, K) if batch > 1 else (M, K)
    a = torch.randint(-3, 4, shape_a, generator=_gen(dev, seed), device=dev).float()
    a = a * pow2(shape_a[:-1] + (1,), dev, seed + 1)
    w = torch.randint(-3, 4, (N, K), generator=_gen(dev, seed + 2), device=dev).float() * pow2((N, 1), dev, seed + 3)
    return a.to(BF), w.to(BF)


def exact_epilogue(w, dev, seed, bias=False, gates=False, alpha=1.0, res_rows=None, batch=1):
    """Epilogue operands on the grid of the module docstring for the weight ``w`` of ``exact_operands``.
    -> dict(bias=, gate0=, gate1=, res=) (None where not asked; res: fp32 values [batch, res_rows, N] to be placed by the caller)."""
    N = w.shape[0]
    unit = torch.full((N,), 2.0 ** -2, device=dev)       # the finest product grid, 2^(min ra + min rw)
    out = dict(bias=None, gate0=None, gate1=None, res=None)
    if bias:
        out["bias"] = (torch.randint(-16, 17, (N,), generator=_gen(dev, seed), device=dev).float() * unit).to(BF)
    gmin = torch.ones(N, device=dev)
    if gates:
        g0, g1 = pow2((N,), dev, seed + 1, -1, 0), pow2((N,), dev, seed + 2, -1, 0)
        out["gate0"], out["gate1"] = g0.to(BF), g1.to(BF)
        gmin = torch.minimum(g0, g1)
    if res_rows is not None:
        r = torch.randint(-64, 65, (batch, res_rows, N), generator=_gen(dev, seed + 3), device=dev).float()
        out["res"] = r * (unit * 0.5 * alpha * gmin)
    return out


def reference(a, w, bias=None, gate0=None, gate1=None, gate_split=0, res=None, rowscale=None, alpha=1.0):
    """fp64 on the device: res + gate * alpha * (a @ w.T + rowscale * bias)  ->  fp64 [(B,) M, N] (round with ``.to(bf16)``)."""
    y = a.double() @ w.double().T
    if bias is not None:
        rs = 1.0 if rowscale is None else rowscale.double().reshape(y.shape[:-1] + (1,))
        y = y + rs * bias.double()
    y = y * alpha
    if gate0 is not None:
        g1 = gate0 if gate1 is None else gate1
        if gate0.dim() == 2:                                  # per batch entry [B, N] (gate_batch_stride = N)
            gate0, g1 = gate0[:, None], g1[:, None]
        rows = torch.arange(y.shape[-2], device=y.device)[:, None]
        y = y * torch.where(rows < gate_split, gate0.double(), g1.double())
    if res is not None:
        y = y + res.double()
    return y


def strided(t, pad):
    """``t`` as a view of rows ``pad`` elements wider (row stride K + pad), same values; works on meta tensors too."""
    if not pad:
        return t
    wide = torch.zeros(*t.shape[:-1], t.shape[-1] + pad, dtype=t.dtype, device=t.device)
    wide[..., :t.shape[-1]] = t
    return wide[..., :t.shape[-1]]


class GuardedOut:
    """An output view [(B,) M, N] (or ``parts`` n_split outputs of N / parts columns each) inside a larger bf16 buffer whose
    other elements hold ``SENTINEL``; the view is poisoned with NaN.  ``col0``: first column of the view in the buffer (in
    elements: 4 makes the view 8- but not 16-byte aligned).  On the meta device it gives the same view geometry (the plan
    queries' stand-ins for the GPU cases)."""

    def __init__(self, M, N, dev, batch=1, parts=1, rows_before=3, rows_after=5, col0=8, gap=8, cols_after=8):
        self.M, self.N, self.batch, self.parts = M, N, batch, parts
        self.width = N // parts
        self.stride = self.width + gap                       # elements between the starts of consecutive outputs
        ld = col0 + parts * self.stride - gap + cols_after
        ld += (-ld) % 8                                      # ldc % 8 == 0 (16-byte row pitch; the view's offset sets the alignment)
        self.r0, self.c0 = rows_before, col0
        self.buf = torch.full((batch, rows_before + M + rows_after, ld), 0, dtype=torch.int16, device=dev)
        self.buf.fill_(SENTINEL)
        self.mask = torch.zeros(self.buf.shape, dtype=torch.bool, device=dev)
        for p in range(parts):
            c = col0 + p * self.stride
            self.buf[:, self.r0:self.r0 + M, c:c + self.width] = POISON
            self.mask[:, self.r0:self.r0 + M, c:c + self.width] = True
        self.bf = self.buf.view(BF)

    def view(self):
        """The first output (with ``parts`` > 1: pass split=(width, stride) to the GEMM)."""
        v = self.bf[:, self.r0:self.r0 + self.M, self.c0:self.c0 + self.width]
        return v if self.batch > 1 else v[0]

    @property
    def split(self):
        return (self.width, self.stride) if self.parts > 1 else None

    def gathered(self):
        """The outputs as one [(B,) M, N] bf16 tensor (parts side by side)."""
        cols = [self.bf[:, self.r0:self.r0 + self.M, self.c0 + p * self.stride:self.c0 + p * self.stride + self.width]
                for p in range(self.parts)]
        t = torch.cat(cols, dim=-1)
        return t if self.batch > 1 else t[0]

    def fill(self, values):
        """Write fp values [(B,) M, N] into the output (residual aliasing C)."""
        v = values.to(BF).reshape(self.batch, self.M, self.N)
        for p in range(self.parts):
            c = self.c0 + p * self.stride
            self.bf[:, self.r0:self.r0 + self.M, c:c + self.width] = v[..., p * self.width:(p + 1) * self.width]

    def guard_intact(self):
        return bool((self.buf[~self.mask] == SENTINEL).all())


def bad_elements(got, ref_bf16):
    """Mask of elements whose bits differ (+0 and -0 count as equal), [(B,) M, N]."""
    g, r = got.contiguous().view(torch.int16), ref_bf16.contiguous().view(torch.int16)
    zero = (g & 0x7FFF == 0) & (r & 0x7FFF == 0)
    return (g != r) & ~zero


def describe(bad, got, ref_bf16):
    """Failure text: count, first bad element, bounding box in units of 16 / 64 / 128 / 256 rows and columns."""
    idx = bad.nonzero()
    if idx.numel() == 0:
        return "no bad elements"
    first = tuple(int(v) for v in idx[0])
    rows, cols = idx[:, -2], idx[:, -1]
    r_lo, r_hi, c_lo, c_hi = int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())
    boxes = ", ".join(f"{u}: rows {r_lo // u}..{r_hi // u} cols {c_lo // u}..{c_hi // u}" for u in UNITS)
    return (f"{idx.shape[0]} of {bad.numel()} elements differ; first {first}: got {float(got[first]):g}, "
            f"want {float(ref_bf16[first]):g}; rows {r_lo}..{r_hi}, cols {c_lo}..{c_hi}; tile box ({boxes})")


def assert_exact(got, ref64, plan=None, what=""):
    """``got`` (bf16) must equal ``ref64`` rounded to bf16 bit for bit; the message names the tiles and the plan that ran."""
    ref = ref64.to(BF)
    bad = bad_elements(got, ref)
    assert not bool(bad.any()), f"{what} [plan {plan}]: {describe(bad, got, ref)}"


def exact_fp8_operand(rows, K, dev, seed):
    """-> (e4m3 codes uint8 [rows, K], fp32 power-of-two row scales [rows], dequantised fp64 [rows, K]): codes of
    {0, +-0.5, +-1, +-1.5, +-2, +-3}, scales 2^-2 .. 2^2 -- every code product a multiple of 1/4 of at most 9, every sum of
    them exact; with both scales applied an element product is a multiple of 2^-6 of at most 144."""
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0], device=dev)
    el = vals[torch.randint(0, len(vals), (rows, K), generator=_gen(dev, seed), device=dev)]
    codes = el.to(torch.float8_e4m3fn).view(torch.uint8)
    scale = pow2((rows,), dev, seed + 1, -2, 2)
    deq = codes.view(torch.float8_e4m3fn).double() * scale.double()[:, None]
    assert torch.equal(deq, el.double() * scale.double()[:, None])
    return codes, scale, deq


def exact_fp8_epilogue(N, dev, seed, bias=False, gates=None, alpha=1.0, res_rows=None, batch=1, batch_gates=False):
    """Epilogue operands of bya_gemm_fp8 on the grid of the module docstring ("The fp8 product through the whole epilogue").
    ``gates``: None, "one" (gate1 absent) or "two"; ``batch_gates``: gate vectors per batch entry, [batch, N] (the launch's
    gate_batch_stride is N).  -> dict(bias=, gate0=, gate1=, res=) (None where not asked; res: fp32 values
    [batch, res_rows, N] = r * 2^-2 * alpha * max gate, to be placed by the caller)."""
    out = dict(bias=None, gate0=None, gate1=None, res=None)
    if bias:
        out["bias"] = (torch.randint(-16, 17, (N,), generator=_gen(dev, seed), device=dev).float() * 2.0 ** -2).to(BF)
    gshape = (batch, N) if batch_gates else (N,)
    gmax = torch.ones(gshape, device=dev)
    if gates:
        g0 = pow2(gshape, dev, seed + 1, -1, 0)
        out["gate0"], gmax = g0.to(BF), g0
        if gates == "two":
            g1 = pow2(gshape, dev, seed + 2, -1, 0)
            out["gate1"], gmax = g1.to(BF), torch.maximum(g0, g1)
    if res_rows is not None:
        r = torch.randint(-64, 65, (batch, res_rows, N), generator=_gen(dev, seed + 3), device=dev).float()
        out["res"] = r * (0.25 * alpha * (gmax[:, None] if batch_gates else gmax))
    return out


def bf16_ulps(got, want64):
    """Error of ``got`` (bf16) against the bf16 rounding of ``want64`` in bf16 ulps of that rounding; results below 2^-6 (the
    flat tails of GELU / SiLU, where fp32 1 + tanh(u) cancels) count in ulps of 2^-6: the measure of
    test_activation_of_the_exact_pre_activation.  -> (worst ulps, flat index of the worst element)."""
    want = want64.to(BF).double()
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -6))) - 7)
    err = (got.double() - want).abs() / ulp
    return float(err.max()), int(err.flatten().argmax())


# Row chunks (the 2 GiB reach of the epilogues' buffer descriptors, csrc/gemm_common.h gemm_row_chunks): an output that is the
# first N columns of rows CHUNK_LD elements (4 MiB + 128 bytes) apart puts row 512 at byte offset 2^31 + 65536, so a launch of
# 513 rows runs as pieces of 256, 256 and 1 rows (per batch entry).
CHUNK_LD = 2 ** 21 + 64


def chunk_view(B, M, N, dev, fill=SENTINEL):
    """-> (int16 buffer [B, M, CHUNK_LD] holding ``fill``, its bf16 view [(B,) M, N] of the first N columns); on the meta
    device the same geometry for the plan queries."""
    buf = torch.empty(B, M, CHUNK_LD, dtype=torch.int16, device=dev)
    if not buf.is_meta:
        buf.fill_(fill)
    out = buf.view(BF)[..., :N]
    return buf, (out if B > 1 else out[0])
