"""Torch-tensor front end of the C-ABI kernels (``include/bya.h``).

Every function enqueues hand-written HIP kernels on torch's current stream and returns ``out``.
Tensors are bf16 device tensors unless stated; 2-D ``[rows, cols]`` or 3-D ``[batch, rows, cols]`` views
with unit inner stride are accepted (no copies are made here).
"""
import ctypes
import os

import torch

from . import _hip
from ._hip import AttnDesc, AttnMixDesc, GemmDesc, check

ACT = {None: 0, "none": 0, "gelu_tanh": 1, "gelu_erf": 2, "relu": 3, "silu": 4, "leaky_relu": 5,
       "gelu_tanh_ieee": 6}        # 6: round-1 GELU form (expf + IEEE division), GEMM epilogue only, kept for A/B


_PINNED_STREAM = None


def _stream():
    """HIP stream every launch goes to: torch's current stream (looked up per call, ~8 us) unless a step pinned it."""
    if _PINNED_STREAM is not None:
        return _PINNED_STREAM
    return torch.cuda.current_stream().cuda_stream


class pinned_stream:
    """Context manager used by the engine around one step: resolve torch's current stream ONCE for the ~2000 launches
    of the step (the lookup was a third of the host-side enqueue time).  Nesting keeps the outer pin."""

    def __enter__(self):
        global _PINNED_STREAM
        self.prev = _PINNED_STREAM
        if _PINNED_STREAM is None:
            _PINNED_STREAM = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, *exc):
        global _PINNED_STREAM
        _PINNED_STREAM = self.prev
        return False


class on_stream:
    """Enqueue the launches inside the block on ``stream`` (a torch.cuda.Stream) instead of the step's pinned stream, behind
    everything already enqueued on the pinned stream; ``join()`` afterwards makes the pinned stream wait for them.  Used for
    work that nothing of the current stream's near future depends on (the step-invariant conditioning, which the first
    routing layer needs ~8 ms later): its small launches fill the CUs the big kernels leave idle."""

    def __init__(self, stream):
        self.stream, self.done = stream, None

    def __enter__(self):
        global _PINNED_STREAM
        self.main = torch.cuda.current_stream()
        self.prev_pin = _PINNED_STREAM
        fork = torch.cuda.Event()
        fork.record(self.main)
        self.stream.wait_event(fork)
        self.ctx = torch.cuda.stream(self.stream)
        self.ctx.__enter__()
        _PINNED_STREAM = self.stream.cuda_stream
        return self

    def __exit__(self, *exc):
        global _PINNED_STREAM
        self.done = torch.cuda.Event()
        self.done.record(self.stream)
        _PINNED_STREAM = self.prev_pin
        self.ctx.__exit__(*exc)
        return False

    def mark(self):
        """Inside the block: an event at this point of the side stream (``need(event)`` later makes the main stream wait for
        everything enqueued up to here, and no more)."""
        ev = torch.cuda.Event()
        ev.record(self.stream)
        return ev

    @staticmethod
    def need(ev):
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def join(self):
        if self.done is not None:
            torch.cuda.current_stream().wait_event(self.done)
            self.done = None


# ---- which kernel serves a skinny Linear is the caller's decision (include/bya.h: bya_gemm_skinny_bf16) ------------
_WEIGHT_STREAMING = False


class weight_streaming:
    """``with ops.weight_streaming():`` -- Linears of at most 64 rows inside the block go to the weight-streaming kernel
    (``bya_gemm_skinny_bf16``) when they qualify.  For code whose row counts are properties of the MODEL (the step-invariant
    conditioning), never for the token stream: a shard's rows must round like the whole's.  BYA_GEMM_SKINNY=0 switches it off."""

    def __enter__(self):
        global _WEIGHT_STREAMING
        self._old, _WEIGHT_STREAMING = _WEIGHT_STREAMING, os.environ.get("BYA_GEMM_SKINNY") != "0"      # (read per block, not per GEMM)
        return self

    def __exit__(self, *exc):
        global _WEIGHT_STREAMING
        _WEIGHT_STREAMING = self._old
        return False


# ---- library options (include/bya.h bya_set_option): the C entry points read no environment ---------------------------
set_option, get_option = _hip.set_option, _hip.get_option


class options:
    """``with ops.options(gemm_splitk=0, attn_streamk=0): ...`` -- set library options (names: ``_hip.OPTIONS``;
    ``reference_forms`` takes a mask or an iterable of ``_hip.REFERENCE_FORMS`` names) for the launches ENQUEUED inside the
    block, restore the previous values on exit."""

    def __init__(self, **kw):
        forms = kw.get("reference_forms")
        if forms is not None and not isinstance(forms, int):
            kw["reference_forms"] = sum(_hip.REFERENCE_FORMS[f] for f in ([forms] if isinstance(forms, str) else forms))
        self.kw = kw

    def __enter__(self):
        self.old = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def strict_summation():
    """No split-K tails, no stream-K attention: every output element is summed in ONE fixed order whatever the launch's
    row count -- the mode in which a rank's shard reproduces the unsharded step bit for bit."""
    return options(gemm_splitk=0, attn_streamk=0)


def board_calibration(device=None, seconds=0.3, zeros=False):
    """TFLOP/s THIS board sustains on a loop of nothing but the GEMM's MFMA (v_mfma_f32_16x16x32_bf16) with gaussian bf16
    operands in registers (include/bya.h bya_mfma_calibration): the ceiling a bench line can be read against on a pool whose
    boxes differ by a few per cent in clock under load.  Two launches of ~``seconds`` each, the second one timed (the first
    brings the board to its steady clock).  Synchronises."""
    lib = _hip.load()
    device = torch.device(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    n = (256 * 256 * 16 * 16) // 2
    g = torch.Generator(device="cpu").manual_seed(1234)
    src = torch.zeros(n, dtype=torch.bfloat16, device=device) if zeros else torch.randn(n, generator=g).to(torch.bfloat16).to(device)
    sink = torch.zeros(1, dtype=torch.float32, device=device)
    flop_per_iter = 256.0 * 4 * 2.0 * 128 * 128 * 32
    iters = max(1000, int(seconds * 2.0e15 / flop_per_iter))
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.device(device):
        for timed in (False, True):
            if timed:
                s.record()
            check(lib.bya_mfma_calibration(src.data_ptr(), src.numel() * 2, sink.data_ptr(), iters, _stream()), "bya_mfma_calibration")
        e.record()
        torch.cuda.synchronize(device)
    return iters * flop_per_iter / (s.elapsed_time(e) * 1e-3) / 1e12


# ---- optional per-entry-point timers (HIP events recorded on the launch stream; used by bench.py) -------------
_TIMERS = None
_FLOPS = {}


_SHAPE_LABELS = False


def enable_kernel_timers(by_shape=False):
    """``by_shape``: GEMM launches are keyed ``bya_gemm_bf16:BxMxNxK:epilogue`` instead of by entry point alone
    (tools/gemm_breakdown.py)."""
    global _TIMERS, _FLOPS, _SHAPE_LABELS
    _TIMERS, _FLOPS, _SHAPE_LABELS = {}, {}, bool(by_shape)
    return _TIMERS


def _begin(name, flops=0.0):
    if _TIMERS is None:
        return None
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()           # torch's CURRENT stream == the stream every kernel here is launched on
    _FLOPS[name] = _FLOPS.get(name, 0.0) + flops
    return (name, s, e)


def _end(tok):
    if tok is not None:
        tok[2].record()
        _TIMERS.setdefault(tok[0], []).append((tok[1], tok[2]))


def collect_kernel_timers():
    """-> {name: [seconds per launch]}; synchronises, then disables the timers."""
    global _TIMERS
    torch.cuda.synchronize()
    out = {k: [s.elapsed_time(e) * 1e-3 for s, e in v] for k, v in (_TIMERS or {}).items()}
    _TIMERS = None
    return out


def kernel_timer_flops():
    return dict(_FLOPS)


def _p(t):
    """Device address of a tensor for a launch (meta tensors are refused: there is nothing behind them)."""
    if t is None:
        return None
    if t.is_meta:
        raise ValueError("a meta tensor cannot be passed to a kernel launch (only the *_plan queries take them)")
    return t.data_ptr()


# The plan queries (gemm_plan & co.) launch nothing and run without a GPU: there meta tensors may stand for device tensors.
# Their "address" is this base plus the view's offset, so the 16-byte alignment of a strided view is what it would be on the
# device.  Launches never see these addresses (_p and _mat refuse meta tensors).
_META_BASE = 1 << 40


def _plan_p(t):
    """Address of a tensor for a query; ``True`` stands for "some aligned tensor" (queries alone: ``_p`` has no such thing)."""
    if t is None:
        return None
    if t is True:
        return _META_BASE
    return _META_BASE + t.storage_offset() * t.element_size() if t.is_meta else t.data_ptr()


def _mat(t, name, allow_meta=False):
    """-> (batch, rows, cols, batch_stride, row_stride) of a 2-D/3-D view with unit inner stride (``allow_meta``: the plan
    queries)."""
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name}: expected bf16, got {t.dtype}")
    if not (t.is_cuda or (allow_meta and t.is_meta)):
        raise ValueError(f"{name}: expected a device tensor (the engine has no CPU path)")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: inner stride must be 1")
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[1], 0, t.stride(0)
    if t.dim() == 3:
        return t.shape[0], t.shape[1], t.shape[2], t.stride(0), t.stride(1)
    raise ValueError(f"{name}: expected 2-D or 3-D, got {t.dim()}-D")


_GEMM_WS = {}          # device index -> workspace tensor (lives as long as the process)


def ensure_gemm_workspace(device):
    """Register the split-K workspace of the persistent GEMM kernel (bya_set_gemm_workspace) once per DEVICE: 64 MiB of
    zero-filled device memory that lives as long as the process.  Without it the kernels still run (no K split).  The
    library picks the workspace of the device that is current when a GEMM is enqueued."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ws = _GEMM_WS.get(idx)
    if ws is not None:
        return ws
    lib = _hip.load()
    n = ctypes.c_int64(0)
    check(lib.bya_gemm_workspace_bytes(ctypes.byref(n)), "bya_gemm_workspace_bytes")
    with torch.cuda.device(idx):
        ws = torch.zeros(n.value, dtype=torch.uint8, device=torch.device("cuda", idx))
        torch.cuda.synchronize(idx)
        check(lib.bya_set_gemm_workspace(ws.data_ptr(), n.value), "bya_set_gemm_workspace")
    _GEMM_WS[idx] = ws
    return ws


def gemm_workspace_status(device=None):
    """Number of split-K tiles of this device whose finisher timed out waiting for a partial sum (bya_gemm_workspace_status):
    0 on a healthy run.  Synchronises the current stream -- call it at step / run end.  ``check_gemm_workspace`` raises."""
    lib = _hip.load()
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    n = ctypes.c_int32(0)
    with torch.cuda.device(idx):
        check(lib.bya_gemm_workspace_status(ctypes.byref(n), _stream()), "bya_gemm_workspace_status")
    return n.value


_HEALED = {}           # device index -> [split-K time-outs, stream-K time-outs] already absorbed by heal_handoffs
HANDOFF_MODE = {}      # device index -> why the split forms are off on that device (absent: they are on)


def _handoff_counts(device=None):
    idx = None if device is None else torch.device(device).index
    if idx is None:                      # (None, "cuda": the current device)
        idx = torch.cuda.current_device()
    g = gemm_workspace_status(idx) if idx in _GEMM_WS else 0
    a = attn_workspace_status(idx) if idx in _ATTN_WS else 0
    seen = _HEALED.get(idx, [0, 0])
    return idx, g - seen[0], a - seen[1], g, a


def heal_handoffs(device=None):
    """Self-healing for the two kernels that hand partial sums between workgroups of ONE launch (split-K tails of
    bya_gemm_bf16, stream-K items of the joint attention).  Both count on the whole grid being resident, which holds on a
    GPU the process owns and not when something else keeps CUs busy (a second job, a profiler's helper process): the
    waiting side then gives up after a bounded spin, finishes without the missing sums and COUNTS the event.  This call
    (it synchronises: once per step) looks at the counters; if any hand-off timed out since the last call it switches both
    split forms off for the rest of the process (library options gemm_splitk = 0, attn_streamk = 0 -- one workgroup per
    tile / item, nothing to wait for), warns, records the mode in ``HANDOFF_MODE`` and returns True: THE CALLER RE-RUNS
    THE STEP, whose result is not to be trusted.  -> False on a healthy step."""
    idx, g_new, a_new, g, a = _handoff_counts(device)
    if not (g_new or a_new):
        return False
    _HEALED[idx] = [g, a]
    set_option("gemm_splitk", 0)
    set_option("attn_streamk", 0)
    HANDOFF_MODE[idx] = (f"unsplit (self-healed: {g_new} split-K and {a_new} stream-K hand-off(s) timed out -- the launch's grid was "
                         f"not co-resident, the GPU is shared; gemm_splitk = attn_streamk = 0 from here on)")
    import warnings
    warnings.warn("bind_your_avatar_implementation_amd: " + HANDOFF_MODE[idx] + "; the step is re-run")
    return True


def check_gemm_workspace(device=None):
    """Raise if a hand-off timed out that ``heal_handoffs`` has not absorbed (callers that do not re-run steps: the end of a
    clip, the end of a bench run), or if a P2P wait gave up."""
    idx, g_new, a_new, _, _ = _handoff_counts(device)
    if g_new:
        raise _hip.ByaError(f"{g_new} split-K tile(s) of bya_gemm_bf16 were finished without all their partial sums (a hand-off "
                            f"between workgroups timed out): results of this run are not to be trusted")
    if a_new:
        raise _hip.ByaError(f"{a_new} stream-K hand-off(s) of the joint attention timed out: results of this run are not to be trusted")
    # ... and no wait of a P2P exchange gave up (sharded runs; the step's output is NaN-poisoned as well, parallel / p2p.py)
    import sys
    p2p = sys.modules.get(__package__ + ".p2p")
    if p2p is not None:
        for g in list(p2p.LIVE_GROUPS):
            g.check()


_ATTN_WS = {}          # device index -> stream-K exchange workspace of the joint-attention kernel


def ensure_attn_workspace(device):
    """Register the stream-K workspace of the joint-attention kernel (bya_set_attn_workspace) once per DEVICE: 69 MB of
    zero-filled device memory that lives as long as the process.  With it, a launch whose (head, q-tile) items do not fill
    whole rounds of 256 CUs runs as 256 persistent workgroups (whole rounds, then the leftover items cut at one key tile
    between "mains" and "helpers"); without it, one workgroup per item (the last round partly idle).  Same results up to
    fp32 summation order at the cut items."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ws = _ATTN_WS.get(idx)
    if ws is not None:
        return ws
    lib = _hip.load()
    n = ctypes.c_int64(0)
    check(lib.bya_attn_workspace_bytes(ctypes.byref(n)), "bya_attn_workspace_bytes")
    with torch.cuda.device(idx):
        ws = torch.zeros(n.value, dtype=torch.uint8, device=torch.device("cuda", idx))
        torch.cuda.synchronize(idx)
        check(lib.bya_set_attn_workspace(ws.data_ptr(), n.value), "bya_set_attn_workspace")
    _ATTN_WS[idx] = ws
    return ws


def attn_workspace_status(device=None):
    """Number of stream-K hand-offs of the joint attention that timed out on this device (0 on a healthy run); synchronises."""
    lib = _hip.load()
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    n = ctypes.c_int32(0)
    with torch.cuda.device(idx):
        check(lib.bya_attn_workspace_status(ctypes.byref(n), _stream()), "bya_attn_workspace_status")
    return n.value


# ---- the front end.  Every launch below goes through _launch, every query through _plan.  Where an entry point has a query, the
# launch / ``*_plan`` pair stands over ONE body that checks the operands, derives dimensions, strides and descriptors once and
# builds the library's argument tuple with the pointer function of its mode (_p: launch, _plan_p: query), so the query answers
# what the launch does by construction.  The GEMMs first: an operand reader checks the operands of its format and hands their
# dimensions to the one descriptor filler (_fill_desc).
_UNSUPPORTED = next(rc for rc, name in _hip.ERRORS.items() if name == "BYA_ERR_UNSUPPORTED")


def _fill_desc(dims, res, split, epi, plan):
    """The bya_gemm_desc of one launch.  ``dims`` = (batch, M, N, K, lda, a_batch_stride, ldw, ldc, c_batch_stride) as the
    operand reader derived them; ``epi`` = (gate_split, gate_batch_stride, act, bias_rowscale, alpha)."""
    ab, M, N, K, lda, a_bs, ldw, ldc, c_bs = dims
    gate_split, gate_batch_stride, act, bias_rowscale, alpha = epi
    d = GemmDesc()
    d.M, d.N, d.K, d.batch = M, N, K, ab
    d.lda, d.ldw, d.ldc = lda, ldw, ldc
    d.a_batch_stride, d.c_batch_stride = a_bs, c_bs
    if res is not None:
        rb, Mr, Nr, r_bs, ldres = _mat(res, "res", plan)
        if (Mr, Nr) != (M, N) or rb not in (1, ab):
            raise ValueError("res shape mismatch")
        d.ldres, d.res_batch_stride = ldres, (r_bs if rb == ab else 0)
    d.gate_batch_stride, d.gate_split, d.act = gate_batch_stride, gate_split, ACT[act]
    d.n_split, d.c_split_stride = (0, 0) if split is None else split
    d.bias_rowscale, d.alpha = (_plan_p if plan else _p)(bias_rowscale), float(alpha)
    if bias_rowscale is not None:
        assert bias_rowscale.dtype == torch.float32 and bias_rowscale.is_contiguous() and bias_rowscale.numel() == ab * M
    return d


_NO_EPILOGUE = (0, 0, None, None, 1.0)          # ``epi`` of a launch without gates, activation, row scale or alpha
_NO_NORM = (None,) * 9                          # the q/k-norm arguments of _qkn_desc, absent (with ``tensors`` 0)


def _qkn_desc(d, tensors, qw, qb, kw, kb, cos, sin, text_rows, eps, k_scale, plan):
    """The bya_qk_norm_desc of a q|k|v projection with descriptor ``d`` (``tensors`` 0: an empty one)."""
    n = _hip.QkNormDesc()
    if not tensors:
        return n
    ptr = _plan_p if plan else _p
    n.qw, n.qb, n.kw, n.kb, n.cos, n.sin = ptr(qw), ptr(qb), ptr(kw), ptr(kb), ptr(cos), ptr(sin)
    n.text_rows, n.width, n.eps, n.k_scale = int(text_rows), d.N // tensors, float(eps), float(k_scale)
    if cos is not None:
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
        assert cos.shape == (d.M - text_rows, 64)
    return n


def _with_stats(call, d, n, stats, plan):
    """``call`` = (fused q|k|v entry point, its arguments) as it is (``stats`` None), or as the call of ``<entry point>_stats``
    with the table behind the arguments: the score-bound table of ``qknorm_rope`` for the launch to fill -- fp32
    [slots, 2, batch * width / 64], zeroed by the caller -- or, in a query, its slot count."""
    if stats is None:
        return call
    if plan and isinstance(stats, int):
        ps, slots = _META_BASE, stats
    else:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.dim() == 3
        assert stats.shape[1:] == (2, d.batch * (n.width // 64))
        ps, slots = (_plan_p if plan else _p)(stats), stats.shape[0]
    entry, args = call
    return entry + "_stats", (*args, ps, slots)


def _label(d, pre="", act=False, gate0=None, res=None):
    """The shape label of a GEMM's timer bucket (``enable_kernel_timers(by_shape=True)``): [pre]:BxMxNxK[:epilogue]."""
    s = f"{pre}:{d.batch}x{d.M}x{d.N}x{d.K}"
    if act is not False:
        s += f":{act or 'none'}{'+gate' if gate0 is not None else ''}{'+res' if res is not None else ''}"
    return s


def _launch(bucket, label, work, call, may_decline=False):
    """Enqueue ``call`` = (entry point, its arguments up to the stream) under timer ``bucket`` (None: the entry point's name; a
    ``bucket`` that starts with ":" is appended to it -- the attention's tag; + ``label`` when shape labels are on) and count its
    FLOPs there: ``work``, or 2 * batch * M * N * K of the bya_gemm_desc ``work`` (read only with the timers on).  -> True; or
    False where ``may_decline`` and the library answers BYA_ERR_UNSUPPORTED: nothing was launched, so no timer entry stays and
    nothing is counted (the caller's other launches count the FLOPs).  A launch that raises counts nothing either."""
    entry, args = call
    if bucket is None or bucket[0] == ":":
        bucket = entry + (bucket or "")
    if label:
        bucket += label
    tok = _begin(bucket)
    rc = getattr(_hip.load(), entry)(*args, _stream())
    if may_decline and rc == _UNSUPPORTED:
        return False
    check(rc, entry)
    if tok is not None:
        _FLOPS[bucket] += work if isinstance(work, float) else 2.0 * work.batch * work.M * work.N * work.K
        _end(tok)
    return True


def _plan(call, may_decline=False, struct=_hip.GemmPlan, to_dict=None):
    """Ask ``<entry point>_plan`` with the arguments of ``call`` (``_launch``), which fills a ``struct``: its ``to_dict`` (by
    default ``gemm_plan``'s dict); None where ``may_decline`` and the library answers BYA_ERR_UNSUPPORTED."""
    entry, args = call
    p = struct()
    rc = getattr(_hip.load(), entry + "_plan")(*args, ctypes.byref(p))
    if may_decline and rc == _UNSUPPORTED:
        return None
    check(rc, entry + "_plan")
    return (to_dict or _plan_dict)(p)


def _gemm_desc(a, w, out, res, split, epi, plan=False):
    ab, M, K, a_bs, lda = _mat(a, "a", plan)
    ob, Mo, N, c_bs, ldc = _mat(out, "out", plan)
    if split is not None:
        N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or w.shape[0] != N or w.stride(1) != 1 or w.dtype != torch.bfloat16:
        raise ValueError(f"w: expected bf16 [{N}, {K}], got {tuple(w.shape)} {w.dtype}")
    if (ab, M) != (ob, Mo):
        raise ValueError("a/out row mismatch")
    return _fill_desc((ab, M, N, K, lda, a_bs, w.stride(0), ldc, c_bs), res, split, epi, plan)


def _takes_skinny(d, gate0, bias_rowscale, split):
    """ops.gemm sends the launch to the weight-streaming kernel (``weight_streaming``)."""
    return (_WEIGHT_STREAMING and d.M <= 64 and d.N <= 8192 and d.N % 16 == 0 and d.K % 32 == 0 and d.K >= 256 and gate0 is None
            and bias_rowscale is None and split is None and d.a_batch_stride % 8 == 0)


def _bf16_bucket(d):
    # per-kernel timers: Linears over fewer than 1024 rows (the step-invariant conditioning: 32 face tokens, 52 audio windows,
    # 577 ViT tokens against 2048..49152-wide weights) stream their WEIGHTS and are bound by HBM, not by the matrix cores --
    # they get their own bucket so that the MFMA roofline of bench.py is taken over the launches it applies to
    return "bya_gemm_bf16" if d.M >= 1024 else "bya_gemm_bf16_small_m"


def _gemm_call(a, w, bias, out, res, gate0, gate1, split, epi, plan):
    d = _gemm_desc(a, w, out, res, split, epi, plan)                     # (validates first)
    if a.is_cuda and a.device.index not in _GEMM_WS:                     # (a launch's ``a`` is a device tensor: _mat)
        ensure_gemm_workspace(a.device)
    q = _plan_p if plan else _p
    if _takes_skinny(d, gate0, epi[3], split):                           # (epi[3]: bias_rowscale)
        return d, ("bya_gemm_skinny_bf16", (q(a), q(w), q(bias), q(out), q(res), ctypes.byref(d)))
    return d, ("bya_gemm_bf16", (q(a), q(w), q(bias), q(out), q(res), q(gate0), q(gate1), ctypes.byref(d)))


def gemm(a, w, out, bias=None, res=None, gate0=None, gate1=None, gate_split=0, gate_batch_stride=0, act=None,
         split=None, bias_rowscale=None, alpha=1.0):
    """out = res + gate * act(a @ w.T + bias).  a: [(B,) M, K], w: [N, K], out/res: [(B,) M, N].

    ``split=(n_split, stride)``: ``out`` is the FIRST of N/n_split equally shaped tensors ``stride`` elements apart;
    column n of the product lands in tensor n // n_split (packed q|k|v projection -> three buffers, one launch)."""
    d, call = _gemm_call(a, w, bias, out, res, gate0, gate1, split, (gate_split, gate_batch_stride, act, bias_rowscale, alpha), False)
    _launch(_bf16_bucket(d), _SHAPE_LABELS and _label(d, "", act, gate0, res), d, call)
    return out


# ---- plan queries (include/bya.h bya_gemm_plan): which kernels a GEMM launch with these arguments runs, under the current
# options and the current device's split-K workspace.  They launch nothing; meta tensors stand for device tensors.  Given
# device tensors they register the device's workspace as the launch would (else a query made before the device's first GEMM
# would miss a split-K the launch then takes).
GEMM_PATHS = _hip.GEMM_PATHS


def _plan_dict(p):
    return {"path": GEMM_PATHS[p.path], "m0": p.m0, "tail": GEMM_PATHS.get(p.tail) if p.m0 > 0 else None,
            "split_k": p.split_k, "row_chunks": p.row_chunks}


def plan_key(plan):
    """One name per distinct kernel sequence: "p256", "p256|t128x128" (row split, tail kernel), "p256+splitk"."""
    return plan["path"] + (f"|{plan['tail']}" if plan["tail"] else "") + ("+splitk" if plan["split_k"] else "")


def gemm_plan(a, w, out, bias=None, res=None, gate0=None, gate1=None, gate_split=0, gate_batch_stride=0, act=None,
              split=None, bias_rowscale=None, alpha=1.0):
    """What ``gemm`` with the same arguments would run: {"path", "m0", "tail", "split_k", "row_chunks"} (kernel names of
    ``GEMM_PATHS``, or path "skinny" for the weight-streaming kernel).  Raises what ``gemm`` would raise."""
    _, call = _gemm_call(a, w, bias, out, res, gate0, gate1, split, (gate_split, gate_batch_stride, act, bias_rowscale, alpha), True)
    if call[0] == "bya_gemm_skinny_bf16":                                # (one kernel: the library has no query for it)
        return {"path": "skinny", "m0": 0, "tail": None, "split_k": 0, "row_chunks": 1}
    return _plan(call)


def _qkn_call(a, w, out, bias, split, norm, tensors, plan, stats=None):
    if tensors not in (2, 3) or w.shape[0] % tensors:
        raise ValueError("gemm_qkv_norm_rope: a [(B,) M, K], w [3 * width, K] (or [2 * width, K]: q | k alone, tensors=2), "
                         "out = the first of the split outputs")
    d = _gemm_desc(a, w, out, None, tuple(split), _NO_EPILOGUE, plan)    # (``split`` is required: None is a TypeError)
    n = _qkn_desc(d, tensors, *norm, plan)
    q = _plan_p if plan else _p
    return d, _with_stats(("bya_gemm_qkv_norm_rope", (q(a), q(w), q(bias), q(out), ctypes.byref(d), ctypes.byref(n))), d, n, stats, plan)


def gemm_qkv_norm_rope(a, w, out, bias, split, qw, qb, kw, kb, cos, sin, text_rows, eps=1e-6, k_scale=1.0, tensors=3, stats=None):
    """The packed q|k|v projection with the q/k LayerNorm(64) + RoPE in its epilogue (bya_gemm_qkv_norm_rope): equals
    ``gemm(..., split=split)`` followed by ``qknorm_rope`` bit for bit, in one launch.  Returns False (nothing launched) when
    the library does not take the shape -- the caller then issues the two launches.  ``stats``: ``qknorm_rope``'s table (fp32
    [slots, 2, B * width / 64], ZEROED by the caller) for this launch to fill as that one would: the same maxima over the slots,
    bit for bit (which slot holds one differs)."""
    d, call = _qkn_call(a, w, out, bias, split, (qw, qb, kw, kb, cos, sin, text_rows, eps, k_scale), tensors, False, stats)
    return _launch(_bf16_bucket(d), None, d, call, True)         # (the bf16 GEMM's bucket, and no shape label)


def gemm_qkv_norm_rope_plan(a, w, out, bias, split, qw, qb, kw, kb, cos, sin, text_rows, eps=1e-6, k_scale=1.0, tensors=3,
                            stats=None):
    """What ``gemm_qkv_norm_rope`` would run (``gemm_plan``'s dict): path "p256" (its row plan 0), "p128" (plan 1), or
    "p256" with m0 and tail "p128" (plan 2); None where it declines the shape (the caller's two launches).  ``stats``: None,
    the number of slots, or the table (as for ``qknorm_rope_plan``)."""
    return _plan(_qkn_call(a, w, out, bias, split, (qw, qb, kw, kb, cos, sin, text_rows, eps, k_scale), tensors, True, stats)[1], True)


def quantize_rows_fp8(x, q=None, scale=None):
    """Per-row symmetric e4m3 quantisation of a bf16 matrix [(B,) M, K] -> (uint8 [.., M, K], fp32 scale [.., M])."""
    b, M, K, bs, ldx = _mat(x, "x")
    if b > 1 and bs != M * ldx:
        raise ValueError("quantize_rows_fp8: batch entries must be evenly stacked rows")
    if q is None:
        q = torch.empty(*x.shape, dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty(*x.shape[:-1], dtype=torch.float32, device=x.device)
    assert q.dtype == torch.uint8 and q.is_contiguous() and scale.dtype == torch.float32 and scale.is_contiguous()
    assert q.numel() == b * M * K and scale.numel() == b * M
    _launch(None, None, 0.0, ("bya_quantize_rows_fp8", (_p(x), _p(q), _p(scale), b * M, K, ldx, K)))
    return q, scale


def _fp8_desc(a8, a_scale, w8, w_scale, out, res, split, epi, plan=False):
    if a8.dim() == 2:
        ab, (M, K) = 1, a8.shape
    else:
        ab, M, K = a8.shape
    ob, Mo, N, c_bs, ldc = _mat(out, "out", plan)
    if split is not None:
        N = w8.shape[0]
    assert a8.dtype == torch.uint8 and w8.dtype == torch.uint8 and a8.is_contiguous() and w8.is_contiguous()
    assert w8.shape == (N, K) and (ab, M) == (ob, Mo)
    assert a_scale.dtype == torch.float32 and a_scale.numel() == ab * M and a_scale.is_contiguous()
    assert w_scale.dtype == torch.float32 and w_scale.numel() == N and w_scale.is_contiguous()
    return _fill_desc((ab, M, N, K, K, M * K, K, ldc, c_bs), res, split, epi, plan)


def _fp8_call(a8, a_scale, w8, w_scale, bias, out, res, gate0, gate1, split, epi, plan):
    d = _fp8_desc(a8, a_scale, w8, w_scale, out, res, split, epi, plan)
    q = _plan_p if plan else _p
    return d, ("bya_gemm_fp8", (q(a8), q(a_scale), q(w8), q(w_scale), q(bias), q(out), q(res), q(gate0), q(gate1), ctypes.byref(d)))


def gemm_fp8(a8, a_scale, w8, w_scale, out, bias=None, res=None, gate0=None, gate1=None, gate_split=0,
             gate_batch_stride=0, act=None, split=None, alpha=1.0):
    """out = res + gate * act(a_scale * w_scale * (a8 @ w8.T) + bias) with e4m3 operands (``quantize_rows_fp8``)."""
    d, call = _fp8_call(a8, a_scale, w8, w_scale, bias, out, res, gate0, gate1, split, (gate_split, gate_batch_stride, act, None, alpha),
                        False)
    _launch("bya_gemm_fp8", _SHAPE_LABELS and _label(d, "", act, gate0, res), d, call)
    return out


def gemm_fp8_plan(a8, a_scale, w8, w_scale, out, bias=None, res=None, gate0=None, gate1=None, gate_split=0,
                  gate_batch_stride=0, act=None, split=None, alpha=1.0):
    """What ``gemm_fp8`` would run (``gemm_plan``'s dict): path "t128x128" or "p256"."""
    return _plan(_fp8_call(a8, a_scale, w8, w_scale, bias, out, res, gate0, gate1, split, (gate_split, gate_batch_stride, act, None, alpha),
                           True)[1])


def _fp8_qkn_call(a8, a_scale, w8, w_scale, out, bias, split, norm, tensors, act, res, alpha, plan, stats=None):
    if tensors not in (2, 3) or w8.shape[0] % tensors or split is None:
        raise ValueError("gemm_fp8_qkv_norm_rope: w8 [3 * width, K] (or [2 * width, K]: q | k alone, tensors=2), "
                         "out = the first of the split outputs, split = (n_split, c_split_stride)")
    # (the entry point has no residual argument: the descriptor says that one was asked for, and it declines)
    d = _fp8_desc(a8, a_scale, w8, w_scale, out, res, split, (0, 0, act, None, alpha), plan)
    n = _qkn_desc(d, tensors, *norm, plan)
    q = _plan_p if plan else _p
    call = ("bya_gemm_fp8_qkv_norm_rope", (q(a8), q(a_scale), q(w8), q(w_scale), q(bias), q(out), ctypes.byref(d), ctypes.byref(n)))
    return d, _with_stats(call, d, n, stats, plan)


def gemm_fp8_qkv_norm_rope(a8, a_scale, w8, w_scale, out, bias, split, qw, qb, kw, kb, cos, sin, text_rows, eps=1e-6,
                           k_scale=1.0, tensors=3, *, act=None, res=None, stats=None):
    """The packed q|k|v projection on e4m3 operands with the q/k LayerNorm(64) + RoPE in its epilogue
    (bya_gemm_fp8_qkv_norm_rope): equals ``gemm_fp8(..., split=split)`` followed by ``qknorm_rope`` bit for bit, in one launch
    on the kernel ``gemm_fp8`` would take (``gemm_fp8_plan``'s path, option ``fp8_kernel`` included).  Returns False (nothing
    launched, nothing counted) when the library does not take the shape -- the caller then issues the two launches.
    ``act`` / ``res`` (keyword only): what the engine never asks of this launch, here so that a caller that does is told False.
    ``stats``: as for ``gemm_qkv_norm_rope``; False where the kernel the launch would take does not record them."""
    d, call = _fp8_qkn_call(a8, a_scale, w8, w_scale, out, bias, split, (qw, qb, kw, kb, cos, sin, text_rows, eps, k_scale), tensors,
                               act, res, 1.0, False, stats)
    return _launch("bya_gemm_fp8_qkv_norm_rope", _SHAPE_LABELS and _label(d), d, call, True)


def gemm_fp8_qkv_norm_rope_plan(a8, a_scale, w8, w_scale, out, bias, split, qw, qb, kw, kb, cos, sin, text_rows, eps=1e-6,
                                k_scale=1.0, tensors=3, *, act=None, res=None, alpha=1.0, stats=None):
    """What ``gemm_fp8_qkv_norm_rope`` would run (``gemm_plan``'s dict): path "t128x128" or "p256", one row chunk; None where
    it declines the shape (the caller's two launches).  ``act`` / ``res`` / ``alpha``: descriptor fields the launch wrapper's
    callers never set, here to ask what the library answers to them."""
    return _plan(_fp8_qkn_call(a8, a_scale, w8, w_scale, out, bias, split, (qw, qb, kw, kb, cos, sin, text_rows, eps, k_scale), tensors,
                               act, res, alpha, True, stats)[1], True)


# OCP MX element formats (include/bya.h, "MX weights"): name -> the matrix instruction's format code, element bits.
# MX_FORMATS: what activations (and weights) may be; MX_WEIGHT_FORMATS: what weights may be -- e2m1 is theirs alone
MX_FORMATS = {"mxfp8": 0, "mxfp6": 2}
MX_WEIGHT_FORMATS = {**MX_FORMATS, "mxfp4": 4}
MX_BITS = {"mxfp8": 8, "mxfp6": 6, "mxfp4": 4}


def mx_fmt_code(fmt):
    if fmt not in MX_FORMATS:
        raise ValueError(f"MX format {fmt!r}: expected one of {sorted(MX_FORMATS)}")
    return MX_FORMATS[fmt]


def mx_weight_fmt_code(fmt):
    if fmt not in MX_WEIGHT_FORMATS:
        raise ValueError(f"MX weight format {fmt!r}: expected one of {sorted(MX_WEIGHT_FORMATS)}")
    return MX_WEIGHT_FORMATS[fmt]


def mx_fmt_pair(fmt, w_fmt):
    """(activation code, weight code) of a GEMM; weights in the activations' format or in "mxfp4"."""
    a = mx_fmt_code(fmt)
    w = a if w_fmt is None else mx_weight_fmt_code(w_fmt)
    if w not in (a, MX_WEIGHT_FORMATS["mxfp4"]):
        raise ValueError(f"MX weight format {w_fmt!r} under {fmt!r} activations: expected {fmt!r} or 'mxfp4'")
    return a, w


def mx_code_bytes(K, fmt):
    """Bytes of one row of K MX codes (no padding)."""
    mx_weight_fmt_code(fmt)
    return K * MX_BITS[fmt] // 8


def quantize_mx(x, fmt="mxfp6", codes=None, scales=None):
    """OCP MX block quantisation of a bf16 matrix [(B,) M, K] -> (uint8 codes [.., M, K * bits / 8], uint8 e8m0 scales
    [.., M, K / 32]).  ``fmt`` "mxfp4" (e2m1) is a weight format: no GEMM takes it as its activations."""
    code = mx_weight_fmt_code(fmt)
    b, M, K, bs, ldx = _mat(x, "x")
    if b > 1 and bs != M * ldx:
        raise ValueError("quantize_mx: batch entries must be evenly stacked rows")
    lead = tuple(x.shape[:-1])
    if codes is None:
        codes = torch.empty(*lead, mx_code_bytes(K, fmt), dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty(*lead, K // 32, dtype=torch.uint8, device=x.device)
    assert codes.dtype == torch.uint8 and codes.is_contiguous() and codes.numel() == b * M * mx_code_bytes(K, fmt)
    assert scales.dtype == torch.uint8 and scales.is_contiguous() and scales.numel() == b * M * (K // 32)
    _launch(None, None, 0.0, ("bya_quantize_mx", (_p(x), _p(codes), _p(scales), b * M, K, ldx, code)))
    return codes, scales


def _mx_desc(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, res, split, epi, plan=False):
    if a_scales.dim() == 2:
        ab, (M, KS) = 1, a_scales.shape
    else:
        ab, M, KS = a_scales.shape
    K = KS * 32
    ob, Mo, N, c_bs, ldc = _mat(out, "out", plan)
    if split is not None:
        N = w_codes.shape[0]
    rb_, rbw = mx_code_bytes(K, fmt), mx_code_bytes(K, w_fmt or fmt)
    assert a_codes.dtype == w_codes.dtype == a_scales.dtype == w_scales.dtype == torch.uint8
    assert a_codes.is_contiguous() and w_codes.is_contiguous() and a_scales.is_contiguous() and w_scales.is_contiguous()
    assert a_codes.numel() == ab * M * rb_ and w_codes.shape == (N, rbw) and w_scales.shape == (N, KS)
    assert (ab, M) == (ob, Mo)
    return _fill_desc((ab, M, N, K, rb_, M * rb_, rbw, ldc, c_bs), res, split, epi, plan)


def _mx_gemm_call(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, bias, res, gate0, gate1, split, epi, plan):
    code, wcode = mx_fmt_pair(fmt, w_fmt)
    d = _mx_desc(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, res, split, epi, plan)
    q = _plan_p if plan else _p
    args = (q(a_codes), q(a_scales), q(w_codes), q(w_scales), q(bias), q(out), q(res), q(gate0), q(gate1), ctypes.byref(d), code)
    return d, (("bya_gemm_mx_mixed", (*args, wcode)) if wcode != code else ("bya_gemm_mx", args))


def gemm_mx(a_codes, a_scales, w_codes, w_scales, out, fmt="mxfp6", bias=None, res=None, gate0=None, gate1=None,
            gate_split=0, gate_batch_stride=0, act=None, split=None, alpha=1.0, w_fmt=None, bias_rowscale=None):
    """out = res + gate * alpha * act(A @ W.T + rowscale * bias) with both operands in MX form (``quantize_mx``); K is read off
    the scales.  ``fmt``: the activations' format; ``w_fmt``: the weights' (None = the same, or "mxfp4": bya_gemm_mx_mixed).
    ``bias_rowscale``: fp32 [batch * M] as for ``gemm`` (every MX kernel's bf16 epilogue honours it)."""
    d, call = _mx_gemm_call(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, bias, res, gate0, gate1, split,
                            (gate_split, gate_batch_stride, act, bias_rowscale, alpha), False)
    mixed = call[0] == "bya_gemm_mx_mixed"
    _launch(call[0], _SHAPE_LABELS and _label(d, f":{fmt + '*' + w_fmt if mixed else fmt}", act, gate0, res), d, call)
    return out


def gemm_mx_plan(a_codes, a_scales, w_codes, w_scales, out, fmt="mxfp6", bias=None, res=None, gate0=None, gate1=None,
                 gate_split=0, gate_batch_stride=0, act=None, split=None, alpha=1.0, w_fmt=None, bias_rowscale=None):
    """What ``gemm_mx`` would run (``gemm_plan``'s dict): path "t128x128" or "t256x256" (mxfp6 activations only), or "p256"
    (mxfp8 activations and weights under option ``mx_kernel``)."""
    return _plan(_mx_gemm_call(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, bias, res, gate0, gate1, split,
                               (gate_split, gate_batch_stride, act, bias_rowscale, alpha), True)[1])


def _mx_qkn_descs(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, split, norm, tensors, act, alpha, plan):
    if tensors not in (2, 3) or w_codes.shape[0] % tensors or split is None:
        raise ValueError("gemm_mx_qkv_norm_rope: w_codes [3 * width, ..] (or [2 * width, ..]: q | k alone, tensors=2), "
                         "out = the first of the split outputs, split = (n_split, c_split_stride)")
    d = _mx_desc(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, None, split, (0, 0, act, None, alpha), plan)
    return d, _qkn_desc(d, tensors, *norm, plan)


def _mx_qkn_call(a_codes, a_scales, w_codes, w_scales, out, bias, split, norm, tensors, fmt, w_fmt, act, alpha, kernel, plan, stats=None):
    code, wcode = mx_fmt_pair(fmt, w_fmt)
    d, n = _mx_qkn_descs(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, split, norm, tensors, act, alpha, plan)
    q = _plan_p if plan else _p
    args = (q(a_codes), q(a_scales), q(w_codes), q(w_scales), q(bias), q(out), code, wcode, ctypes.byref(d), ctypes.byref(n))
    if stats is not None:                # (bya_gemm_mx_qkv_norm_rope_stats: the kernel is always an argument)
        return d, _with_stats(("bya_gemm_mx_qkv_norm_rope", (*args, int(kernel))), d, n, stats, plan)
    return d, (("bya_gemm_mx_qkv_norm_rope", args) if kernel == 0 else ("bya_gemm_mx_qkv_norm_rope_on", (*args, int(kernel))))


def gemm_mx_qkv_norm_rope(a_codes, a_scales, w_codes, w_scales, out, bias, split, qw, qb, kw, kb, cos, sin, text_rows,
                          eps=1e-6, k_scale=1.0, tensors=3, fmt="mxfp6", w_fmt=None, kernel=0, stats=None):
    """The packed q|k|v projection on MX operands with the q/k LayerNorm(64) + RoPE in its epilogue
    (bya_gemm_mx_qkv_norm_rope): equals ``gemm_mx(..., split=split)`` followed by ``qknorm_rope`` bit for bit, in one launch.
    Returns False (nothing launched, nothing counted) when the library does not take the shape -- the caller then issues the
    two launches.  ``kernel``: 0 = the tiled kernel; 1 = the persistent 256 x 256 kernel where the launch fills it (mxfp8
    activations and weights only, the same bits; bya_gemm_mx_qkv_norm_rope_on), 2 = without the tile count (tests).  Option
    ``mx_kernel`` has no say here.  ``stats``: as for ``gemm_qkv_norm_rope``; False where the kernel the launch would take does
    not record them (the tiled kernels)."""
    d, call = _mx_qkn_call(a_codes, a_scales, w_codes, w_scales, out, bias, split, (qw, qb, kw, kb, cos, sin, text_rows, eps, k_scale),
                              tensors, fmt, w_fmt, None, 1.0, kernel, False, stats)
    return _launch("bya_gemm_mx_qkv_norm_rope", _SHAPE_LABELS and _label(d, f":{fmt}*{w_fmt or fmt}"), d, call, True)


def gemm_mx_qkv_norm_rope_plan(a_codes, a_scales, w_codes, w_scales, out, bias, split, qw, qb, kw, kb, cos, sin, text_rows,
                               eps=1e-6, k_scale=1.0, tensors=3, fmt="mxfp6", w_fmt=None, act=None, alpha=1.0, kernel=0, stats=None):
    """What ``gemm_mx_qkv_norm_rope`` would run (``gemm_plan``'s dict): path "t128x128" or "t256x256" (mxfp6 activations
    only), or "p256" (``kernel`` 1 or 2, mxfp8 activations and weights); None where it declines the shape (the caller's two
    launches).  ``act`` / ``alpha``: descriptor fields the launch wrapper never sets, here to ask what the library answers
    to them."""
    return _plan(_mx_qkn_call(a_codes, a_scales, w_codes, w_scales, out, bias, split, (qw, qb, kw, kb, cos, sin, text_rows, eps, k_scale),
                              tensors, fmt, w_fmt, act, alpha, kernel, True, stats)[1], True)


def _mx_quant_desc(a_codes, a_scales, w_codes, w_scales, out_codes, out_scales, fmt, w_fmt, out_fmt, act, alpha):
    if a_scales.dim() == 2:
        ab, (M, KS) = 1, a_scales.shape
    else:
        ab, M, KS = a_scales.shape
    K, N = KS * 32, w_codes.shape[0]
    rb_, rbw, rbo = mx_code_bytes(K, fmt), mx_code_bytes(K, w_fmt or fmt), mx_code_bytes(N, out_fmt)
    for t in (a_codes, a_scales, w_codes, w_scales, out_codes, out_scales):
        assert t.dtype == torch.uint8 and t.is_contiguous()
    assert a_codes.numel() == ab * M * rb_ and w_codes.shape == (N, rbw) and w_scales.shape == (N, KS)
    if N % 32 or out_codes.numel() != ab * M * rbo or out_scales.numel() != ab * M * (N // 32):
        raise ValueError("gemm_mx_quant: out_codes / out_scales must hold [batch * M, N * bits / 8] and [batch * M, N / 32]")
    return _fill_desc((ab, M, N, K, rb_, M * rb_, rbw, rbo, M * rbo), None, None, (0, 0, act, None, alpha), False)


def _mx_quant_call(a_codes, a_scales, w_codes, w_scales, out_codes, out_scales, fmt, w_fmt, out_fmt, bias, act, alpha, plan):
    code, wcode = mx_fmt_pair(fmt, w_fmt)
    out_fmt = fmt if out_fmt is None else out_fmt
    ocode = mx_fmt_code(out_fmt)
    d = _mx_quant_desc(a_codes, a_scales, w_codes, w_scales, out_codes, out_scales, fmt, w_fmt, out_fmt, act, alpha)
    q = _plan_p if plan else _p
    return d, out_fmt, ("bya_gemm_mx_quant", (q(a_codes), q(a_scales), q(w_codes), q(w_scales), q(bias), q(out_codes), q(out_scales),
                                              ctypes.byref(d), code, wcode, ocode))


def gemm_mx_quant(a_codes, a_scales, w_codes, w_scales, out_codes, out_scales, fmt="mxfp6", w_fmt=None, out_fmt=None,
                  bias=None, act=None, alpha=1.0):
    """``quantize_mx(gemm_mx(...), out_fmt)`` in one launch (bya_gemm_mx_quant): the GEMM's epilogue writes the MX codes and
    block scales of its bf16-rounded result, byte for byte what the two launches write, into the preallocated pair
    ``out_codes`` [(B,) M, N * bits / 8], ``out_scales`` [(B,) M, N / 32].  ``out_fmt``: "mxfp8" or "mxfp6" (None = ``fmt``).
    Returns ``(out_codes, out_scales)``: the ``quantised=`` pair of the next MX Linear."""
    d, out_fmt, call = _mx_quant_call(a_codes, a_scales, w_codes, w_scales, out_codes, out_scales, fmt, w_fmt, out_fmt, bias, act, alpha,
                                      False)
    _launch("bya_gemm_mx_quant", _SHAPE_LABELS and _label(d, f":{fmt}*{w_fmt or fmt}>{out_fmt}", act), d, call)
    return out_codes, out_scales


def gemm_mx_quant_plan(a_codes, a_scales, w_codes, w_scales, out_codes, out_scales, fmt="mxfp6", w_fmt=None, out_fmt=None,
                       bias=None, act=None, alpha=1.0):
    """What ``gemm_mx_quant`` would run (``gemm_plan``'s dict): path "t128x128" or "t256x256" (mxfp6 activations only), or
    "p256" (mxfp8 activations, weights and output under option ``mx_kernel``)."""
    return _plan(_mx_quant_call(a_codes, a_scales, w_codes, w_scales, out_codes, out_scales, fmt, w_fmt, out_fmt, bias, act, alpha,
                                True)[2])


def _mx_call(a_codes, a_scales, w_codes, w_scales, out, kernel, fmt, w_fmt, bias, res, gate0, gate1, split, epi, out_scales,
             out_fmt, norm, plan):
    """(bya_mx_gemm_call, bya_gemm_desc, the norm descriptor the call points to, the epilogue's name) of ``gemm_mx_call``."""
    code, wcode = mx_fmt_pair(fmt, w_fmt)
    ptr = _plan_p if plan else _p
    c, n = _hip.MxGemmCall(), None
    _, _, act, bias_rowscale, alpha = epi
    if bias_rowscale is not None and (norm is not None or out_scales is not None):
        raise ValueError("gemm_mx_call: bias_rowscale goes with the bf16 epilogue alone")
    if norm is not None and out_scales is not None:
        # (the library refuses the pair; build the bf16 descriptor and an empty norm so that it is asked)
        d = _mx_desc(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, res, split, epi, plan)
        c.q_scales, n, name = ptr(out_scales), _qkn_desc(d, 0, *_NO_NORM, plan), "both"
    elif norm is not None:
        d, n = _mx_qkn_descs(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, split,
                             (norm["qw"], norm["qb"], norm["kw"], norm["kb"], norm.get("cos"), norm.get("sin"), norm["text_rows"],
                              norm.get("eps", 1e-6), norm.get("k_scale", 1.0)), norm.get("tensors", 3), act, alpha, plan)
        name = "qkn"
    elif out_scales is not None:
        out_fmt = fmt if out_fmt is None else out_fmt
        d = _mx_quant_desc(a_codes, a_scales, w_codes, w_scales, out, out_scales, fmt, w_fmt, out_fmt, act, alpha)
        c.q_scales, c.out_fmt, name = ptr(out_scales), mx_fmt_code(out_fmt), "quant"
    else:
        d, name = _mx_desc(a_codes, a_scales, w_codes, w_scales, out, fmt, w_fmt, res, split, epi, plan), "bf16"
    if n is not None:
        c.norm = ctypes.pointer(n)
    c.A, c.a_scales, c.W, c.w_scales, c.bias, c.C = ptr(a_codes), ptr(a_scales), ptr(w_codes), ptr(w_scales), ptr(bias), ptr(out)
    c.res, c.gate0, c.gate1 = ptr(res), ptr(gate0), ptr(gate1)
    c.a_fmt, c.w_fmt, c.kernel = code, wcode, int(kernel)
    return c, d, n, name


def _mx_call_with_stats(fn, a_codes, a_scales, w_codes, w_scales, out, kernel, fmt, w_fmt, bias, split, norm, others, alpha):
    """``gemm_mx_call`` / ``gemm_mx_call_plan`` with a table in the ``norm`` dict: ``fn`` = ``gemm_mx_qkv_norm_rope`` / its
    ``_plan`` twin with the call's ``kernel``; nothing but the q/k-norm epilogue's own arguments goes with a table."""
    if any(o is not None for o in others) or alpha != 1.0 or split is None:
        raise ValueError("gemm_mx_call: a statistics table goes with the q/k-norm epilogue's arguments alone (bias, split)")
    return fn(a_codes, a_scales, w_codes, w_scales, out, bias, split, norm["qw"], norm["qb"], norm["kw"], norm["kb"], norm.get("cos"),
              norm.get("sin"), norm["text_rows"], eps=norm.get("eps", 1e-6), k_scale=norm.get("k_scale", 1.0),
              tensors=norm.get("tensors", 3), fmt=fmt, w_fmt=w_fmt, kernel=kernel, stats=norm["stats"])


def gemm_mx_call(a_codes, a_scales, w_codes, w_scales, out, kernel=0, fmt="mxfp8", w_fmt=None, bias=None, res=None, gate0=None,
                 gate1=None, gate_split=0, gate_batch_stride=0, act=None, split=None, alpha=1.0, out_scales=None, out_fmt=None,
                 norm=None, bias_rowscale=None):
    """Any MX GEMM as one call whose kernel is an ARGUMENT (bya_gemm_mx_call; option ``mx_kernel`` has no say): ``kernel`` 0 =
    the tiled kernels, exactly ``gemm_mx`` / ``gemm_mx_quant`` / ``gemm_mx_qkv_norm_rope`` under ``mx_kernel`` 0; 1 = the
    persistent 256 x 256 kernel where the launch fills it and is eligible -- "mxfp8" activations with "mxfp8" OR "mxfp4"
    weights, the same bits; 2 (tests) = without the tile count; 16 + one of them (``_hip.MX_KERNEL_FP6``; 17, 18; 16 = 0) =
    the same, and "mxfp6" activations (with "mxfp6" or "mxfp4" weights) and "mxfp6" output of the quantising epilogue are
    admitted to that kernel as well -- without the flag they stay tiled.  The epilogue follows from the arguments: ``out_scales``
    given = the quantising one (``out`` = the output codes, ``out_fmt``; returns ``(out, out_scales)``); ``norm`` given = the
    q/k-norm + RoPE one (a dict: qw, qb, kw, kb, cos, sin, text_rows and optionally eps, k_scale, tensors, stats; ``split``
    required; returns False, nothing launched, where the library declines the shape); else the bf16 one of ``gemm_mx``, which
    alone takes ``bias_rowscale`` (fp32 [batch * M], as for ``gemm``).  A ``norm`` dict with a ``stats`` table goes to
    ``gemm_mx_qkv_norm_rope(..., kernel=kernel, stats=...)``: bya_mx_gemm_call has no place for a table, and
    bya_gemm_mx_qkv_norm_rope_stats reads ``kernel`` as this call does."""
    if norm is not None and norm.get("stats") is not None:
        return _mx_call_with_stats(gemm_mx_qkv_norm_rope, a_codes, a_scales, w_codes, w_scales, out, kernel, fmt, w_fmt, bias, split, norm,
                                   (res, gate0, gate1, act, out_scales, bias_rowscale), alpha)
    c, d, n, name = _mx_call(a_codes, a_scales, w_codes, w_scales, out, kernel, fmt, w_fmt, bias, res, gate0, gate1, split,
                             (gate_split, gate_batch_stride, act, bias_rowscale, alpha), out_scales, out_fmt, norm, False)
    if not _launch("bya_gemm_mx_call", _SHAPE_LABELS and _label(d, f":{name}:k{int(kernel)}:{fmt}*{w_fmt or fmt}", act), d,
                   ("bya_gemm_mx_call", (ctypes.byref(c), ctypes.byref(d))), name == "qkn"):
        return False
    return True if name == "qkn" else (out, out_scales) if name == "quant" else out


def gemm_mx_call_plan(a_codes, a_scales, w_codes, w_scales, out, kernel=0, fmt="mxfp8", w_fmt=None, bias=None, res=None,
                      gate0=None, gate1=None, gate_split=0, gate_batch_stride=0, act=None, split=None, alpha=1.0,
                      out_scales=None, out_fmt=None, norm=None, bias_rowscale=None):
    """What ``gemm_mx_call`` would run (``gemm_plan``'s dict): path "t128x128", "t256x256" (mxfp6 activations only) or "p256"
    (``kernel`` 1 or 2, "mxfp8" activations, "mxfp8" or "mxfp4" weights and "mxfp8" output; ``kernel`` 17 or 18: "mxfp6"
    activations and / or "mxfp6" output too); None where the q/k-norm epilogue declines the shape."""
    if norm is not None and norm.get("stats") is not None:
        return _mx_call_with_stats(gemm_mx_qkv_norm_rope_plan, a_codes, a_scales, w_codes, w_scales, out, kernel, fmt, w_fmt, bias, split,
                                   norm, (res, gate0, gate1, act, out_scales, bias_rowscale), alpha)
    c, d, n, name = _mx_call(a_codes, a_scales, w_codes, w_scales, out, kernel, fmt, w_fmt, bias, res, gate0, gate1, split,
                             (gate_split, gate_batch_stride, act, bias_rowscale, alpha), out_scales, out_fmt, norm, True)
    return _plan(("bya_gemm_mx_call", (ctypes.byref(c), ctypes.byref(d))), name == "qkn")


# ---- the small step kernels.  A ``_*_call`` body serves a launch (``plan`` False) and its query (True): -> (entry point, the
# arguments of the launch up to the stream, or of ``<entry point>_plan`` up to the answer).
def _step_plan(p, kernel):
    return {"kernel": kernel, "grid": p.grid, "rounds": p.rounds, "items": p.items, "items_per_round": p.items_per_round}


def _lin_call(x, w, bias, out, silu_in, act_out, plan):
    q = _plan_p if plan else _p
    M, K = x.shape
    N = w.shape[0]
    assert x.is_contiguous() and w.is_contiguous() and out.is_contiguous() and out.shape == (M, N)
    assert x.dtype == w.dtype == out.dtype == torch.bfloat16 and w.shape[1] == K
    return "bya_linear_small_m", ((q(x), q(w), q(out), M, N, K, ACT[act_out]) if plan else
                                  (q(x), q(w), q(bias), q(out), M, N, K, int(silu_in), ACT[act_out]))


def linear_small_m(x, w, bias, out, silu_in=False, act_out=None):
    """out[M<=8, N] = f(x) @ w.T + bias (weight-streaming kernel)."""
    _launch(None, None, 0.0, _lin_call(x, w, bias, out, silu_in, act_out, False))
    return out


def linear_small_m_plan(x, w, out, act_out=None):
    """What ``linear_small_m`` would launch (meta tensors will do): {"kernel": rows of the instantiation (2 / 8), "grid", "rounds"
    (trips of lane 0 over K), "items" (output columns = waves with work), "items_per_round"}."""
    return _plan(_lin_call(x, w, None, out, False, act_out, True), False, _hip.StepPlan, lambda p: _step_plan(p, p.kernel))


def timestep_features(timesteps, out, flip_sin_to_cos=True, freq_shift=0.0):
    assert timesteps.dtype == torch.int64 and timesteps.is_cuda and out.dtype == torch.bfloat16
    b, dim = out.shape
    _launch(None, None, 0.0, ("bya_timestep_features", (_p(timesteps), _p(out), b, dim, int(flip_sin_to_cos), float(freq_shift))))
    return out


# ---- LayerNorm into its four output kinds, and the q/k norm + RoPE
def _code_rows(q, batch, rows, row_bytes, name, plan=False):
    """-> (row stride, batch stride) in bytes of a uint8 code matrix: contiguous [batch * rows * row_bytes] bytes in any shape,
    or a strided view [(batch,) rows, row_bytes] with unit inner stride (rows padded to a wider pitch).  A query reads a
    [(batch,) rows, width] matrix by its strides even where it is contiguous (2-D: batch stride 0, as ``_mat`` has it), and leaves
    the width to the library to judge."""
    assert q.dtype == torch.uint8, f"{name}: expected uint8"
    matrix = q.dim() in (2, 3) and q.stride(-1) == 1 and q.shape[-2] == rows
    if q.is_contiguous() and not (plan and matrix):
        assert q.numel() == batch * rows * row_bytes, f"{name}: {q.numel()} bytes for {batch} x {rows} rows of {row_bytes}"
        return row_bytes, rows * row_bytes
    assert matrix and (plan or tuple(q.shape) in ((rows, row_bytes), (batch, rows, row_bytes))), f"{name}: shape {tuple(q.shape)}"
    return q.stride(-2), q.stride(0) if q.dim() == 3 else 0


def _ln_call(x, out, scales, kind, params, split, mod_batch_stride, eps, plan):
    """LayerNorm of ``x`` into ``out``: bf16 (``kind`` "bf16"), or the uint8 codes of "fp8" / "mxfp8" / "mxfp6" with their
    ``scales`` (a launch's; a query has none).  ``params``: weight, bias, shift0, scale0, shift1, scale1."""
    q = _plan_p if plan else _p
    last = _hip.LN_OUT_KINDS[kind] if plan else mx_fmt_code(kind) if kind.startswith("mx") else None
    xb, rows, D, x_bs, ldx = _mat(x, "x", plan)
    if kind == "bf16":
        ob, rows_o, Do, y_bs, ldy = _mat(out, "out", plan)
        assert (xb, rows, D) == (ob, rows_o, Do)
    else:
        ldy, y_bs = _code_rows(out, xb, rows, D if kind == "fp8" else mx_code_bytes(D, kind), "q" if kind == "fp8" else "codes", plan)
    outs = (q(out),)
    if not plan and kind != "bf16":                  # (a launch's scales: fp32 per row, or an e8m0 byte per block of 32)
        dtype, n = (torch.float32, xb * rows) if kind == "fp8" else (torch.uint8, xb * rows * (D // 32))
        assert scales.dtype == dtype and scales.is_contiguous() and scales.numel() == n
        outs = (q(out), q(scales))
    args = (q(x), *outs, *(q(t) for t in params), rows, xb, D, ldx, ldy, x_bs, y_bs, mod_batch_stride, split)
    # (the four kinds have one query: the kind is its last argument)
    entry ="bya_layernorm" if plan or kind == "bf16" else "bya_layernorm_fp8" if kind == "fp8" else "bya_layernorm_mx"
    return entry, (*args, last) if plan else (*args, float(eps)) if last is None else (*args, float(eps), last)


def layernorm(x, out, weight=None, bias=None, eps=1e-5, shift0=None, scale0=None, shift1=None, scale1=None,
              split=0, mod_batch_stride=0):
    """LayerNorm over the last dim (+ affine, + AdaLN modulation: rows < split use (shift0, scale0))."""
    _launch(None, None, 0.0, _ln_call(x, out, None, "bf16", (weight, bias, shift0, scale0, shift1, scale1), split, mod_batch_stride, eps,
                                      False))
    return out


def layernorm_fp8(x, q, q_scale, weight=None, bias=None, eps=1e-5, shift0=None, scale0=None, shift1=None, scale1=None,
                  split=0, mod_batch_stride=0):
    """``layernorm`` + ``quantize_rows_fp8`` of its output in one pass (same bytes, no bf16 round trip)."""
    _launch(None, None, 0.0, _ln_call(x, q, q_scale, "fp8", (weight, bias, shift0, scale0, shift1, scale1), split, mod_batch_stride, eps,
                                      False))
    return q, q_scale


def layernorm_mx(x, codes, scales, fmt="mxfp6", weight=None, bias=None, eps=1e-5, shift0=None, scale0=None, shift1=None,
                 scale1=None, split=0, mod_batch_stride=0):
    """``layernorm`` + ``quantize_mx`` of its bf16-rounded output in one pass (same bytes, no bf16 round trip)."""
    mx_fmt_code(fmt)                                 # ("mxfp4" is a weight format, "bf16" / "fp8" are other wrappers')
    _launch(None, None, 0.0, _ln_call(x, codes, scales, fmt, (weight, bias, shift0, scale0, shift1, scale1), split, mod_batch_stride, eps,
                                      False))
    return codes, scales


def layernorm_plan(x, out, weight=None, bias=None, shift0=None, scale0=None, shift1=None, scale1=None, split=0,
                   mod_batch_stride=0, out_kind="bf16"):
    """What ``layernorm`` (``out_kind`` "bf16"), ``layernorm_fp8`` ("fp8") or ``layernorm_mx`` ("mxfp8" / "mxfp6") would run
    (host-side, launches nothing; device or meta tensors): {"kernel" (``_hip.LN_KERNELS``), "vec", "nv", "modulated",
    "rows_per_wave", "waves", "grid"}.  ``out``: the bf16 output, or the uint8 code matrix [(B,) rows, row bytes] of the quantised
    forms.  Parameters: tensors, or True for "some aligned vector"."""
    call = _ln_call(x, out, None, out_kind, (weight, bias, shift0, scale0, shift1, scale1), split, mod_batch_stride, 0.0, True)
    return _plan(call, False, _hip.LayerNormPlan, lambda p: {
        "kernel": _hip.LN_KERNELS[p.kernel], "vec": p.vec, "nv": p.nv, "modulated": bool(p.modulated), "rows_per_wave": p.rows_per_wave,
        "waves": p.waves, "grid": p.grid})


def _qkn_rope_call(q, k, params, cos, sin, heads, text_rows, eps, k_scale, stats, plan):
    """``params``: qw, qb, kw, kb.  A query may name its operands loosely: True for a present tensor, a slot count for ``stats``."""
    ptr = _plan_p if plan else _p
    layout = b, S, _, bs, ld = _mat(q if q is not None else k, "q", plan)
    assert q is None or k is None or _mat(k, "k", plan) == layout
    if plan and isinstance(stats, int):
        ps, slots = _META_BASE, stats
    elif stats is not None:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.dim() == 3 and stats.shape[1:] == (2, b * heads)
        ps, slots = ptr(stats), stats.shape[0]
    else:
        ps, slots = None, 0
    if cos is not None and cos is not True:
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
        assert cos.shape == (S - text_rows, 64)
    args = (ptr(q), ptr(k), *(ptr(t) for t in params), ptr(cos), ptr(sin), b, S, heads, ld, bs if b > 1 else 0, text_rows)
    return "bya_qknorm_rope", (*args, ps, slots) if plan else (*args, float(eps), float(k_scale), ps, slots)


def qknorm_rope(q, k, qw, qb, kw, kb, cos, sin, heads, text_rows, eps=1e-6, k_scale=1.0, stats=None):
    """In place on q, k [B, S, heads*64]; q or k may be None (only the other one is processed).  ``stats``: fp32
    [slots, 2, B * heads], ZEROED by the caller: the kernel raises its entries to the squared norms of the rows it writes
    (max over the slots = max ||q||^2, max ||k||^2 per (batch, head): the data-dependent score bound of ``attention``)."""
    _launch(None, None, 0.0, _qkn_rope_call(q, k, (qw, qb, kw, kb), cos, sin, heads, text_rows, eps, k_scale, stats, False))


def qknorm_rope_plan(q, k, heads, text_rows, cos=True, stats=None):
    """What ``qknorm_rope`` would run (host-side; device or meta tensors): {"stats" (the STATS instance), "only" (0: q and k,
    1: q alone, 2: k alone), "slots", "pairs" ((row, head) pairs: q's, then k's), "waves" (8 pairs each), "grid"}.  ``cos``: None,
    True (tables present) or the tensor; ``stats``: None, the number of slots, or the tensor."""
    call = _qkn_rope_call(q, k, (True,) * 4, cos, cos, heads, text_rows, 0.0, 0.0, stats, True)
    return _plan(call, False, _hip.QkNormRopePlan, lambda p: {
        "stats": bool(p.stats), "only": p.only, "slots": p.slots, "pairs": p.pairs, "waves": p.waves, "grid": p.grid})


# ---- attention.  (call tag, softmax variant) -> launches since the last reset; the variant is reported by the library itself
ATTN_VARIANT_NAMES = _hip.ATTN_VARIANTS
ATTN_BOUND_LIMIT = 90.0          # BYA_ATTN_BOUND_LIMIT (include/bya.h): |score| <= 90 keeps P = exp2(s) and its row sums normal
ATTN_VARIANTS = {}
KV_MIX_FORMS = _hip.KV_MIX_FORMS
MIX_MAX_SEGMENTS = _hip.MIX_MAX_SEGMENTS        # segments of one attn_kv_mix_segments launch
TINY_INSTANCES = _hip.TINY_INSTANCES


def _attn_desc(head_dim, heads, nb1, nb2, Sq, Skv, q_strides, k_strides, v_strides, o_strides, scale, prescaled, score_bound,
               bound, plan=False):
    d = AttnDesc()
    d.head_dim, d.heads, d.nb1, d.nb2, d.Sq, d.Skv = head_dim, heads, nb1, nb2, Sq, Skv
    d.q_s1, d.q_s2, d.q_row = q_strides
    d.k_s1, d.k_s2, d.k_row = k_strides
    d.v_s1, d.v_s2, d.v_row = v_strides
    d.o_s1, d.o_s2, d.o_row = o_strides
    d.scale = float(scale)
    d.scores_prescaled = int(prescaled)
    d.score_bound = float(score_bound)
    if bound is not None:
        stats, bh0, flags = bound
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.dim() == 3 and stats.shape[1] == 2
        assert flags.dtype == torch.int32 and flags.is_contiguous() and flags.numel() >= nb1 * nb2 * heads
        d.bound_dev, d.bound_slots, d.bound_heads, d.bound_bh0 = (_plan_p if plan else _p)(stats), stats.shape[0], stats.shape[2], int(bh0)
        d.fallback_flags = (_plan_p if plan else _p)(flags)
    return d


def _mx_out_pair(mx_out, who, plan):
    """``mx_out`` = (codes, scales, fmt) -> (codes, scales, format code): uint8 device tensors (a query: or meta tensors) in an
    activation format.  Where the rows lie is the caller's rule."""
    codes, scales, fmt = mx_out
    code = mx_fmt_code(fmt)                          # "mxfp4" is a weight format: refused here like everywhere for activations
    for t, name in ((codes, "codes"), (scales, "scales")):
        if t.dtype != torch.uint8:
            raise TypeError(f"{who}: mx_out {name}: expected uint8, got {t.dtype}")
        if not (t.is_cuda or (plan and t.is_meta)):
            raise ValueError(f"{who}: mx_out {name}: expected a device tensor")
    return codes, scales, code


def _attn_mx_out(mx_out, heads, head_dim, nb1, nb2, Sq, o_strides, plan=False):
    """``mx_out`` = (codes, scales, fmt) of ``attention`` -> (codes, scales, format code, the six byte strides).  The pair holds the
    [nb1 * nb2 * Sq, heads * 64] output as ``quantize_mx`` would: uint8 codes [.., heads * 64 * bits / 8], uint8 scales [.., heads
    * 2], contiguous, batches stacked (level 1 over level 2 over rows)."""
    if o_strides is not None and tuple(o_strides) != (0, 0, 0):
        raise ValueError("attention: with mx_out there is no bf16 output -- pass out=None and no o_strides")
    codes, scales, code = _mx_out_pair(mx_out, "attention", plan)
    if head_dim != 64:
        raise ValueError("attention: mx_out needs head_dim 64 (one MX block per 32 columns, two per head)")
    rows, cb, sb = nb1 * nb2 * Sq, mx_code_bytes(heads * 64, mx_out[2]), heads * 2
    for t, name, width in ((codes, "codes", cb), (scales, "scales", sb)):
        if not t.is_contiguous() or t.numel() != rows * width or t.shape[-1] != width:
            raise ValueError(f"attention: mx_out {name} must be a contiguous [{rows} rows, {width}] uint8 tensor, got "
                             f"{tuple(t.shape)}")
    return codes, scales, code, (nb2 * Sq * cb, Sq * cb, cb, nb2 * Sq * sb, Sq * sb, sb)


def _attn_call(qkv, out, mx_out, workspace, plan, head_dim, heads, nb1, nb2, Sq, Skv, q_strides, k_strides, v_strides, o_strides, scale,
               prescaled, score_bound, bound):
    """-> (descriptor, ``_attn_mx_out``'s tuple or None, the call) of an attention launch (``qkv`` = (q, k, v)) or its query (()).
    The query's call carries ``workspace``: None = as the launch finds it."""
    ptr = _plan_p if plan else _p
    mx = None
    if mx_out is not None:
        if out is not None:
            raise ValueError("attention: with mx_out there is no bf16 output -- pass out=None")
        mx = _attn_mx_out(mx_out, heads, head_dim, nb1, nb2, Sq, o_strides, plan)
        o_strides = (0, 0, 0)
    for t in qkv + (() if mx is not None else (out,)):
        assert t.dtype == torch.bfloat16 and (t.is_cuda or (plan and t.is_meta))
    d = _attn_desc(head_dim, heads, nb1, nb2, Sq, Skv, q_strides, k_strides, v_strides, o_strides, scale, prescaled,
                   score_bound, bound, plan)
    o = out if mx is None else mx[0]
    if workspace is None and prescaled and (score_bound > 0 or bound is not None) and o.is_cuda and o.device.index not in _ATTN_WS:
        ensure_attn_workspace(o.device)
    if plan:                                         # (bya_attn_plan / bya_attn_mx_plan: no q, k, v, and the workspace to assume)
        if workspace is None:
            workspace = -1 if o.is_cuda else 0
        return d, mx, (("bya_attn", (ctypes.byref(d), ptr(out), int(workspace))) if mx is None else
                       ("bya_attn_mx", (ctypes.byref(d), ptr(mx[0]), ptr(mx[1]), mx[2], *mx[3], int(workspace))))
    q, k, v = qkv
    return d, mx, (("bya_attn_fwd", (ptr(q), ptr(k), ptr(v), ptr(out), ctypes.byref(d))) if mx is None else
                   ("bya_attn_fwd_mx", (ptr(q), ptr(k), ptr(v), ptr(mx[0]), ptr(mx[1]), ctypes.byref(d), mx[2], *mx[3])))


def attention(q, k, v, out, *, head_dim, heads, nb1, nb2, Sq, Skv, q_strides, k_strides, v_strides, o_strides=None,
              scale, tag="other", prescaled=False, score_bound=0.0, bound=None, mx_out=None):
    """Flash attention with explicit (level-1, level-2, row) element strides for q, k, v, out.
    ``bound`` = (stats, bh0, flags): the data-dependent score bound -- ``stats`` fp32 [slots, 2, n] as written by
    ``qknorm_rope(stats=...)``, this launch's (batch, head) index bh at column bh0 + bh, ``flags`` int32 [nb1 * nb2 * heads]
    (scratch: which heads went to the running-maximum kernel).
    ``mx_out`` = (codes, scales, fmt) with ``out`` None (head_dim 64): the output leaves as MX codes and block scales --
    byte for byte ``quantize_mx(out, fmt)`` of the [nb1 * nb2 * Sq, heads * 64] output, which is never written; returns the
    pair, the ``quantised=`` operand of the next MX Linear.  fmt: "mxfp8" or "mxfp6"."""
    d, mx, call = _attn_call((q, k, v), out, mx_out, None, False, head_dim, heads, nb1, nb2, Sq, Skv, q_strides, k_strides, v_strides,
                             o_strides, scale, prescaled, score_bound, bound)
    var = ATTN_VARIANT_NAMES.get(_hip.load().bya_attn_variant(ctypes.byref(d)), "rejected")
    ATTN_VARIANTS[tag, var] = ATTN_VARIANTS.get((tag, var), 0) + 1
    label = _SHAPE_LABELS and f":{nb1}x{nb2}x{heads}h_q{Sq}_kv{Skv}_d{head_dim}" + (f">{mx_out[2]}" if mx is not None else "")
    _launch(":" + tag, label, 4.0 * nb1 * nb2 * heads * Sq * Skv * head_dim, call)
    return (mx[0], mx[1]) if mx is not None else out


def attention_plan(out, *, head_dim, heads, nb1, nb2, Sq, Skv, q_strides, k_strides, v_strides, o_strides=None, scale,
                   prescaled=False, score_bound=0.0, bound=None, workspace=None, mx_out=None):
    """What ``attention`` with the same arguments would run (host-side, launches nothing; meta tensors may stand for device
    tensors): {"variant" (``ATTN_VARIANT_NAMES``), "grid", "q_tile", "stream_k", "sk_rem", "sk_cut", "o_wide", "second_launch"}.
    ``workspace``: True / False = as if a stream-K workspace were / were not registered; None = as the launch would find it
    (a device ``out`` registers the device's workspace like ``attention`` does; with a meta ``out``: none).  ``mx_out`` (with
    ``out`` None): the plan of the MX-output launch; the dict then also has "mx_out": the format."""
    d, mx, call = _attn_call((), out, mx_out, workspace, True, head_dim, heads, nb1, nb2, Sq, Skv, q_strides, k_strides, v_strides,
                             o_strides, scale, prescaled, score_bound, bound)
    plan = _plan(call, False, _hip.AttnPlan, lambda p: {
        "variant": ATTN_VARIANT_NAMES[p.variant], "grid": p.grid, "q_tile": p.q_tile, "stream_k": p.stream_k, "sk_rem": p.sk_rem,
        "sk_cut": p.sk_cut, "o_wide": p.o_wide, "second_launch": p.second_launch})
    assert plan["variant"] == ATTN_VARIANT_NAMES.get(_hip.load().bya_attn_variant(ctypes.byref(d)))
    if mx is not None:
        plan["mx_out"] = mx_out[2]
    return plan


def attention_plan_key(plan):
    """One name per distinct attention kernel path: variant, "+streamk", and the epilogue: "/wide" or "/narrow" (the bf16 store
    width) or "/mxfp8" / "/mxfp6" (the MX-output launch)."""
    tail = "/" + plan["mx_out"] if plan.get("mx_out") else ("/wide" if plan["o_wide"] else "/narrow")
    return plan["variant"] + ("+streamk" if plan["stream_k"] else "") + tail


def self_attention(q, k, v, out, heads, head_dim=64, scale=None, tag="other", prescaled=False, score_bound=0.0, bound=None,
                   mx_out=None):
    """q,k,v,out: [B, S, heads*head_dim] views (row-strided ok).  ``mx_out`` = (codes, scales, fmt) with ``out`` None: see
    ``attention``."""
    b, S, _, q_bs, q_ld = _mat(q, "q")
    _, Skv, _, k_bs, k_ld = _mat(k, "k")
    _, _, _, v_bs, v_ld = _mat(v, "v")
    o_strides = None
    if mx_out is None:
        _, _, _, o_bs, o_ld = _mat(out, "out")
        o_strides = (o_bs, 0, o_ld)
    scale = head_dim ** -0.5 if scale is None else scale
    return attention(q, k, v, out, head_dim=head_dim, heads=heads, nb1=b, nb2=1, Sq=S, Skv=Skv,
                     q_strides=(q_bs, 0, q_ld), k_strides=(k_bs, 0, k_ld), v_strides=(v_bs, 0, v_ld),
                     o_strides=o_strides, scale=scale, tag=tag, prescaled=prescaled, score_bound=score_bound, bound=bound,
                     mx_out=mx_out)


def _mix_mx_out(mx_out, z, z_strides, heads, head_dim, n_grp, Sq, plan=False):
    """``mx_out`` = (codes, scales, fmt) of ``attn_kv_mix`` -> (codes, scales, format code, (c_grp, c_row, sc_grp, sc_row) in
    bytes).  The pair holds rows of the [n_grp * Sq, heads * head_dim] mix as ``quantize_mx`` would: uint8, last dimension
    contiguous and at least heads * head_dim * bits / 8 (codes) / heads * head_dim / 32 (scales) wide.  2-D [n_grp * Sq, width]:
    groups are stacked rows; 3-D [n_grp, Sq, width]: the strides are the tensor's (views of larger buffers are fine)."""
    if z is not None or z_strides is not None:
        raise ValueError("attn_kv_mix: with mx_out there is no bf16 output -- pass z=None and no z_strides")
    codes, scales, code = _mx_out_pair(mx_out, "attn_kv_mix", plan)
    strides = []
    for t, name, width in ((codes, "codes", mx_code_bytes(heads * head_dim, mx_out[2])), (scales, "scales", heads * head_dim // 32)):
        ok = t.dim() in (2, 3) and t.stride(-1) == 1 and t.shape[-1] >= width
        if ok and t.dim() == 2:
            ok = t.shape[0] >= n_grp * Sq
            grp, row = Sq * t.stride(0), t.stride(0)
        elif ok:
            ok = t.shape[0] >= n_grp and t.shape[1] >= Sq
            grp, row = t.stride(0), t.stride(1)
        if not ok:
            raise ValueError(f"attn_kv_mix: mx_out {name} must be uint8 [{n_grp * Sq}, >= {width}] or [{n_grp}, {Sq}, >= {width}] "
                             f"with a contiguous last dimension, got {tuple(t.shape)} strides {tuple(t.stride())}")
        strides += [grp, row]
    return codes, scales, code, tuple(strides)


def _mix_desc(head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides, z_strides, scale):
    d = AttnMixDesc()
    d.head_dim, d.heads, d.n_id, d.n_grp, d.Sq, d.Skv = head_dim, heads, n_id, n_grp, Sq, Skv
    d.q_grp, d.q_row = q_strides
    d.k_id, d.k_grp, d.k_row = k_strides
    d.v_id, d.v_grp, d.v_row = v_strides
    d.z_grp, d.z_row = z_strides
    d.scale = float(scale)
    return d


def _mix_segments(segments):
    """[(K / V group, first row, rows)] -> the bya_attn_mix_segments of ``attn_kv_mix_segments`` (what the entries hold is the
    library's to check; a list the struct cannot hold is refused here: splitting it is the caller's job)."""
    if len(segments) > _hip.MIX_MAX_SEGMENTS:
        raise ValueError(f"attn_kv_mix_segments: {len(segments)} segments, one launch takes at most {_hip.MIX_MAX_SEGMENTS}")
    s = _hip.AttnMixSegments()
    s.n = len(segments)
    for i, (grp, start, length) in enumerate(segments):
        s.grp[i], s.start[i], s.len[i] = grp, start, length
    return s


def _mix_call(qkvr, af, z, wsum, mx_out, plan, head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides, z_strides, scale,
              segments=None):
    """-> (``_mix_mx_out``'s tuple or None, the call) of an ``attn_kv_mix`` launch (``qkvr`` = (q, k, v, r)) or its query (()).
    ``segments`` (``attn_kv_mix_segments``): the launch over that table -- ``n_grp`` then counts K / V groups alone, r, wsum and
    the MX pair hold ``Sq`` rows in all and no group stride."""
    ptr = _plan_p if plan else _p
    row_grps = n_grp if segments is None else 1
    table = None if segments is None else _mix_segments(segments)
    mx = None
    if mx_out is not None:
        mx = _mix_mx_out(mx_out, z, z_strides, heads, head_dim, row_grps, Sq, plan)
        if segments is not None:
            mx = (*mx[:3], (0, mx[3][1], 0, mx[3][3]))
        z_strides = (0, 0)
    d = _mix_desc(head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides, z_strides, scale)
    for t in qkvr + (() if mx is not None else (z,)):
        assert t.dtype == torch.bfloat16 and (t.is_cuda or (plan and t.is_meta))
    assert not qkvr or (qkvr[3].is_contiguous() and qkvr[3].numel() == row_grps * Sq * n_id)
    assert af is None or (af.is_contiguous() and af.dtype == torch.bfloat16 and af.numel() == n_id * n_id)
    assert wsum is None or (wsum.dtype == torch.float32 and wsum.is_contiguous() and wsum.numel() >= row_grps * Sq)
    outs = (ptr(z),) if mx is None else (ptr(mx[0]), ptr(mx[1]))
    tail = (ctypes.byref(d),) if table is None else (ctypes.byref(d), ctypes.byref(table))
    if mx is not None:
        tail += (mx[2], *mx[3])
    return mx, ("bya_attn_kv_mix" + ("" if mx is None else "_mx") + ("" if segments is None else "_seg"),
                (*outs, ptr(af), *tail) if plan else (*(ptr(t) for t in qkvr), ptr(af), *outs, ptr(wsum), *tail))


def _mix_plan_dict(p):
    return {"form": KV_MIX_FORMS[p.form], "head_dim": p.head_dim, "grid": p.grid, "row_chunks": p.row_chunks, "lds_bytes": p.lds_bytes,
            "big_lds": p.big_lds}


def attn_kv_mix(q, k, v, r, af, z, wsum=None, *, head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides,
                z_strides=None, scale, mx_out=None):
    """z[g, n] = sum_id w[g n, id] * softmax(q[g, n] . K[id, g]^T * scale) V[id, g]: cross-attention onto <= 64 keys per identity
    with the router's masked combine in its epilogue.  q_strides = (group, row), k / v_strides = (identity, group, row),
    z_strides = (group, row), in elements; r: bf16 [n_grp * Sq, n_id]; af: None (face) or bf16 [n_id, n_id].
    ``mx_out`` = (codes, scales, fmt) with ``z`` None and no ``z_strides``: the mix leaves as MX codes and block scales
    (layout: ``_mix_mx_out``) -- byte for byte ``quantize_mx(z, fmt)``, z itself never written; returns the pair, the
    ``quantised=`` operand of the next MX Linear, or False (nothing launched, nothing counted) where the library declines (more
    than 32 keys, the generic reference form): the caller then issues the two launches."""
    mx, call = _mix_call((q, k, v, r), af, z, wsum, mx_out, False, head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides,
                         z_strides, scale)
    launched = _launch(None, None, 4.0 * n_id * n_grp * heads * Sq * Skv * head_dim, call, mx is not None)
    return z if mx is None else launched and (mx[0], mx[1])


def attn_kv_mix_plan(z, af=None, *, head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides, z_strides=None,
                     scale=1.0, mx_out=None):
    """What ``attn_kv_mix`` would run (host-side; meta tensors may stand for device tensors): {"form" (``KV_MIX_FORMS``),
    "head_dim", "grid", "row_chunks", "lds_bytes", "big_lds"}.  ``mx_out`` (with ``z`` None): the plan of the MX-output launch
    (the dict then also has "mx_out": the format); None where the library declines it (more than 32 keys, or the generic
    reference form)."""
    mx, call = _mix_call((), af, z, None, mx_out, True, head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides,
                         z_strides, scale)
    plan = _plan(call, mx is not None, _hip.AttnMixPlan, _mix_plan_dict)
    if plan is not None and mx is not None:
        plan["mx_out"] = mx_out[2]
    return plan


def attn_kv_mix_segments(q, k, v, r, af, z, wsum=None, *, segments, head_dim, heads, n_id, n_grp, Sq, Skv, q_row, k_strides, v_strides,
                         z_row=None, scale, mx_out=None):
    """``attn_kv_mix`` for rows cut into ``segments`` = [(grp, start, length)], at most 16, ascending and disjoint: rows
    [start, start + length) of q / r / z / wsum (``Sq`` rows in all, row strides ``q_row`` / ``z_row``, no group stride) attend to
    K / V group ``grp`` < ``n_grp``; rows in no segment are neither read nor written.  One launch, byte for byte the
    ``attn_kv_mix(..., n_grp=1, Sq=length)`` launches per segment on views advanced by ``start`` rows.  ``mx_out`` as there (``z``
    None, no ``z_row``; the pair holds ``Sq`` rows).  Returns z, or the MX pair, or False (nothing launched, nothing counted)
    where the library has no segment form (more than 32 keys, the generic reference form, a z that is not 16-byte aligned,
    head_dim 128): the caller then issues those launches."""
    mx, call = _mix_call((q, k, v, r), af, z, wsum, mx_out, False, head_dim, heads, n_id, n_grp, Sq, Skv, (0, q_row), k_strides, v_strides,
                         None if z_row is None else (0, z_row), scale, segments)
    launched = _launch(None, None, 4.0 * n_id * heads * Skv * head_dim * sum(s[2] for s in segments), call, True)
    return launched and (z if mx is None else (mx[0], mx[1]))


def attn_kv_mix_segments_plan(z, af=None, *, segments, head_dim, heads, n_id, n_grp, Sq, Skv, q_row, k_strides, v_strides, z_row=None,
                              scale=1.0, mx_out=None):
    """What ``attn_kv_mix_segments`` would run (host-side; meta tensors may stand for device tensors): ``attn_kv_mix_plan``'s
    dict -- "form" "mix32", "row_chunks" those of the longest segment, "grid" = row_chunks * heads * len(segments) -- or None
    where the library declines the segment form."""
    mx, call = _mix_call((), af, z, None, mx_out, True, head_dim, heads, n_id, n_grp, Sq, Skv, (0, q_row), k_strides, v_strides,
                         None if z_row is None else (0, z_row), scale, segments)
    plan = _plan(call, True, _hip.AttnMixPlan, _mix_plan_dict)
    if plan is not None and mx is not None:
        plan["mx_out"] = mx_out[2]
    return plan


def _sample_stride(t, n, name):
    """Elements from one sample to the next of a tensor whose first dimension is the batch; one sample for the whole batch
    (shape[0] == 1) is a stride of 0."""
    if t.shape[0] not in (1, n):
        raise ValueError(f"{name}: first dimension {t.shape[0]}, expected the {n} samples of the batch (or 1: shared)")
    return t.stride(0) if t.shape[0] > 1 else 0


def _mix_batch_call(qkvr, af, z, wsum, mx_out, plan, n, **kw):
    """``_mix_call`` for sample 0 of tensors that carry the batch in front, with the bya_attn_mix_samples / _mx_samples of their
    first-dimension strides behind the arguments: the call of ``attn_kv_mix_batch`` or its query."""
    first = lambda t: None if t is None else t[0]
    mx0 = None if mx_out is None else (mx_out[0][0], mx_out[1][0], mx_out[2])
    mx, (entry, args) = _mix_call(tuple(first(t) for t in qkvr), first(af), first(z), first(wsum), mx0, plan, **kw)
    s = _hip.AttnMixSamples() if mx is None else _hip.AttnMixMxSamples()
    s.n = n
    for name, t in zip("qkvr", qkvr):
        setattr(s, name, _sample_stride(t, n, name))
    s.af = 0 if af is None else _sample_stride(af, n, "af")
    s.wsum = 0 if wsum is None else _sample_stride(wsum, n, "wsum")
    if mx is None:
        s.z = _sample_stride(z, n, "z")
    else:
        s.codes, s.scales = _sample_stride(mx_out[0], n, "mx_out codes"), _sample_stride(mx_out[1], n, "mx_out scales")
    return mx, (entry + "_batch", (*args, s))


def attn_kv_mix_batch(q, k, v, r, af, z, wsum=None, *, head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides,
                      z_strides=None, scale, mx_out=None):
    """``attn_kv_mix`` for a batch of samples in ONE launch: every tensor carries the batch in front -- q [n, ..], k / v [n, ..],
    r [n or 1, n_grp * Sq, n_id] (1: one forcing tensor for the whole batch), af None or [n, n_id, n_id], z [n, ..], wsum None or
    [n, n_grp * Sq], ``mx_out`` = (codes [n, ..], scales [n, ..], fmt) -- and the strides given are those WITHIN a sample, as for
    ``attn_kv_mix`` on ``q[b]``, ``k[b]`` ...  Byte for byte those n launches.  Returns z, or the MX pair, or False (nothing
    launched, nothing counted) where the library has no batch form (more than 32 keys, the generic reference form, a z that is
    not 16-byte aligned in every sample): the caller then issues the launches per sample."""
    n = q.shape[0]
    mx, call = _mix_batch_call((q, k, v, r), af, z, wsum, mx_out, False, n, head_dim=head_dim, heads=heads, n_id=n_id, n_grp=n_grp, Sq=Sq,
                               Skv=Skv, q_strides=q_strides, k_strides=k_strides, v_strides=v_strides, z_strides=z_strides, scale=scale)
    launched = _launch(None, None, 4.0 * n * n_id * n_grp * heads * Sq * Skv * head_dim, call, True)
    return launched and (z if mx is None else (mx_out[0], mx_out[1]))


def attn_kv_mix_batch_plan(z, af=None, *, n, head_dim, heads, n_id, n_grp, Sq, Skv, q_strides, k_strides, v_strides, z_strides=None,
                           scale=1.0, mx_out=None, sample_strides=None):
    """What ``attn_kv_mix_batch`` would run (host-side; meta tensors may stand for device tensors): ``attn_kv_mix_plan``'s dict of
    ONE sample with "grid" multiplied by ``n`` -- or None where the library declines the batch form.  z / af / the MX pair carry
    the batch in front; ``sample_strides`` = {"q", "k", "v", "r", "wsum": elements from one sample to the next} for the operands
    the query does not see (default: 0)."""
    mx0 = None if mx_out is None else (mx_out[0][0], mx_out[1][0], mx_out[2])
    mx, (entry, args) = _mix_call((), None if af is None else af[0], None if z is None else z[0], None, mx0, True, head_dim, heads, n_id,
                                  n_grp, Sq, Skv, q_strides, k_strides, v_strides, z_strides, scale)
    s = _hip.AttnMixSamples() if mx is None else _hip.AttnMixMxSamples()
    s.n = n
    for name, val in (sample_strides or {}).items():
        setattr(s, name, val)
    s.af = 0 if af is None else _sample_stride(af, n, "af")
    if mx is None:
        s.z = _sample_stride(z, n, "z")
    else:
        s.codes, s.scales = _sample_stride(mx_out[0], n, "mx_out codes"), _sample_stride(mx_out[1], n, "mx_out scales")
    plan = _plan((entry + "_batch", (*args, s)), True, _hip.AttnMixPlan, _mix_plan_dict)
    if plan is not None and mx is not None:
        plan["mx_out"] = mx_out[2]
    return plan


def _tiny_call(q, k, v, out, L, heads, n_outer, n_inner, strides, ld_qkv, ld_o, scale, plan):
    ptr = _plan_p if plan else _p
    args = (ptr(q), ptr(k), ptr(v), ptr(out), L, heads, n_outer, n_inner)
    return "bya_attn_tiny", (*args, ld_qkv, ld_o) if plan else (*args, *strides, ld_qkv, ld_o, float(scale))


def attn_tiny(q, k, v, out, L, heads, n_outer, n_inner, outer_stride, seq_stride, ld_qkv, ld_o, scale):
    _launch(None, None, 0.0, _tiny_call(q, k, v, out, L, heads, n_outer, n_inner, (outer_stride, seq_stride), ld_qkv, ld_o, scale, False))
    return out


def attn_tiny_plan(q, k, v, out, L, heads, n_outer, n_inner, ld_qkv, ld_o):
    """Which of the eight ``attn_tiny`` kernel instances would run: {"instance" (``TINY_INSTANCES``), "grid", "waves"}."""
    return _plan(_tiny_call(q, k, v, out, L, heads, n_outer, n_inner, (), ld_qkv, ld_o, 0.0, True), False, _hip.AttnTinyPlan,
                 lambda p: {"instance": TINY_INSTANCES[p.instance], "grid": p.grid, "waves": p.waves})


# ---- the embedding router's scores, head and combines; patches; the activation; the scheduler step
def _scores_call(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, eps, plan):
    ptr = _plan_p if plan else _p
    for t in (qr, kr, ln_w, ln_b, pos_emb, out):
        assert t.is_contiguous() and t.dtype == torch.bfloat16
    args = (ptr(qr), ptr(kr), ptr(ln_w), ptr(ln_b), ptr(pos_emb), ptr(out), n_id, N, 16, 32)
    return "bya_router_scores", args if plan else (*args, float(eps))


def router_scores(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, eps=1e-5):
    _launch(None, None, 2.0 * n_id * N * 32 * qr.shape[-1], _scores_call(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, eps, False))
    return out


def router_scores_plan(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N):
    """What ``router_scores`` would launch (meta tensors will do): {"kernel": "wave" / "lds", "grid", "rounds", "items" (16-token
    tiles per identity), "items_per_round" (tiles of one identity per round of the waves' walk)}."""
    return _plan(_scores_call(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, 0.0, True), False, _hip.StepPlan,
                 lambda p: _step_plan(p, _hip.ROUTER_SCORES_KERNELS[p.kernel]))


def router_head(x, w, b, r, n_id, N):
    assert x.is_contiguous() and r.is_contiguous()
    _launch(None, None, 0.0, ("bya_router_head", (_p(x), _p(w), _p(b), _p(r), n_id, N, x.shape[-1])))
    return r


def _scores_batch_call(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, eps, plan):
    """``_scores_call`` for sample 0 of qr [n, N, 2048], kr [n, n_id, 32, 2048] and out [n, n_id, N, 512] with the
    bya_router_scores_samples of their first-dimension strides behind the arguments."""
    for t in (qr, kr, out):
        assert t[0].is_contiguous()
    entry, args = _scores_call(qr[0], kr[0], ln_w, ln_b, pos_emb, out[0], n_id, N, eps, plan)
    s = _hip.RouterScoresSamples()
    s.n = out.shape[0]
    s.qr, s.kr, s.out = _sample_stride(qr, s.n, "qr"), _sample_stride(kr, s.n, "kr"), _sample_stride(out, s.n, "out")
    return entry + "_batch", (*args, s)


def router_scores_batch(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, eps=1e-5):
    """``router_scores`` for the samples of a batch in ONE launch: qr [n, N, 2048], kr [n, n_id, 32, 2048], out [n, n_id, N, 512]
    (each sample contiguous); byte for byte ``router_scores(qr[b], kr[b], ..., out[b])`` for every b.  Returns out, or False where
    the library declines."""
    n = out.shape[0]
    return _launch(None, None, 2.0 * n * n_id * N * 32 * qr.shape[-1], _scores_batch_call(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, eps, False),
                   True) and out


def router_scores_batch_plan(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N):
    """What ``router_scores_batch`` would launch (meta tensors will do): ``router_scores_plan``'s dict of one sample with "grid"
    multiplied by the samples; None where the library declines."""
    return _plan(_scores_batch_call(qr, kr, ln_w, ln_b, pos_emb, out, n_id, N, 0.0, True), True, _hip.StepPlan,
                 lambda p: _step_plan(p, _hip.ROUTER_SCORES_KERNELS[p.kernel]))


def _head_batch_call(x, w, b, r, n_id, N, plan):
    ptr = _plan_p if plan else _p
    assert x[0].is_contiguous() and r[0].is_contiguous()
    s = _hip.RouterHeadSamples()
    s.n = x.shape[0]
    s.x, s.r = _sample_stride(x, s.n, "x"), _sample_stride(r, s.n, "r")
    return "bya_router_head_batch", (ptr(x), ptr(w), ptr(b), ptr(r), n_id, N, x.shape[-1], s)


def router_head_batch(x, w, b, r, n_id, N):
    """``router_head`` for the samples of a batch in ONE launch: x [n, n_id, N, D], r [n, N, n_id] (each sample contiguous).
    Returns r, or False where the library declines."""
    return _launch(None, None, 0.0, _head_batch_call(x, w, b, r, n_id, N, False), True) and r


def router_head_batch_plan(x, w, b, r, n_id, N):
    """What ``router_head_batch`` would launch (meta tensors will do): {"kernel": "rows", "grid" = ceil(N * n_id / 4) * samples,
    "rounds", "items" (= N * n_id, one wave each), "items_per_round"}; None where the library declines."""
    return _plan(_head_batch_call(x, w, b, r, n_id, N, True), True, _hip.StepPlan, lambda p: _step_plan(p, "rows"))


def forcing_max_over_frames(forcing, out, frames, per_frame, n_id):
    assert forcing.is_contiguous() and out.is_contiguous() and forcing.dtype == out.dtype == torch.bfloat16
    _launch(None, None, 0.0, ("bya_forcing_max_over_frames", (_p(forcing), _p(out), frames, per_frame, n_id)))
    return out


ROUTE_MODES = {"face": 0, "audio": 1}            # how routing logits become the identities' weights (include/bya.h)


def masked_combine(x, feat, r, af, mode, alpha=1.0):
    """x [B, N, D] view (in place) += combine(feat [B, n_id, N, D], r [B or 1, N, n_id])."""
    b, N, D, x_bs, x_row = _mat(x, "x")
    assert feat.is_contiguous() and feat.shape[0] == b and feat.shape[2] == N and feat.shape[3] == D
    n_id = feat.shape[1]
    assert r.is_contiguous() and r.shape[-2:] == (N, n_id) and r.dtype == torch.bfloat16
    r_bs = 0 if r.shape[0] == 1 else N * n_id
    if af is not None:
        assert af.is_contiguous() and af.dtype == torch.bfloat16 and af.shape == (b, n_id, n_id)
    _launch(None, None, 0.0, ("bya_masked_combine", (_p(x), _p(feat), _p(r), _p(af), ROUTE_MODES[mode], float(alpha), b, n_id, N, D, x_row,
                                                     x_bs, r_bs)))
    return x


def routed_mix(feat, r, af, mode, z, wsum=None):
    """z [B, N, D] = sum_id w[b,n,id] * feat [B, n_id, N, D]; wsum [B, N] fp32 = sum_id w (optional)."""
    b, n_id, N, D = feat.shape
    assert feat.is_contiguous() and z.is_contiguous() and z.shape == (b, N, D)
    assert r.is_contiguous() and r.shape[-2:] == (N, n_id) and r.dtype == torch.bfloat16
    r_bs = 0 if r.shape[0] == 1 else N * n_id
    if wsum is not None:
        assert wsum.dtype == torch.float32 and wsum.is_contiguous() and wsum.numel() == b * N
    _launch(None, None, 0.0, ("bya_routed_mix", (_p(feat), _p(r), _p(af), _p(z), _p(wsum), ROUTE_MODES[mode], b, n_id, N, D, r_bs)))
    return z


def patchify(x, cols):
    b, t, c, h, w = x.shape
    assert x.is_contiguous() and cols.is_contiguous() and x.dtype == cols.dtype == torch.bfloat16
    _launch(None, None, 0.0, ("bya_patchify", (_p(x), _p(cols), b, t, c, h, w)))
    return cols


def unpatchify(y, out):
    b, t, c, h, w = out.shape
    assert y.is_contiguous() and out.is_contiguous() and y.dtype == out.dtype == torch.bfloat16
    _launch(None, None, 0.0, ("bya_unpatchify", (_p(y), _p(out), b, t, c, h, w)))
    return out


def _act_call(x, out, act, res, plan):
    ptr = _plan_p if plan else _p
    assert x.is_contiguous() and out.is_contiguous() and (res is None or res.is_contiguous())
    return "bya_act_add", (ptr(x), ptr(res), ptr(out), x.numel(), ACT[act])


def act_add(x, out, act=None, res=None):
    _launch(None, None, 0.0, _act_call(x, out, act, res, False))
    return out


def act_add_plan(x, out, act=None, res=None):
    """What ``act_add`` would launch (meta tensors will do): {"grid", "rounds" of the grid-stride loop, "items" (16-byte pieces),
    "items_per_round"}."""
    return _plan(_act_call(x, out, act, res, True), False, _hip.StepPlan, lambda p: _step_plan(p, "act_add"))


# ---- the first-block step cache (include/bya.h, "First-block step cache"): three streaming passes over the joint stream
def _cache_tensors(plan, n, **tensors):
    """The bf16 operands of a step-cache pass: contiguous, n elements each (None passes where the entry point allows it)."""
    for name, t in tensors.items():
        if t is None:
            continue
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"{name}: expected a contiguous bf16 tensor of {n} elements")
        if not (t.is_cuda or (plan and t.is_meta)):
            raise ValueError(f"{name}: expected a device tensor (the engine has no CPU path)")


def _probe_call(x, E, r_ref, r_new, partials, sums, plan):
    ptr = _plan_p if plan else _p
    n = x.numel()
    _cache_tensors(plan, n, x=x, E=E, r_ref=r_ref, r_new=r_new)
    head = (ptr(x), ptr(E), ptr(r_ref), ptr(r_new))
    if plan:
        return "bya_step_cache_probe", (*head, n)
    for name, t, least in (("partials", partials, step_cache_probe_plan(x, E, r_ref, r_new)["partials_bytes"] // 8), ("sums", sums, 2)):
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() < least:
            raise ValueError(f"{name}: expected a contiguous fp64 device tensor of at least {least} elements")
    return "bya_step_cache_probe", (*head, _p(partials), _p(sums), n)


def step_cache_probe(x, E, r_ref, r_new, partials, sums):
    """The probe of the first-block step cache: r_new = bf16(x - E), E <- x, sums[0] = sum |r_new - r_ref| and sums[1] =
    sum |r_ref| in fp64 (both 0 where ``r_ref`` is None), through ``partials`` (fp64, ``step_cache_probe_plan``'s
    "partials_bytes") and a one-workgroup finish launch: the same inputs give the same 16 bytes.  Returns ``sums``."""
    _launch(None, None, 0.0, _probe_call(x, E, r_ref, r_new, partials, sums, False))
    return sums


def step_cache_probe_plan(x, E, r_ref, r_new):
    """What ``step_cache_probe`` (and, on the same grid, ``step_cache_capture`` / ``step_cache_apply``) would launch (meta
    tensors will do): {"grid", "vec" (bf16 per lane and pass), "wg_pass_elems", "passes" of workgroup 0, "partials_bytes"}."""
    return _plan(_probe_call(x, E, r_ref, r_new, None, None, True), False, _hip.StepCachePlan,
                 lambda p: {"grid": p.grid, "vec": p.vec, "wg_pass_elems": p.wg_pass_elems, "passes": p.passes,
                            "partials_bytes": p.partials_bytes})


def step_cache_capture(x, E, R):
    """R = bf16(x - E): the residual of blocks 1..L-1 behind a full step (``E`` holds x after block 0).  Returns ``R``."""
    _cache_tensors(False, x.numel(), x=x, E=E, R=R)
    _launch(None, None, 0.0, ("bya_step_cache_capture", (_p(x), _p(E), _p(R), x.numel())))
    return R


def step_cache_apply(x, R):
    """x = bf16(x + R) in place: a re-used step's stand-in for blocks 1..L-1.  Returns ``x``."""
    _cache_tensors(False, x.numel(), x=x, R=R)
    _launch(None, None, 0.0, ("bya_step_cache_apply", (_p(x), _p(R), x.numel())))
    return x


def step_cache_snapshot(x, E):
    """E <- x, the device copy in front of block 0, under a kernel-timer label of its own like every launch of the step."""
    tok = _begin("step_cache_snapshot")
    E.copy_(x)
    _end(tok)
    return E


def _sched_pred(pred, n):
    """-> (n_pred, pred_stride) of a prediction [1 or 2, ...]: the rows may be rows of a wider buffer (stride(0) >= n)."""
    n_pred = pred.shape[0] if pred.numel() != n else 1
    assert pred.dtype == torch.bfloat16 and n_pred in (1, 2) and pred.numel() == n_pred * n
    if n_pred == 1:
        assert pred.is_contiguous()
        return 1, n
    assert pred[0].is_contiguous() and pred.stride(0) >= n
    return 2, pred.stride(0)


def _sched_call(pred, sample, coef, old_x0, noise, x0_out, out, plan):
    """-> (the output: ``out``, or where there is none a launch's new tensor / a query's ``sample``, the call)."""
    ptr = _plan_p if plan else _p
    n = sample.numel()
    n_pred, pred_stride = _sched_pred(pred, n)
    assert sample.dtype == torch.bfloat16 and sample.is_contiguous()
    for t, dt in ((old_x0, torch.float32), (noise, torch.bfloat16), (x0_out, torch.float32)):
        assert t is None or (t.dtype == dt and t.is_contiguous() and t.numel() == n)
    if out is None:
        out = sample if plan else torch.empty_like(sample)
    c = _hip.SchedCoef(**{k: float(v) for k, v in coef.items()})
    head = (ptr(pred), n_pred, pred_stride, ptr(sample))
    return out, ("bya_cfg_scheduler_step", (*head, ptr(out), n, ctypes.byref(c)) if plan else
                 (*head, ptr(old_x0), ptr(noise), ptr(out), ptr(x0_out), n, ctypes.byref(c)))


def cfg_scheduler_step_plan(pred, sample, coef, out=None):
    """What ``cfg_scheduler_step`` would launch (meta tensors will do): {"grid", "rounds" of the grid-stride loop, "items"
    (elements), "items_per_round"}."""
    return _plan(_sched_call(pred, sample, coef, None, None, None, out, True)[1], False, _hip.StepPlan,
                 lambda p: _step_plan(p, "cfg_scheduler_step"))


def cfg_scheduler_step(pred, sample, coef, old_x0=None, noise=None, x0_out=None, out=None):
    """Fused CFG combine + scheduler step (reference models/pipeline_bindyouravatar.py:924-948).
    pred: bf16 [1 or 2, ...] model output ([uncond, cond] when 2; the two may be rows of a wider buffer); sample: bf16
    latents [1, ...] (or any shape with the element count of one prediction); coef: dict with the fields of ``bya_sched_coef``; old_x0 / x0_out: fp32;
    noise: bf16.  Returns the new bf16 latents."""
    out, call = _sched_call(pred, sample, coef, old_x0, noise, x0_out, out, False)
    _launch(None, None, 0.0, call)
    return out


def masks_to_routing_logits(masks, frames=13, h=30, w=45, out=None):
    """Tracking masks uint8 [n_id, T, H, W] (> 0 = foreground) -> ``routing_logits_forcing`` bf16 [1, frames*h*w, n_id]
    (reference util/utils.py:871-936; feed it to ``forward(routing_logits_forcing=...)``)."""
    assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.dim() == 4
    n_id, Ti, Hi, Wi = masks.shape
    if out is None:
        out = torch.empty(1, frames * h * w, n_id, dtype=torch.bfloat16, device=masks.device)
    _launch(None, None, 0.0, ("bya_masks_to_routing_logits", (_p(masks), _p(out), n_id, Ti, Hi, Wi, frames, h, w)))
    return out


# ---- the router's row kernels (K = 512).  A launch reads its rows off the tensors and its weights off a pack; a query may
# name them loosely: a plain row count for ``x`` (contiguous rows, aligned pointers), True for "some aligned" residual, output or
# pack (_SOME_PACK).  Both read row counts and strides in _rows_of / _like_rows.
def pack_rowgemm512(weight, bias, ln_weight=None, ln_bias=None):
    """Pack a [N, 512] Linear (optionally preceded by LayerNorm(512)) for ``rowgemm512``: gamma folded into the bf16
    weight, its fp32 row sums, and the fp32 constant vector  W . beta + bias  (see include/bya.h)."""
    w32 = weight.float()
    b32 = bias.float() if bias is not None else torch.zeros(weight.shape[0], device=weight.device)
    if ln_weight is None:
        return dict(w=weight.to(torch.bfloat16).contiguous(), colsum=None, cvec=b32.contiguous(), ln=False)
    wg = (w32 * ln_weight.float()[None, :]).to(torch.bfloat16).contiguous()
    return dict(w=wg, colsum=wg.float().sum(1).contiguous(), cvec=(w32 @ ln_bias.float() + b32).contiguous(), ln=True)


_SOME_PACK = dict(w=True, colsum=True, cvec=True, ln=True)


def _rows_of(x, ptr, width=512):
    """-> (M, row stride, address) of the [M, width] rows ``x`` (a tensor) or of M contiguous rows (an int: queries)."""
    if isinstance(x, int):
        return x, width, ptr(True)
    (M, K), (ld, inner) = x.shape, x.stride()        # (2-D: anything else does not unpack)
    assert K == width and inner == 1
    return M, ld, ptr(x)


def _like_rows(t, M, width, ptr):
    if t is None or t is True:
        return width, ptr(True)
    assert tuple(t.shape) == (M, width)
    ld, inner = t.stride()
    assert inner == 1
    return ld, ptr(t)


def _rowgemm_call(x, N, pack, out, res, act, eps, nsplit, plan):
    ptr = _plan_p if plan else _p
    M, ldx, px = _rows_of(x, ptr)
    ldc, pc = _like_rows(out, M, N, ptr)
    ldres, pr = _like_rows(res, M, N, ptr) if res is not None else (0, None)
    args = (px, ptr(pack["w"]), ptr(pack["colsum"]), ptr(pack["cvec"]), pr, pc, M, N, ldx, ldc, ldres, int(pack["ln"]))
    return M, ("bya_rowgemm512", (*args, ACT[act]) if plan else (*args, float(eps), ACT[act], int(nsplit)))


def rowgemm512(x, pack, out, res=None, act=None, eps=1e-5, nsplit=0):
    """out = res + act( LN?(x) @ W.T + b ) for K = 512 (router projections, reference models/router.py:468-493)."""
    N = pack["w"].shape[0]
    M, call = _rowgemm_call(x, N, pack, out, res, act, eps, nsplit, False)
    _launch(None, None, 2.0 * M * N * 512, call)
    return out


def rowgemm512_plan(x, N, out=None, ln=False, res=None, act=None):
    """What ``rowgemm512`` would run: {"form" (``_hip.ROWGEMM_FORMS``), "ln", "res", "gelu" (the kernel's template instance),
    "grid", "work_items", "crosses_row_block"}.  ``res``: None, True (some aligned residual) or the tensor."""
    pack = dict(w=True, colsum=True if ln else None, cvec=True, ln=ln)
    return _plan(_rowgemm_call(x, N, pack, out, res, act, 0.0, 0, True)[1], False, _hip.RowGemmPlan, lambda p: {
        "form": _hip.ROWGEMM_FORMS[p.form], "ln": bool(p.ln), "res": bool(p.res), "gelu": p.act == ACT["gelu_erf"], "grid": p.grid,
        "work_items": p.work_items, "crosses_row_block": bool(p.crosses_row_block)})


def _rowk_call(entry, x, packs, out, geometry, floats, tail, plan):
    """The call of one of the three fused row kernels: ``packs`` = (the pack with the LayerNorm folded in, the out-projection's
    or second Linear's pack or None); ``out`` None = in place; ``geometry`` = the groups (L, n_outer, n_inner, outer_stride,
    seq_stride) or (); ``floats`` = eps (, scale): a launch's alone; ``tail`` = (tiles_pass0,) or ().  -> (M, addresses of x and
    out, the call)."""
    ptr = _plan_p if plan else _p
    M, ldx, px = _rows_of(x, ptr)
    ldc, pc = _like_rows(out, M, 512, ptr) if out is not None else (ldx, px)
    first, second = packs
    weights = (ptr(first["w"]), ptr(first["colsum"]), ptr(first["cvec"])) + (() if second is None else (ptr(second["w"]), ptr(second["cvec"])))
    args = (px, *weights, pc, M, ldx, ldc, *(int(g) for g in geometry))
    return M, px, pc, (entry, (*args, *(int(t) for t in tail)) if plan else (*args, *(float(f) for f in floats), *(int(t) for t in tail)))


def _group_attn_call(x, pack, out, groups, floats, plan):
    return _rowk_call("bya_router_group_attn", x, (pack, None), out, groups, floats, (), plan)


def _mlp_call(x, packs, out, floats, tiles_pass0, plan):
    return _rowk_call("bya_router_mlp_fused", x, packs, out, (), floats, (tiles_pass0,), plan)


def _attn_out_call(x, packs, out, groups, floats, tiles_pass0, plan):
    return _rowk_call("bya_router_group_attn_out", x, packs, out, groups, floats, (tiles_pass0,), plan)


def router_group_attn(x, pack, out, L, n_outer, n_inner, outer_stride, seq_stride, eps=1e-5, scale=0.125):
    """out = softmax(q k^T * scale) v per group of L rows, (q | k | v) = LN(x) @ Wqkv.T + b, 8 heads x 64: the temporal /
    multi-ID attention of SpatialTemporalAttentionBlock up to its out-projection in ONE launch (reference
    models/router.py:476-478, :482-484; include/bya.h).  ``pack`` = ``pack_rowgemm512`` of the concatenated
    to_q | to_k | to_v with the LayerNorm folded in; groups as for ``attn_tiny``."""
    assert pack["ln"] and pack["w"].shape == (1536, 512)
    M, px, po, call = _group_attn_call(x, pack, out, (L, n_outer, n_inner, outer_stride, seq_stride), (eps, scale), False)
    assert px != po
    _launch(None, None, 2.0 * M * 1536 * 512 + 4.0 * M * L * 512, call)
    return out


def router_group_attn_plan(x, L, n_outer, n_inner, outer_stride, seq_stride, out=None):
    """What ``router_group_attn`` would run: {"P" (slots per group), "G" (groups per 16-row tile), "wide" (16 < L <= 32: the
    two-tile kernel), "tiles", "blocks"}."""
    call = _group_attn_call(x, _SOME_PACK, True if out is None else out, (L, n_outer, n_inner, outer_stride, seq_stride), (), True)[3]
    return _plan(call, False, _hip.GroupAttnPlan, lambda p: {"P": p.P, "G": p.G, "wide": bool(p.wide), "tiles": p.tiles, "blocks": p.blocks})


def _chain_dict(p):
    return {"tiles": p.tiles, "tp0": p.tp0, "grid": p.grid, "passes": p.passes, "tiles_last": p.tiles_last, "wgs_last": p.wgs_last}


def router_mlp_fused(x, pack1, pack2, eps=1e-5, out=None, tiles_pass0=0):
    """x += mlp[2](GELU(mlp[0](LayerNorm(x)))) on router rows in ONE launch, the hidden activation in registers (reference
    models/router.py:491; include/bya.h).  ``pack1`` = ``pack_rowgemm512`` of mlp[0] with norm4 folded in, ``pack2`` of
    mlp[2].  Bit-identical to ``rowgemm512(x, pack1, h, act="gelu_erf"); rowgemm512(h, pack2, x, res=x)``."""
    assert pack1["ln"] and not pack2["ln"] and pack1["w"].shape == (512, 512) and pack2["w"].shape == (512, 512)
    M, _, _, call = _mlp_call(x, (pack1, pack2), out, (eps,), tiles_pass0, False)
    _launch(None, None, 4.0 * M * 512 * 512, call)
    return x if out is None else out


def router_mlp_fused_plan(x, out=None, tiles_pass0=0):
    """What ``router_mlp_fused`` would run: {"tiles", "tp0", "grid", "passes", "tiles_last" (tiles per workgroup in the last
    pass), "wgs_last" (workgroups that have a tile there)}."""
    return _plan(_mlp_call(x, (_SOME_PACK, _SOME_PACK), out, (), tiles_pass0, True)[3], False, _hip.RouterChainPlan, _chain_dict)


def router_group_attn_out(x, pack, pack_out, L, n_outer, n_inner, outer_stride, seq_stride, eps=1e-5, scale=0.125, out=None,
                          tiles_pass0=0):
    """x += to_out(attention over groups of L rows of LayerNorm(x)) in ONE launch (reference models/router.py:482-483,
    :486-487; include/bya.h): ``router_group_attn`` followed by the out-projection + residual, the attention output in
    registers.  L <= 16.  Bit-identical to the two launches."""
    assert pack["ln"] and pack["w"].shape == (1536, 512) and not pack_out["ln"] and pack_out["w"].shape == (512, 512)
    M, _, _, call = _attn_out_call(x, (pack, pack_out), out, (L, n_outer, n_inner, outer_stride, seq_stride), (eps, scale), tiles_pass0,
                                   False)
    _launch(None, None, 2.0 * M * 2048 * 512 + 4.0 * M * L * 512, call)
    return x if out is None else out


def router_group_attn_out_plan(x, L, n_outer, n_inner, outer_stride, seq_stride, out=None, tiles_pass0=0):
    """What ``router_group_attn_out`` would run (``router_mlp_fused_plan``'s dict; its tiles hold 16 / P whole groups)."""
    call = _attn_out_call(x, (_SOME_PACK, _SOME_PACK), out, (L, n_outer, n_inner, outer_stride, seq_stride), (), tiles_pass0, True)[3]
    return _plan(call, False, _hip.RouterChainPlan, _chain_dict)


# ---- video VAE (csrc/vae.hip) ----------------------------------------------------------
def vae_patches(x, cache, out, KT, stride, pad, up, tmode, Ho, Wo, t0, nt):
    """Patch matrix of a causal KT x 3 x 3 convolution over channels-last x [Ts, Hs, Ws, C] -> out [nt * Ho * Wo, Kpad]."""
    Ts, Hs, Ws, C = x.shape
    assert x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype == torch.bfloat16
    assert cache is None or (cache.is_contiguous() and tuple(cache.shape) == (KT - 1, Hs, Ws, C))
    assert out.shape[0] == nt * Ho * Wo
    _launch(None, None, 0.0, ("bya_vae_patches", (_p(x), _p(cache), _p(out), Ts, Hs, Ws, C, KT, stride, pad, int(up), tmode, Ho, Wo, t0, nt,
                                                  out.shape[1])))
    return out


def vae_groupnorm_stats(x2d, sums, groups, partial=None, moments=False):
    """``sums`` [groups, 2] fp32 = (sum x, sum x^2) per group of x2d [rows, C]; ``moments``: (mean, var) instead, formed in fp64
    before the one rounding (bya_vae_groupnorm_moments; its ``partial`` scratch is fp64) -- what ``vae_norm_act(moments=True)`` reads."""
    rows, C = x2d.shape
    assert x2d.is_contiguous() and sums.dtype == torch.float32 and sums.numel() == 2 * groups
    need = (rows + 511) // 512 * groups * 2
    pdt = torch.float64 if moments else torch.float32
    if partial is None:
        partial = torch.empty(need, dtype=pdt, device=x2d.device)
    assert partial.dtype == pdt and partial.numel() >= need and partial.is_contiguous()
    _launch(None, None, 0.0, ("bya_vae_groupnorm_moments" if moments else "bya_vae_groupnorm_stats",
                              (_p(x2d), _p(sums), _p(partial), rows, C, groups)))
    return sums


def vae_norm_act(x, y, sums, gamma, beta, groups, act="silu", eps=1e-6, zy=None, zb=None, latent_shape=None, tmode=1,
                 out_pad=False, moments=False):
    """x: [T, H, W, C] channels-last; y: the same, or (out_pad) the zero-padded conv input [T + 2, H + 2, W + 2, C] whose
    interior frames 2.. are written; zy / zb: [Tz * hz * wz, C] views (row stride = their .stride(0)).  ``moments``: ``sums``
    holds (mean, var) per group (``vae_groupnorm_stats(moments=True)``) and not (sum x, sum x^2)."""
    T, H, W, C = x.shape
    assert x.is_contiguous() and y.is_contiguous()
    assert tuple(y.shape) == ((T + 2, H + 2, W + 2, C) if out_pad else (T, H, W, C))
    Tz, hz, wz = latent_shape if latent_shape is not None else (T, H, W)
    ldz = zy.stride(0) if zy is not None else 0
    _launch(None, None, 0.0, ("bya_vae_norm_act_moments" if moments else "bya_vae_norm_act",
                              (_p(x), _p(y), _p(sums), _p(gamma), _p(beta), _p(zy), _p(zb), T * H * W, C, groups,
                               {None: 0, "none": 0, "silu": 1}[act], float(eps), T, H, W, Tz, hz, wz, tmode, ldz,
                               int(bool(out_pad)))))
    return y


def vae_conv3d(xpad, w, bias, out, res=None, KT=3):
    """Causal KT x 3 x 3 convolution as an implicit GEMM: xpad [To + KT - 1, H + 2, W + 2, C] zero-padded (KT = 3: its two
    context frames in front), w [Cout, >= 9 KT C] (tap-major columns), out / res [To, H, W, Cout] (out = res + bias + conv)."""
    Tp, Hp, Wp, C = xpad.shape
    To, H, W, Cout = out.shape
    assert (Tp, Hp, Wp) == (To + KT - 1, H + 2, W + 2) and xpad.is_contiguous() and w.is_contiguous() and w.shape[0] >= Cout
    assert out.stride(3) == 1
    ldc = out.stride(2)
    assert out.stride(1) == W * ldc and out.stride(0) == H * W * ldc
    ldres = 0
    if res is not None:
        ldres = res.stride(2)
        assert res.shape == out.shape and res.stride(1) == W * ldres and res.stride(0) == H * W * ldres and res.stride(3) == 1
    _launch(None, None, 2.0 * To * H * W * Cout * 9 * KT * C,
            ("bya_vae_conv3d", (_p(xpad), _p(w), _p(bias), _p(res), _p(out), To, H, W, C, Cout, KT, w.stride(0), ldc, ldres)))
    return out


def vae_upsample_pad(x, ypad, tmode):
    """Nearest up-sampling of x [T, H, W, C] into the interior of the zero-padded ypad [To, 2 H + 2, 2 W + 2, C]."""
    T, H, W, C = x.shape
    To = T if tmode == 0 else (2 * T if tmode == 1 else 2 * T - 1)
    assert x.is_contiguous() and ypad.is_contiguous() and tuple(ypad.shape) == (To, 2 * H + 2, 2 * W + 2, C)
    _launch(None, None, 0.0, ("bya_vae_upsample_pad", (_p(x), _p(ypad), T, H, W, C, tmode)))
    return ypad

