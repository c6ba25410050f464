"""CPU: the host side of the q/k score-bound statistics recorded by the fused q|k|v launches (the ``*_stats`` entry points of
include/bya.h) -- their declarations in the header and in ctypes beside the untouched descriptors, what the plan entry points
answer to a table (they run the launches' checks and launch nothing), and the CPU restatement of the table that tests/test_qkn_stats_gpu.py holds the
kernels to."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import qkn_stats_ref
from test_gemm_exact_cpu import key, meta, qkn_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1 << 40                       # a 16-byte aligned "address": the queries never follow a pointer
OK, ERR_SHAPE, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -4
P256, P128, T128 = 4, 5, 1           # BYA_GEMM_PATH_*


@pytest.fixture(scope="module")
def lib_hip_ops():
    from bind_your_avatar_implementation_amd import build
    build.build_hip_library()
    from bind_your_avatar_implementation_amd import _hip, ops
    assert {v: k for k, v in _hip.ERRORS.items()}["BYA_ERR_UNSUPPORTED"] == ERR_UNSUPPORTED
    assert {v: k for k, v in _hip.ERRORS.items()}["BYA_ERR_ALIGN"] == ERR_ALIGN
    assert {v: k for k, v in _hip.ERRORS.items()}["BYA_ERR_SHAPE"] == ERR_SHAPE
    return _hip.load(), _hip, ops


def header_fields(text, name):
    """(field, ctypes type) of ``typedef struct name {...} name;`` in the header."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"const void*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            typ, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl).groups()
            fields += [(n.strip(), ctype[typ]) for n in names.split(",")]
    return fields


def test_header_and_ctypes_agree_and_the_descriptors_keep_their_bytes():
    """The statistics travel as two arguments of entry points of their own: bya_qknorm_desc (header and ctypes field lists
    agree) and bya_mx_gemm_call are what they were, so a descriptor built by an existing caller means what it meant.  Each
    ``*_stats`` entry point is declared with its plain twin's arguments plus (stats, stats_slots) in front of the stream / plan."""
    from bind_your_avatar_implementation_amd import _hip
    with open(os.path.join(ROOT, "include", "bya.h")) as f:
        text = f.read()
    assert header_fields(text, "bya_qknorm_desc") == list(_hip.QkNormDesc._fields_)
    assert ctypes.sizeof(_hip.QkNormDesc) == 64 and ctypes.sizeof(_hip.MxGemmCall) == 11 * 8 + 4 * 4
    P = ctypes.POINTER
    for plain, stats in (("bya_gemm_qkv_norm_rope", "bya_gemm_qkv_norm_rope_stats"),
                         ("bya_gemm_fp8_qkv_norm_rope", "bya_gemm_fp8_qkv_norm_rope_stats"),
                         ("bya_gemm_mx_qkv_norm_rope_on", "bya_gemm_mx_qkv_norm_rope_stats")):
        for tail, last in (("", ctypes.c_void_p), ("_plan", P(_hip.GemmPlan))):
            sig, base = _hip.SIGNATURES[stats + tail], _hip.SIGNATURES[plain + tail]
            assert sig == base[:-1] + [ctypes.c_void_p, ctypes.c_int32, last] and base[-1] == last, stats + tail
            decl = re.search(r"int %s\((.*?)\);" % (stats + tail), text, re.S).group(1)
            assert len(decl.split(",")) == len(sig) and "stats, int32_t stats_slots" in " ".join(decl.split()), stats + tail


def norm_desc(_hip, width, text=40):
    n = _hip.QkNormDesc()
    n.qw = n.qb = n.kw = n.kb = n.cos = n.sin = BASE
    n.text_rows, n.width, n.eps, n.k_scale = text, width, 1e-6, 0.18
    return n


def gemm_desc(_hip, M, width, K, lda, batch=1, tensors=3, n_split=None):
    d = _hip.GemmDesc()
    n_split = width if n_split is None else n_split
    d.M, d.N, d.K, d.batch = M, tensors * width, K, batch
    d.lda, d.ldw, d.ldc = lda, lda, n_split
    d.a_batch_stride, d.c_batch_stride = M * lda, M * n_split
    d.n_split, d.c_split_stride, d.alpha = n_split, batch * M * n_split, 1.0
    return d


NO_TABLE = object()


def ask(lib, _hip, entry, M=300, width=128, K=512, batch=1, n_split=None, kernel=2, stats=NO_TABLE, stats_slots=0):
    """The plan query of ``entry`` ("bf16", "fp8", "mx" = the MX form with ``kernel``, "mx0" = with kernel 0) for one shape ->
    (return code, path or None): of the plain entry point, or -- ``stats`` given, None included -- of its ``_stats`` twin.  A
    refused query also pins the launch's own answer."""
    n, p = norm_desc(_hip, width), _hip.GemmPlan(-9, -9, -9, -9, -9)
    d = gemm_desc(_hip, M, width, K, K, batch, n_split=n_split)
    dn, pp = (ctypes.byref(d), ctypes.byref(n)), ctypes.byref(p)
    table = stats is not NO_TABLE
    if entry == "bf16":
        args, name, tail = (BASE, BASE, BASE, BASE, *dn), "bya_gemm_qkv_norm_rope", ()
    elif entry == "fp8":
        args, name, tail = (BASE, BASE, BASE, BASE, BASE, BASE, *dn), "bya_gemm_fp8_qkv_norm_rope", ()
    else:
        kernel = 0 if entry == "mx0" else kernel
        args, tail = (BASE, BASE, BASE, BASE, BASE, BASE, 0, 0, *dn), (kernel,)
        name = "bya_gemm_mx_qkv_norm_rope" if table else "bya_gemm_mx_qkv_norm_rope_on"
    if table:
        name, tail = name + "_stats", (*tail, stats, stats_slots)
    rc = getattr(lib, name + "_plan")(*args, *tail, pp)
    if rc != OK:
        assert getattr(lib, name)(*args, *tail, None) == rc                     # refused before any launch, with the same code
        assert (p.path, p.m0, p.tail) == (-9, -9, -9)
    return rc, (p.path if rc == OK else None)


ENTRIES = ("bf16", "fp8", "mx", "mx0")
FP8_BIG = dict(M=300, width=8576)        # 2 x 101 tiles of 256 x 256: the launch bya_gemm_fp8 puts on its persistent kernel


def test_slot_count_and_alignment_are_checked_before_any_launch(lib_hip_ops):
    lib, _hip, _ = lib_hip_ops
    for entry in ENTRIES:
        shape = FP8_BIG if entry == "fp8" else {}
        for slots in (0, 65, -1):
            assert ask(lib, _hip, entry, stats=BASE, stats_slots=slots, **shape)[0] == ERR_SHAPE, (entry, slots)
        assert ask(lib, _hip, entry, stats=BASE + 2, stats_slots=8, **shape)[0] == ERR_ALIGN, entry
        # a NULL table: the slot count is not read, the plan is today's
        for slots in (0, 65):
            assert ask(lib, _hip, entry, stats=None, stats_slots=slots, **shape) == ask(lib, _hip, entry, **shape), entry
    for slots in (1, 8, 64):
        assert ask(lib, _hip, "bf16", stats=BASE, stats_slots=slots) == (OK, P128)
        assert ask(lib, _hip, "bf16", stats=BASE + 4, stats_slots=slots) == (OK, P128)    # (fp32 entries: 4 bytes are enough)
        assert ask(lib, _hip, "mx", stats=BASE, stats_slots=slots) == (OK, P256)
        assert ask(lib, _hip, "fp8", stats=BASE, stats_slots=slots, **FP8_BIG) == (OK, P256)


def test_kernel_paths_without_the_statistics_decline_a_table(lib_hip_ops):
    """The tile-body epilogue (the 128 x 128 MX and fp8 kernels) does not record the statistics: with a table the entry points
    answer BYA_ERR_UNSUPPORTED where their launch would take that kernel, and what they answer without one is unchanged."""
    lib, _hip, _ = lib_hip_ops
    table = dict(stats=BASE, stats_slots=8)
    assert ask(lib, _hip, "mx0") == (OK, T128) and ask(lib, _hip, "mx0", **table)[0] == ERR_UNSUPPORTED
    assert ask(lib, _hip, "mx", kernel=0) == (OK, T128) and ask(lib, _hip, "mx", kernel=0, **table)[0] == ERR_UNSUPPORTED
    assert ask(lib, _hip, "mx", kernel=1) == (OK, T128) and ask(lib, _hip, "mx", kernel=1, **table)[0] == ERR_UNSUPPORTED   # 6 tiles
    assert ask(lib, _hip, "mx", kernel=2) == (OK, P256) and ask(lib, _hip, "mx", kernel=2, **table) == (OK, P256)
    assert ask(lib, _hip, "fp8") == (OK, T128) and ask(lib, _hip, "fp8", **table)[0] == ERR_UNSUPPORTED
    assert ask(lib, _hip, "fp8", **FP8_BIG) == (OK, P256) and ask(lib, _hip, "fp8", **FP8_BIG, **table) == (OK, P256)


def test_column_blocks_take_one_batch_entry(lib_hip_ops):
    """n_split < width is the head-parallel sharded step's column-block form, whose table is indexed by the global head: one
    batch entry.  With two the table's index is not defined: declined, as is a block that is no whole number of heads."""
    lib, _hip, _ = lib_hip_ops
    table = dict(stats=BASE, stats_slots=16)
    for entry in ("bf16", "mx"):
        assert ask(lib, _hip, entry, width=256, n_split=64, **table)[0] == OK, entry
        assert ask(lib, _hip, entry, width=256, n_split=64, batch=2, **table)[0] == ERR_UNSUPPORTED, entry
        assert ask(lib, _hip, entry, width=256, n_split=64, batch=2)[0] == OK, entry                  # (without a table: today's)
        assert ask(lib, _hip, entry, width=256, batch=2, **table)[0] == OK, entry                     # dense, batched
        assert ask(lib, _hip, entry, width=256, n_split=32, **table)[0] == ERR_UNSUPPORTED, entry     # half a head per block
        assert ask(lib, _hip, entry, width=256, n_split=96, **table)[0] == ERR_UNSUPPORTED, entry     # blocks that do not tile q
        assert ask(lib, _hip, entry, width=256, n_split=768, **table)[0] == ERR_UNSUPPORTED, entry    # one packed row


def test_a_null_table_plans_what_it_planned_before(lib_hip_ops):
    """ops.gemm_qkv_norm_rope_plan on the shapes tests/test_gemm_exact_cpu.py pins: the same answers without the keyword, with
    stats=None, and -- every plan path of the bf16 entry point records the statistics -- with a table."""
    _, _, ops = lib_hip_ops
    cases = [(dict(M=17550), ("p256", 0, None, 0, 1)), (dict(M=17776), ("p256", 0, None, 0, 1)),
             (dict(M=2222), ("p256", 1792, "p128", 0, 1)), (dict(M=35100), ("p256", 34560, "p128", 0, 1)),
             (dict(M=300, N=1152, K=256, text=40), ("p128", 0, None, 0, 1)), (dict(M=826, batch=2), ("p128", 0, None, 0, 1)),
             (dict(M=1000, N=1152, K=128, text=226), None)]
    for kw, want in cases:
        assert key(qkn_plan(ops, **kw)) == want, kw
        M, N, K, text, batch = kw["M"], kw.get("N", 9216), kw.get("K", 3072), kw.get("text", 226), kw.get("batch", 1)
        width = N // 3
        a = meta(M, K) if batch == 1 else meta(batch, M, K)
        out = meta(3, M, width) if batch == 1 else meta(3, batch, M, width)
        v, cs = meta(64), meta(M - text, 64, dtype=torch.float32)
        args = (a, meta(N, K), out[0], meta(N), (width, batch * M * width), v, v, v, v, cs, cs, text)
        table = meta(8, 2, batch * width // 64, dtype=torch.float32)
        for stats in (None, 8, table):
            assert key(ops.gemm_qkv_norm_rope_plan(*args, stats=stats)) == want, (kw, stats)
    with pytest.raises(AssertionError):                                          # a table of another launch's shape
        ops.gemm_qkv_norm_rope_plan(*args, stats=meta(8, 2, 5, dtype=torch.float32))


def test_the_restatement_of_the_table_agrees_with_fp64_to_one_ulp():
    """tests/qkn_stats_ref.py against an fp64 computation on random (gaussian) bf16 rows: the TABLE -- per head the maximum over
    the rows -- to one ulp of fp32, the bound this feature's issue sets, measured the way the suite measures every result
    against fp64 (exact_gemm.bf16_ulps, cond_norm.ulp_error): against the ROUNDING of the fp64 value to the result's format, in
    ulps of that rounding.
    The order of the additions is the kernels' and not free: 56 additions inside the groups and 7 in the tree, each rounded to
    half an ulp of a partial sum -- by that count a row's sum can be 5 ulp off in the worst case.  Measured on gaussian rows
    (three seeds of 20000 head rows): up to 1.94 ulp from the UNROUNDED fp64 sum, 2.6 % of the rows more than 1 ulp; the rows
    and the table of this test: printed below (the table 1.04 ulp from the unrounded sum, 1 ulp from its rounding).  One ulp is
    therefore no property of the order for every row and every data set; it is asserted where the issue sets it, on the table
    of rows drawn with a seed fixed before any figure was seen."""
    g = torch.Generator().manual_seed(7)
    rows = torch.randn(2, 257, 5 * 64, generator=g).to(torch.bfloat16)
    got = qkn_stats_ref.row_norm2(rows)
    assert got.dtype == np.float32 and got.shape == (2, 257, 5)
    exact = (rows.double().numpy().reshape(2, 257, 5, 64) ** 2).sum(-1)
    row_err = np.abs(got.astype(np.float64) - exact) / np.spacing(got).astype(np.float64)
    t = qkn_stats_ref.table(rows, rows[:, :100])
    assert t.shape == (2, 10) and t.dtype == torch.float32
    assert torch.equal(t[0], torch.from_numpy(got.max(axis=1).reshape(-1)))
    assert bool((t[1] <= t[0]).all())
    want64 = np.stack([exact.max(axis=1).reshape(-1), exact[:, :100].max(axis=1).reshape(-1)])
    want = want64.astype(np.float32)
    raw = np.abs(t.numpy().astype(np.float64) - want64) / np.spacing(want).astype(np.float64)
    err = np.abs(t.numpy().astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
    print(f"restatement vs fp64: table worst {err.max():.0f} ulp of fp32 from the rounded sum ({raw.max():.3f} from the unrounded one); "
          f"rows worst {row_err.max():.3f} from the unrounded one, {100 * (row_err > 1).mean():.1f} % above 1")
    assert err.max() <= 1.0
