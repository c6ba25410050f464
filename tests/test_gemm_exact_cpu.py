"""CPU: which kernels the GEMM entry points plan for the shapes the docs and tests name (the plan queries of include/bya.h,
which launch nothing), and why the exact-data comparator of tests/exact_gemm.py replaces a global error bar for tiled kernels.
Meta tensors stand for device tensors: the queries see their shapes, strides and (view-offset) alignment."""
import math

import pytest
import torch

from conftest import rel_fro
from exact_gemm import BF, POISON, assert_exact, bad_elements, describe, reference

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from bind_your_avatar_implementation_amd import build
    build.build_hip_library()
    from bind_your_avatar_implementation_amd import ops
    return ops


def meta(*shape, dtype=BF16):
    return torch.empty(*shape, dtype=dtype, device="meta")


def bf16_plan(ops, M, N, K, batch=1, **kw):
    a = meta(M, K) if batch == 1 else meta(batch, M, K)
    out = meta(M, N) if batch == 1 else meta(batch, M, N)
    return ops.gemm_plan(a, meta(N, K), out, **kw)


def qkn_plan(ops, M, N=9216, K=3072, text=226, batch=1):
    width = N // 3
    a = meta(M, K) if batch == 1 else meta(batch, M, K)
    out = meta(3, M, width) if batch == 1 else meta(3, batch, M, width)
    v, cs = meta(64), meta(M - text, 64, dtype=torch.float32)
    return ops.gemm_qkv_norm_rope_plan(a, meta(N, K), out[0], meta(N), (width, batch * M * width), v, v, v, v, cs, cs, text)


def fp8_plan(ops, M, N, K, batch=1):
    a = meta(M, K, dtype=torch.uint8) if batch == 1 else meta(batch, M, K, dtype=torch.uint8)
    out = meta(M, N) if batch == 1 else meta(batch, M, N)
    return ops.gemm_fp8_plan(a, meta(batch * M, dtype=torch.float32), meta(N, K, dtype=torch.uint8),
                             meta(N, dtype=torch.float32), out)


def mx_plan(ops, M, N, K, fmt, batch=1):
    rb = ops.mx_code_bytes(K, fmt)
    sc = meta(M, K // 32, dtype=torch.uint8) if batch == 1 else meta(batch, M, K // 32, dtype=torch.uint8)
    out = meta(M, N) if batch == 1 else meta(batch, M, N)
    return ops.gemm_mx_plan(meta(batch * M * rb, dtype=torch.uint8), sc, meta(N, rb, dtype=torch.uint8),
                            meta(N, K // 32, dtype=torch.uint8), out, fmt)


def key(p):
    return None if p is None else (p["path"], p["m0"], p["tail"], p["split_k"], p["row_chunks"])


# (M, N, K) -> (path, m0, tail, split_k, row_chunks) under the default options and no split-K workspace
BF16_PLANS = [
    ((17776, 3072, 3072), ("p256", 16384, "p128s", 0, 1)),   # attn1.to_out: 3 full rounds of 256-row tiles + 1392 rows on 128 x 256
    ((17776, 3072, 12288), ("p256", 16384, "p128s", 0, 1)),  # FF2: the same row plan
    ((17550, 3072, 3072), ("p256", 16384, "p128s", 0, 1)),   # audio out-projection
    ((17776, 12288, 3072), ("p256", 17664, "p128s", 0, 1)),  # FF1
    ((17776, 9216, 3072), ("p256", 0, None, 0, 1)),          # q|k|v: 2520 tiles, the last round 84 % full
    ((2222, 3072, 3072), ("p128s", 0, None, 0, 1)),          # one rank's rows of an 8-GPU step
    ((2222, 9216, 3072), ("p256", 1792, "p128s", 0, 1)),     # ... its q|k|v: one full round + 430 rows on 128 x 256
    ((2221, 3072, 12288), ("p128s", 0, None, 0, 1)),         # one rank's FF2 (odd rows)
    ((520, 87552, 512), ("p128s", 0, None, 0, 1)),           # few rows, short K, a deep grid: the persistent 128 x 256 kernel
    ((832, 258048, 768), ("p256", 768, "p128s", 0, 1)),      # the audio K/V projection of all layers in one launch
    ((300, 64, 512), ("t128x64", 0, None, 0, 1)),            # N <= 64
    ((4000, 64, 3072), ("t128x64", 0, None, 0, 1)),
    ((2222, 3072, 64), ("t128x128", 0, None, 0, 1)),         # K of 1, 2, 3 K-tiles: short K stays on the 128 x 128 kernel
    ((2222, 3072, 128), ("t128x128", 0, None, 0, 1)),
    ((2222, 3072, 192), ("t128x128", 0, None, 0, 1)),
    ((1024, 1024, 64), ("t128x128", 0, None, 0, 1)),         # test_gemm_pipelined_256's shapes: none reaches a 256-row tile
    ((2500, 3072, 192), ("t128x128", 0, None, 0, 1)),
    ((4100, 768, 3072), ("p128s", 0, None, 0, 1)),
    ((17776, 512, 512), ("t128x128", 0, None, 0, 1)),
    ((90226, 12288, 256), ("t128x128", 0, None, 0, 2)),      # 97 frames at 720p: the 2.2 GB activation is cut into 2 row chunks
]


@pytest.mark.parametrize("shape,want", BF16_PLANS, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
def test_bf16_plan_of_the_named_shapes(ops, shape, want):
    assert key(bf16_plan(ops, *shape)) == want


def test_bf16_plan_fallbacks_options_and_forced_tiles(ops):
    # a C view 8- but not 16-byte aligned (4 columns into a strided buffer): the 8-wave 256 x 256 kernel, no 128-row tile
    buf = meta(17776, 3072 + 8)
    p = ops.gemm_plan(meta(17776, 3072), meta(3072, 3072), buf[:, 4:4 + 3072])
    assert key(p) == ("w8_256", 0, None, 0, 1)
    # ... the same view 16-byte aligned keeps the row plan
    assert key(ops.gemm_plan(meta(17776, 3072), meta(3072, 3072), buf[:, 8:8 + 3072]))[:3] == ("p256", 16384, "p128s")
    with ops.options(gemm_variant=1):
        assert bf16_plan(ops, 17776, 3072, 3072)["path"] == "w8_256"
    with ops.options(gemm_variant=2):              # 256 x 256 only: no 128-row tile, whole or tail
        assert key(bf16_plan(ops, 17776, 3072, 3072)) == ("p256", 0, None, 0, 1)
    # split-K needs the current device's workspace: none without a GPU, whatever the option says (on the 256-row kernel, the
    # only one that splits: the GPU matrix's split-K case, where it does)
    with ops.options(gemm_splitk=1, gemm_splitk_min=8, gemm_tile=4):
        assert key(bf16_plan(ops, 4000, 1536, 1024)) == ("p256", 0, None, 0, 1)
    # forced tiles; the persistent ones fall back where they are not eligible (K < 3 / 4 K-tiles, an activation they lack)
    for tile, want in enumerate(["t128x64", "t128x128", "t256x128", "t256x256", "p256", "p128", "p128s"]):
        with ops.options(gemm_tile=tile):
            assert bf16_plan(ops, 515, 264, 256)["path"] == want, tile
            if tile >= 4:
                assert bf16_plan(ops, 515, 264, 128)["path"] == "w8_256", tile
                assert bf16_plan(ops, 515, 264, 256, act="silu")["path"] == "t128x128", tile
    with ops.options(gemm_tile=4):
        assert bf16_plan(ops, 515, 260, 256)["path"] == "w8_256"          # N % 8 != 0


def test_skinny_plan_is_the_callers_choice(ops):
    with ops.weight_streaming():
        assert bf16_plan(ops, 37, 3072, 2048)["path"] == "skinny"
        assert bf16_plan(ops, 65, 3072, 2048)["path"] == "t128x128"
    assert bf16_plan(ops, 37, 3072, 2048)["path"] == "t128x128"


def test_qkv_norm_rope_plans(ops):
    # 17550 / 17776 rows (the single-GPU step): plan 0, all 256-row tiles
    assert key(qkn_plan(ops, 17550)) == ("p256", 0, None, 0, 1)
    assert key(qkn_plan(ops, 17776)) == ("p256", 0, None, 0, 1)
    # one rank's 2222 rows: plan 2 (rows split at 1792; test_kernels_gpu.py's docstring says 128 x 256 for the whole launch)
    assert key(qkn_plan(ops, 2222)) == ("p256", 1792, "p128", 0, 1)
    assert key(qkn_plan(ops, 35100)) == ("p256", 34560, "p128", 0, 1)
    # plan 1: few rows
    assert key(qkn_plan(ops, 300, N=1152, K=256, text=40)) == ("p128", 0, None, 0, 1)
    assert key(qkn_plan(ops, 826, batch=2)) == ("p128", 0, None, 0, 1)
    # forced tiles 5 / 6 -> 128-row tiles, anything else -> 256-row tiles
    with ops.options(gemm_tile=5):
        assert qkn_plan(ops, 17776)["path"] == "p128"
    with ops.options(gemm_tile=4):
        assert key(qkn_plan(ops, 2222)) == ("p256", 0, None, 0, 1)
    # declined shapes: two launches instead
    assert qkn_plan(ops, 1000, N=1152, K=128, text=226) is None


def test_fp8_and_mx_plans_of_the_dit_linears(ops):
    for M, N, K in [(17776, 9216, 3072), (17776, 3072, 3072), (17776, 12288, 3072), (2222, 9216, 3072)]:
        assert fp8_plan(ops, M, N, K)["path"] == "p256"
        assert mx_plan(ops, M, N, K, "mxfp6")["path"] == "t256x256"
        assert mx_plan(ops, M, N, K, "mxfp8")["path"] == "t128x128"
    # one rank's FF2, 2221 rows: 108 tiles of 256 x 256, below the 200 the big tiles ask for
    assert fp8_plan(ops, 2221, 3072, 12288)["path"] == "t128x128"
    assert mx_plan(ops, 2221, 3072, 12288, "mxfp6")["path"] == "t128x128"
    # the ragged, batched e2m3 shape of the exact GPU matrix
    assert mx_plan(ops, 3621, 3844, 256, "mxfp6", batch=2)["path"] == "t256x256"
    with ops.options(fp8_kernel=1):
        assert fp8_plan(ops, 17776, 3072, 3072)["path"] == "t128x128"


def test_gemm_path_names_match_the_header():
    import os
    import re
    from bind_your_avatar_implementation_amd import _hip
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bya.h")).read()
    codes = {int(v): n for n, v in re.findall(r"#define BYA_GEMM_PATH_(\w+) (\d+)", src) if n != "COUNT"}
    count = int(re.search(r"#define BYA_GEMM_PATH_COUNT (\d+)", src).group(1))
    assert sorted(codes) == list(range(count)) == sorted(_hip.GEMM_PATHS)
    for c, n in codes.items():
        assert _hip.GEMM_PATHS[c] == n.lower(), (c, n)


# ---------------------------------------------------------------------------------------------------------------------------
def test_exact_comparator_names_the_planted_faults_a_global_bar_passes_them():
    """Why the exact comparator: an exact product at reduced size with two planted faults -- one 16 x 16 fragment that lost
    one of its 48 K-tiles, one 16 x 16 fragment never written (stale values) -- is flagged fragment by fragment, while the
    first fault, at the proportions of 17776 x 3072 x 3072 (the same per-element RMS over 17776 x 3072 outputs), scores far
    below the rel-Fro bar of 1e-3."""
    from exact_gemm import exact_operands
    M, N, K = 256, 192, 48 * 64
    a, w = exact_operands(M, N, K, "cpu", seed=5)
    ref = reference(a, w)
    got = ref.to(BF).clone()
    # fault 1: fragment (rows 32..47, cols 80..95) without K-tile 7
    r, c, kt = slice(32, 48), slice(80, 96), slice(7 * 64, 8 * 64)
    lost = reference(a[r, kt], w[c, kt])
    got[r, c] = (ref[r, c] - lost).to(BF)
    # fault 2: fragment (rows 160..175, cols 16..31) never written: what the buffer held before (a stale earlier result)
    got[160:176, 16:32] = (ref[160:176, 16:32] * 0.5 + 1).to(BF)
    bad = bad_elements(got, ref.to(BF))
    assert bool(bad[32:48, 80:96].any()) and bool(bad[160:176, 16:32].all())
    assert int(bad.sum()) == int(bad[32:48, 80:96].sum()) + 256
    msg = describe(bad[:, :64], got[:, :64], ref.to(BF)[:, :64])
    assert "16: rows 10..10 cols 1..1" in msg, msg                    # the stale fragment, named in 16-element units
    msg = describe(bad[:, 64:], got[:, 64:], ref.to(BF)[:, 64:])
    assert "16: rows 2..2 cols 1..1" in msg, msg                      # the short fragment (columns counted from 64)
    with pytest.raises(AssertionError, match="elements differ"):
        assert_exact(got, ref, plan="planted")
    # NaN poison: an element no kernel wrote fails, whatever the reference
    poisoned = ref.to(BF).clone()
    poisoned.view(torch.int16)[3, 4] = POISON
    assert int(bad_elements(poisoned, ref.to(BF)).sum()) == 1
    # the usual bar against fault 1 alone, scaled to a 17776 x 3072 output of the same per-element RMS
    one = ref.to(BF).clone()
    one[r, c] = got[r, c]
    delta = (one.double() - ref.to(BF).double()).norm()
    rms = ref.to(BF).double().norm() / math.sqrt(M * N)
    full = float(delta / (rms * math.sqrt(17776 * 3072)))
    print(f"one fragment short of one of 48 K-tiles at 17776 x 3072: rel-Fro {full:.2e}")
    assert full <= 1e-3                     # passes the global bar ...
    assert rel_fro(one.float(), ref.to(BF).float()) > 0     # ... though the result is wrong


def test_the_exact_gpu_matrix_reaches_the_paths_it_names(ops):
    """The cases of test_gemm_exact_gpu.py, planned here on meta tensors of the same shapes, strides and view offsets (built by
    the same GuardedOut); the split-K ones need a device's workspace and are checked on the GPU only."""
    import test_gemm_exact_gpu as g
    for cid, M, N, K, opts, expect, kw in g.BF16_CASES:
        if "splitk" in expect:
            continue
        args = g.meta_case(M, N, K, **kw)
        with ops.options(**opts):
            assert ops.plan_key(ops.gemm_plan(args.pop("a"), args.pop("w"), args.pop("out"), **args)) == expect, cid
    for B, M in g.SKINNY_CASES:
        args = g.meta_case(M, 272, 512, batch=B, bias=True, res="separate", alpha=2.0)
        with ops.weight_streaming():
            assert ops.gemm_plan(args.pop("a"), args.pop("w"), args.pop("out"), **args)["path"] == "skinny"
    for B, M, N, K, opts, expect in g.FP8_CASES:
        with ops.options(**opts):
            assert fp8_plan(ops, M, N, K, batch=B)["path"] == expect, (B, M, N, K)
    for fmt, B, M, N, K, expect in g.MX_CASES:
        assert mx_plan(ops, M, N, K, fmt, batch=B)["path"] == expect, (fmt, B, M, N, K)
    for B, M, N, K, text, opts, expect in g.QKN_CASES:
        with ops.options(**opts):
            assert ops.plan_key(qkn_plan(ops, M, N=N, K=K, text=text, batch=B)) == expect, (B, M, N, K, text)


def test_the_exact_gpu_matrix_covers_every_planned_kernel(ops):
    """Every kernel a planner can return has a case in test_gemm_exact_gpu.py (each case asserts that it reaches the kernel
    it names, so the names below are what the matrix runs): a path added later without an exact case fails here."""
    import test_gemm_exact_gpu as g
    bf16 = {c[5] for c in g.BF16_CASES}
    kernels = {k.split("+")[0] for name in bf16 for k in name.split("|")}
    assert kernels == set(ops.GEMM_PATHS.values()), sorted(kernels ^ set(ops.GEMM_PATHS.values()))
    assert {"p256|p128s", "p256|t128x128", "p256+splitk"} <= bf16, sorted(bf16)        # both row-split tails, split-K
    assert g.SKINNY_CASES
    assert {c[-1] for c in g.QKN_CASES} == {"p256", "p128", "p256|p128"}              # row plans 0, 1, 2
    assert {c[-1] for c in g.FP8_CASES} == {"t128x128", "p256"}
    # ... and the e4m3 GEMM's own matrix (test_fp8_exact_gpu.py) holds, for EACH of its two kernels, every epilogue kind, batch
    # 2, a launch cut into row chunks, and an odd and an even K-tile count: a case dropped later fails here
    import test_fp8_exact_gpu as f8
    for path in ("t128x128", "p256"):
        cases = [c for c in f8.FP8_EXACT_CASES if c[6] == path and (path == "p256" or c[0].startswith("t-"))]
        kinds = set().union(*(f8.epilogue_kinds(c[2], c[7]) for c in cases))
        assert kinds >= f8.REQUIRED_KINDS, (path, sorted(f8.REQUIRED_KINDS - kinds))
        assert any(c[1] == 2 for c in cases), path
        assert {(c[4] // 128) % 2 for c in cases} == {0, 1}, path
        assert any(c[5] == path and c[6] > 1 for c in f8.CHUNK_CASES), path
    assert {c[4] for c in f8.FP8_EXACT_CASES if c[6] == "t128x128"} >= {128, 256, 384, 12288}
    assert {c[4] for c in f8.FP8_EXACT_CASES if c[6] == "p256"} >= {512, 640, 768, 1152}
    assert {(c[0], c[-1]) for c in g.MX_CASES} == {("mxfp8", "t128x128"), ("mxfp6", "t128x128"), ("mxfp6", "t256x256")}


def test_launches_refuse_meta_tensors_before_the_library(ops):
    """Only the plan queries take meta tensors: a launch with them is a ValueError, never a kernel on a made-up address."""
    a, w, out = meta(300, 512), meta(256, 512), meta(300, 256)
    with pytest.raises(ValueError, match="device tensor"):
        ops.gemm(a, w, out)
    with pytest.raises(ValueError):
        ops.gemm_fp8(meta(300, 512, dtype=torch.uint8), meta(300, dtype=torch.float32), meta(256, 512, dtype=torch.uint8),
                     meta(256, dtype=torch.float32), out)
    rb = ops.mx_code_bytes(512, "mxfp6")
    with pytest.raises(ValueError):
        ops.gemm_mx(meta(300 * rb, dtype=torch.uint8), meta(300, 16, dtype=torch.uint8), meta(256, rb, dtype=torch.uint8),
                    meta(256, 16, dtype=torch.uint8), out, "mxfp6")
    v, cs = meta(64), meta(300 - 40, 64, dtype=torch.float32)
    with pytest.raises(ValueError):
        ops.gemm_qkv_norm_rope(meta(300, 256), meta(1152, 256), meta(3, 300, 384)[0], meta(1152), (384, 300 * 384),
                               v, v, v, v, cs, cs, 40)
    with pytest.raises(ValueError):                     # the strict address helper itself
        ops._p(a)
    assert ops.gemm_plan(a, w, out)["path"]             # ... while the query takes them
