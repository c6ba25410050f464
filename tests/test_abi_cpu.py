"""CPU: the C-ABI library builds for gfx950, loads, and exports exactly what include/bya.h declares
(no compute is launched: there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from bind_your_avatar_implementation_amd.build import build_hip_library
    return build_hip_library()


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "bya.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(bya_\w+)\s*\(", src)))


def test_header_declares_the_documented_entry_points():
    syms = declared_symbols()
    for must in ["bya_gemm_bf16", "bya_gemm_bf16_plan", "bya_gemm_qkv_norm_rope_plan", "bya_gemm_fp8_plan", "bya_gemm_mx_plan",
                 "bya_gemm_skinny_bf16", "bya_attn_fwd", "bya_attn_plan", "bya_attn_kv_mix_plan", "bya_attn_tiny_plan", "bya_rowgemm512_plan",
                 "bya_router_mlp_fused_plan", "bya_router_group_attn_plan", "bya_router_group_attn_out_plan", "bya_layernorm", "bya_layernorm_plan", "bya_qknorm_rope", "bya_qknorm_rope_plan", "bya_masked_combine",
                 "bya_router_scores", "bya_router_head", "bya_forcing_max_over_frames", "bya_patchify",
                 "bya_unpatchify", "bya_linear_small_m", "bya_timestep_features", "bya_attn_tiny", "bya_act_add",
                 "bya_router_scores_plan", "bya_linear_small_m_plan", "bya_act_add_plan", "bya_cfg_scheduler_step", "bya_cfg_scheduler_step_plan",
                 "bya_abi_version"]:
        assert must in syms


def test_library_exports_every_declared_symbol(lib_path):
    lib = ctypes.CDLL(lib_path)
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} declared in include/bya.h but not exported"
    assert lib.bya_abi_version() >= 1


def test_python_binding_table_matches_header(lib_path):
    from bind_your_avatar_implementation_amd import _hip
    assert sorted(_hip.SIGNATURES) == declared_symbols()
    lib = _hip.load()
    # argument validation happens before any launch: NULL pointers / bad shapes are rejected on a CPU-only box too
    d = _hip.GemmDesc()
    assert lib.bya_gemm_bf16(None, None, None, None, None, None, None, ctypes.byref(d), None) == -1
    a = _hip.AttnDesc()
    assert lib.bya_attn_fwd(None, None, None, None, ctypes.byref(a), None) == -1
    # the GEMM plan queries validate like their entry points and fill the plan (host-side, launch nothing)
    p = _hip.GemmPlan(-9, -9, -9, -9, -9)
    assert lib.bya_gemm_bf16_plan(None, None, None, None, None, None, None, ctypes.byref(d), ctypes.byref(p)) == -1
    assert lib.bya_gemm_fp8_plan(None, None, None, None, None, None, None, None, None, ctypes.byref(d), ctypes.byref(p)) == -1
    assert lib.bya_gemm_mx_plan(None, None, None, None, None, None, None, None, None, ctypes.byref(d), 2, ctypes.byref(p)) == -1
    n = _hip.QkNormDesc()
    assert lib.bya_gemm_qkv_norm_rope_plan(None, None, None, None, ctypes.byref(d), ctypes.byref(n), ctypes.byref(p)) == -1
    assert (p.path, p.m0) == (-9, -9)                                       # untouched on rejection
    d.M, d.N, d.K, d.batch, d.lda, d.ldw, d.ldc = 300, 64, 512, 1, 512, 512, 64
    base = 1 << 40
    assert lib.bya_gemm_bf16_plan(base, base, None, base, None, None, None, ctypes.byref(d), ctypes.byref(p)) == 0
    assert (p.path, p.m0, p.tail, p.split_k, p.row_chunks) == (0, 0, -1, 0, 1)    # N <= 64: 128 x 64 tiles
    assert lib.bya_gemm_bf16_plan(base, base, None, base + 2, None, None, None, ctypes.byref(d), ctypes.byref(p)) == -2
    assert lib.bya_gemm_bf16_plan(base, base, None, base, None, None, None, ctypes.byref(d), None) == -1
    # the softmax-variant query mirrors bya_attn_fwd's kernel choice (host-side, launches nothing)
    a.head_dim, a.scores_prescaled, a.score_bound = 64, 1, 11.8
    assert lib.bya_attn_variant(ctypes.byref(a)) == 4          # static bound on the one-wave-per-SIMD kernel
    a.score_bound = 60.0                                        # P = exp2(s) without an offset: usable up to 90
    assert lib.bya_attn_variant(ctypes.byref(a)) == 4
    a.score_bound = 100.0
    assert lib.bya_attn_variant(ctypes.byref(a)) == 1
    dummy = (ctypes.c_float * 4)()
    a.bound_dev, a.fallback_flags = ctypes.addressof(dummy), ctypes.addressof(dummy)      # data-dependent bound: static kernel +
    assert lib.bya_attn_variant(ctypes.byref(a)) == 5                                      # per-head running-maximum fallback
    a.bound_dev, a.fallback_flags = None, None
    a.scores_prescaled = 0
    assert lib.bya_attn_variant(ctypes.byref(a)) == 0
    a.head_dim = 128
    assert lib.bya_attn_variant(ctypes.byref(a)) == 3
    # the attention plan queries validate like their entry points, fill the plan, and leave it alone on rejection
    ap = _hip.AttnPlan(-9, -9)
    a = _hip.AttnDesc()
    assert lib.bya_attn_plan(None, base, 0, ctypes.byref(ap)) == -1 and lib.bya_attn_plan(ctypes.byref(a), base, 0, None) == -1
    a.head_dim, a.heads, a.nb1, a.nb2, a.Sq, a.Skv = 64, 48, 1, 1, 17776, 17776
    a.q_row = a.k_row = a.v_row = a.o_row = 48 * 64
    a.scores_prescaled, a.score_bound = 1, 11.8
    assert lib.bya_attn_plan(ctypes.byref(a), None, 0, ctypes.byref(ap)) == -1 and ap.variant == -9
    assert lib.bya_attn_plan(ctypes.byref(a), base + 4, 0, ctypes.byref(ap)) == -2 and ap.variant == -9      # o not 8-byte aligned
    assert lib.bya_attn_plan(ctypes.byref(a), base, 1, ctypes.byref(ap)) == 0
    assert (ap.variant, ap.grid, ap.q_tile, ap.stream_k, ap.o_wide, ap.second_launch) == (4, 256, 512, 1, 1, 0)
    assert ap.variant == lib.bya_attn_variant(ctypes.byref(a))
    assert lib.bya_attn_plan(ctypes.byref(a), base + 8, 0, ctypes.byref(ap)) == 0 and (ap.grid, ap.stream_k, ap.o_wide) == (1680, 0, 0)
    a.o_row = 48 * 64 + 2
    assert lib.bya_attn_plan(ctypes.byref(a), base, 0, ctypes.byref(ap)) == -2                                 # o_row % 4
    mp, md = _hip.AttnMixPlan(-9), _hip.AttnMixDesc()
    assert lib.bya_attn_kv_mix_plan(None, None, ctypes.byref(md), ctypes.byref(mp)) == -1
    assert lib.bya_attn_kv_mix_plan(base, None, ctypes.byref(md), None) == -1
    md.head_dim, md.heads, md.n_id, md.n_grp, md.Sq, md.Skv = 64, 48, 2, 13, 1350, 32
    md.q_row = md.k_row = md.v_row = md.z_row = 48 * 64
    assert lib.bya_attn_kv_mix_plan(base + 4, None, ctypes.byref(md), ctypes.byref(mp)) == -2 and mp.form == -9
    assert lib.bya_attn_kv_mix_plan(base, None, ctypes.byref(md), ctypes.byref(mp)) == 0 and (mp.form, mp.head_dim) == (0, 64)
    assert lib.bya_attn_kv_mix_plan(base + 8, None, ctypes.byref(md), ctypes.byref(mp)) == 0 and mp.form == 1
    md.n_id = 1
    assert lib.bya_attn_kv_mix_plan(base, base, ctypes.byref(md), ctypes.byref(mp)) == -1                      # audio needs >= 2 streams
    md.head_dim = 96
    assert lib.bya_attn_kv_mix_plan(base, None, ctypes.byref(md), ctypes.byref(mp)) == -4
    tp = _hip.AttnTinyPlan(-9)
    assert lib.bya_attn_tiny_plan(None, base, base, base, 13, 8, 2, 90, 1536, 512, ctypes.byref(tp)) == -1 and tp.instance == -9
    assert lib.bya_attn_tiny_plan(base, base, base, base, 13, 8, 2, 90, 1536, 512, None) == -1
    assert lib.bya_attn_tiny_plan(base, base, base, base, 33, 8, 2, 90, 1536, 512, ctypes.byref(tp)) == -1
    assert lib.bya_attn_tiny_plan(base, base, base, base, 13, 8, 2, 90, 1536, 512, ctypes.byref(tp)) == 0
    assert (tp.instance, tp.grid, tp.waves) == (2, 45, 180)
    assert lib.bya_attn_tiny_plan(base, base + 8, base, base, 13, 8, 2, 90, 1536, 512, ctypes.byref(tp)) == 0 and tp.instance == 6
    # the router row kernels' plan queries: validate like their entry points, fill the plan, leave it alone on rejection
    rp = _hip.RowGemmPlan(-9)
    assert lib.bya_rowgemm512_plan(None, base, None, base, None, base, 300, 512, 512, 512, 0, 0, 0, ctypes.byref(rp)) == -1 and rp.form == -9
    assert lib.bya_rowgemm512_plan(base, base, None, base, None, base, 300, 512, 512, 512, 0, 0, 0, None) == -1
    assert lib.bya_rowgemm512_plan(base, base, None, base, None, base, 300, 512, 512, 512, 0, 1, 0, ctypes.byref(rp)) == -1   # ln without colsum
    assert lib.bya_rowgemm512_plan(base, base, None, base, None, base + 8, 300, 512, 512, 512, 0, 0, 0, ctypes.byref(rp)) == -2
    assert lib.bya_rowgemm512_plan(base, base, None, base, None, base, 300, 512, 512, 512, 0, 0, 1, ctypes.byref(rp)) == -4   # gelu_tanh
    assert lib.bya_rowgemm512_plan(base, base, None, base, None, base, 300, 512, 512, 512, 0, 0, 0, ctypes.byref(rp)) == 0
    assert (rp.form, rp.ln, rp.res, rp.act, rp.grid, rp.crosses_row_block, rp.work_items) == (0, 0, 0, 0, 16, 0, 16)
    assert lib.bya_rowgemm512_plan(base, base, None, base, base, base, 35100, 512, 768, 512, 512, 0, 2, ctypes.byref(rp)) == 0
    assert (rp.form, rp.ln, rp.res, rp.act, rp.grid, rp.work_items) == (1, 0, 1, 2, 256, 2194)
    assert lib.bya_rowgemm512_plan(base, base, base, base, None, base, 35100, 1536, 512, 1536, 0, 1, 0, ctypes.byref(rp)) == 0
    assert (rp.form, rp.ln, rp.grid, rp.crosses_row_block, rp.work_items) == (0, 1, 256, 1, 138 * 24)
    cp = _hip.RouterChainPlan(-9)
    assert lib.bya_router_mlp_fused_plan(base, base, base, base, base, None, base, 35100, 512, 512, 0, ctypes.byref(cp)) == -1 and cp.tiles == -9
    assert lib.bya_router_mlp_fused_plan(base, base, base, base, base, base, base, 35100, 512, 512, 9, ctypes.byref(cp)) == -1
    assert lib.bya_router_mlp_fused_plan(base, base, base, base, base, base, base, 35100, 520, 512, 0, ctypes.byref(cp)) == 0
    assert (cp.tiles, cp.tp0, cp.grid, cp.passes, cp.tiles_last, cp.wgs_last) == (2194, 8, 256, 2, 1, 146)
    assert lib.bya_router_group_attn_out_plan(base, base, base, base, base, base, base, 35100, 512, 512, 17, 2, 1350, 17550, 1350, 0,
                                              ctypes.byref(cp)) == -4
    assert lib.bya_router_group_attn_out_plan(base, base, base, base, base, base, base, 35100, 512, 512, 13, 2, 1350, 17550, 1350, 0,
                                              ctypes.byref(cp)) == 0
    assert (cp.tiles, cp.tp0, cp.grid, cp.passes, cp.tiles_last, cp.wgs_last) == (2700, 8, 256, 2, 3, 218)
    gp = _hip.GroupAttnPlan(-9)
    assert lib.bya_router_group_attn_plan(base, base, base, base, base, 35100, 512, 512, 33, 2, 1350, 17550, 1350, ctypes.byref(gp)) == -4
    assert gp.P == -9 and lib.bya_router_group_attn_plan(base, base, base, base, base, 35100, 512, 512, 13, 2, 1350, 17550, 1350, None) == -1
    assert lib.bya_router_group_attn_plan(base, base, base, base, base, 35100, 512, 512, 13, 2, 1350, 17550, 1350, ctypes.byref(gp)) == 0
    assert (gp.P, gp.G, gp.wide, gp.blocks, gp.tiles) == (16, 1, 0, 256, 2700)
    assert lib.bya_router_group_attn_plan(base, base, base, base, base, 3333, 512, 512, 3, 1, 1111, 0, 1111, ctypes.byref(gp)) == 0
    assert (gp.P, gp.G, gp.wide, gp.blocks, gp.tiles) == (4, 4, 0, 144, 278)
    assert lib.bya_router_group_attn_plan(base, base, base, base, base, 2250, 512, 512, 25, 2, 45, 1125, 45, ctypes.byref(gp)) == 0
    assert (gp.P, gp.G, gp.wide, gp.tiles) == (16, 1, 1, 180)
    # the norm kernels' plan queries: validate like their entry points, fill the plan, leave it alone on rejection
    lp = _hip.LayerNormPlan(-9)
    ln = lambda x, y, w, b, sh, rows, batch, D, ldy, kind, plan: lib.bya_layernorm_plan(x, y, w, b, sh, sh, sh, sh, rows, batch, D, D, ldy, rows * D,
                                                                                   rows * ldy, 2 * D, 226, kind, plan)
    assert ln(None, base, base, base, None, 4099, 2, 3072, 3072, 0, ctypes.byref(lp)) == -1 and lp.kernel == -9
    assert ln(base, base, base, base, None, 4099, 2, 3072, 3072, 0, None) == -1
    assert ln(base, base, base, base, None, 4099, 2, 3072, 3072, 4, ctypes.byref(lp)) == -1                     # unknown output kind
    assert lib.bya_layernorm_plan(base, base, None, None, base, None, None, None, 4, 1, 512, 512, 512, 0, 0, 0, 0, 0, ctypes.byref(lp)) == -1
    assert ln(base, base + 8, base, base, None, 4099, 2, 3072, 3072, 0, ctypes.byref(lp)) == -2                 # bf16 output: 16 bytes
    assert ln(base, base, None, None, None, 300, 1, 640, 640, 0, ctypes.byref(lp)) == -4 and lp.kernel == -9
    assert ln(base, base, base, base, base, 4099, 2, 3072, 3072, 0, ctypes.byref(lp)) == 0
    assert (lp.kernel, lp.vec, lp.nv, lp.modulated, lp.rows_per_wave, lp.grid, lp.waves) == (1, 8, 6, 1, 3, 684, 2733)
    assert ln(base, base, base, None, None, 4099, 2, 3072, 3072, 0, ctypes.byref(lp)) == 0                      # w without b: generic
    assert (lp.kernel, lp.vec, lp.nv, lp.modulated, lp.rows_per_wave, lp.grid, lp.waves) == (0, 8, 6, 0, 1, 2050, 8198)
    assert ln(base, base, None, None, None, 333, 1, 768, 768, 0, ctypes.byref(lp)) == 0 and (lp.kernel, lp.vec, lp.nv, lp.grid) == (0, 4, 3, 84)
    assert ln(base, base + 8, base, base, base, 333, 2, 3072, 3072, 1, ctypes.byref(lp)) == 0                   # fp8 codes: 8 bytes
    assert (lp.kernel, lp.vec, lp.nv, lp.modulated, lp.rows_per_wave, lp.waves) == (0, 8, 6, 1, 1, 666)
    assert ln(base, base, base, base, base, 333, 2, 768, 768, 1, ctypes.byref(lp)) == -4                        # fp8 / MX: D = 3072 only
    assert ln(base, base, base, base, base, 333, 2, 3072, 2304, 3, ctypes.byref(lp)) == 0
    assert ln(base, base, base, base, base, 333, 2, 3072, 2296, 3, ctypes.byref(lp)) == -1                      # a row of e2m3 codes: 2304 bytes
    qp = _hip.QkNormRopePlan(-9)
    qk = lambda q, k, cos, S, heads, text, stats, slots, plan: lib.bya_qknorm_rope_plan(q, k, base, base, base, base, cos, cos, 2, S, heads,
                                                                                     3 * heads * 64, (S + 3) * 3 * heads * 64, text, stats, slots, plan)
    assert qk(None, None, base, 37, 6, 5, None, 0, ctypes.byref(qp)) == -1 and qp.stats == -9
    assert qk(base, base, base, 37, 6, 5, None, 0, None) == -1
    assert qk(base, base, None, 37, 6, 5, None, 0, ctypes.byref(qp)) == -1                                       # rows to rotate, no tables
    assert qk(base, base, base, 37, 6, 5, base, 65, ctypes.byref(qp)) == -1
    assert qk(base + 8, base, base, 37, 6, 5, None, 0, ctypes.byref(qp)) == -2
    assert qk(base, base, base, 37, 6, 5, None, 0, ctypes.byref(qp)) == 0
    assert (qp.stats, qp.only, qp.grid, qp.slots, qp.pairs, qp.waves) == (0, 0, 28, 0, 888, 111)
    assert qk(None, base, None, 37, 6, 37, base, 8, ctypes.byref(qp)) == 0
    assert (qp.stats, qp.only, qp.grid, qp.slots, qp.pairs, qp.waves) == (1, 2, 14, 8, 444, 56)
    # the small step kernels' plan queries: validate like their entry points, fill the plan, leave it alone on rejection
    sp = _hip.StepPlan(-9)
    assert lib.bya_linear_small_m_plan(base, None, base, 8, 512, 1280, 0, ctypes.byref(sp)) == -1 and sp.kernel == -9
    assert lib.bya_linear_small_m_plan(base, base, base, 8, 512, 1280, 0, None) == -1
    assert lib.bya_linear_small_m_plan(base, base + 8, base, 8, 512, 1280, 0, ctypes.byref(sp)) == -2
    assert lib.bya_linear_small_m_plan(base, base, base, 8, 512, 1280, 2, ctypes.byref(sp)) == -4 and sp.kernel == -9     # gelu_erf
    assert lib.bya_linear_small_m_plan(base, base, base, 8, 18432, 1280, 0, ctypes.byref(sp)) == 0                        # the face mapper: 8 rows
    assert (sp.kernel, sp.grid, sp.rounds, sp.items, sp.items_per_round) == (8, 4608, 3, 18432, 512)
    assert lib.bya_linear_small_m_plan(base, base, base, 2, 18432, 512, 4, ctypes.byref(sp)) == 0 and (sp.kernel, sp.rounds) == (2, 1)
    assert lib.bya_router_scores_plan(base, base, base, base, None, base, 2, 17550, 16, 32, ctypes.byref(sp)) == -1
    assert lib.bya_router_scores_plan(base, base, base, base, base, base, 2, 17550, 16, 31, ctypes.byref(sp)) == -4
    assert lib.bya_router_scores_plan(base, base, base, base, base, base, 2, 17550, 16, 32, ctypes.byref(sp)) == 0
    assert (sp.kernel, sp.grid, sp.rounds, sp.items, sp.items_per_round) == (1, 256, 2, 1097, 1024)                       # keys in LDS
    assert lib.bya_router_scores_plan(base, base, base, base, base, base, 2, 4095, 16, 32, ctypes.byref(sp)) == 0
    assert (sp.kernel, sp.grid, sp.rounds, sp.items, sp.items_per_round) == (0, 128, 1, 256, 256)                         # one wave per tile
    assert lib.bya_act_add_plan(base, base, base, 17550 * 3072, 1, ctypes.byref(sp)) == 0
    assert (sp.kernel, sp.grid, sp.rounds, sp.items, sp.items_per_round) == (0, 4096, 7, 17550 * 384, 4096 * 256)
    assert lib.bya_act_add_plan(base, base, base + 8, 4096, 1, ctypes.byref(sp)) == -2 and lib.bya_act_add_plan(base, None, base, 4100, 1, ctypes.byref(sp)) == -1
    sc = _hip.SchedCoef()
    assert lib.bya_cfg_scheduler_step_plan(base, 2, 100, base, base, 1000, ctypes.byref(sc), ctypes.byref(sp)) == -1      # pred_stride < n
    assert lib.bya_cfg_scheduler_step_plan(base, 2, 1000, base, None, 1000, ctypes.byref(sc), ctypes.byref(sp)) == -1
    assert lib.bya_cfg_scheduler_step_plan(base, 2, 1064, base, base, 1000, ctypes.byref(sc), ctypes.byref(sp)) == 0
    assert (sp.kernel, sp.grid, sp.rounds, sp.items, sp.items_per_round) == (0, 4, 1, 1000, 1024)
    # one-stream audio weights do not exist: refused before the alignment check behind it, which one face stream reaches
    assert lib.bya_masked_combine(base, base, base, base, 1, 1.0, 1, 1, 64, 12, 16, 1024, 0, None) == -4
    assert lib.bya_masked_combine(base, base, base, None, 0, 1.0, 1, 1, 64, 12, 16, 1024, 0, None) == -2
    assert lib.bya_routed_mix(base, base, base, base, None, 1, 1, 1, 64, 12, 0, None) == -4
    assert lib.bya_routed_mix(base, base, None, base, None, 0, 1, 1, 64, 12, 0, None) == -2
    # the RCCL entry points validate their arguments before touching a communicator
    assert lib.bya_allgather_kv(None, None, None, None, 1, 1, None, None) == -1
    cnt = (ctypes.c_int64 * 2)(1, 1)
    assert lib.bya_alltoall_router(None, None, cnt, cnt, 2, None, None) == -1


def test_struct_layout_matches_header():
    """ctypes mirrors of bya_gemm_desc / bya_attn_desc / bya_gemm_plan: field order and sizes as in the header."""
    from bind_your_avatar_implementation_amd import _hip
    src = open(os.path.join(ROOT, "include", "bya.h")).read()
    for cname, cls in (("bya_gemm_desc", _hip.GemmDesc), ("bya_attn_desc", _hip.AttnDesc), ("bya_gemm_plan", _hip.GemmPlan),
                       ("bya_attn_plan_info", _hip.AttnPlan), ("bya_attn_kv_mix_plan_info", _hip.AttnMixPlan),
                       ("bya_attn_tiny_plan_info", _hip.AttnTinyPlan), ("bya_rowgemm512_plan_info", _hip.RowGemmPlan),
                       ("bya_router_group_attn_plan_info", _hip.GroupAttnPlan), ("bya_router_chain_plan_info", _hip.RouterChainPlan),
                       ("bya_layernorm_plan_info", _hip.LayerNormPlan), ("bya_qknorm_rope_plan_info", _hip.QkNormRopePlan),
                       ("bya_step_plan_info", _hip.StepPlan)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            first, *more = decl.split(",")
            typ, name = re.match(r"(.*?)(\w+)$", first.strip(), flags=re.S).groups()
            fields += [(name, typ.strip())] + [(n.strip(), typ.strip()) for n in more]
        assert [f[0] for f in fields] == [f[0] for f in cls._fields_], cname
        size = {"int32_t": 4, "int64_t": 8, "float": 4, "const float*": 8, "int32_t*": 8}
        for (n, typ), (_, ct) in zip(fields, cls._fields_):
            assert ctypes.sizeof(ct) == size[typ], (cname, n)


def test_product_path_fails_loudly_without_gpu():
    """No CPU fallback: a CPU-resident model must refuse to run instead of computing with torch."""
    import torch
    from bind_your_avatar_implementation_amd import BindyouravatarTransformer3DModel
    with torch.device("meta"):
        m = BindyouravatarTransformer3DModel(num_layers=1, in_channels=48, use_rotary_positional_embeddings=True,
                                             use_learned_positional_embeddings=True, is_train_audio=True)
    from bind_your_avatar_implementation_amd.engine import DenoiseEngine
    with pytest.raises(RuntimeError, match="GPU"):
        DenoiseEngine(m)
    src = open(os.path.join(ROOT, "bind_your_avatar_implementation_amd", "engine.py")).read() + \
        open(os.path.join(ROOT, "bind_your_avatar_implementation_amd", "ops.py")).read() + \
        open(os.path.join(ROOT, "bind_your_avatar_implementation_amd", "transformer.py")).read()
    assert "oracle" not in src.replace("oracle's", ""), "the product must never import the oracle"
    assert "F.scaled_dot_product_attention" not in src and "torch.nn.functional" not in src


def test_generated_gemm_schedules_match_their_tables():
    """The hand-placed instruction streams of gemm_v4.hip, gemm_fp8_v4.hip and attn_w4.hip are emitted by
    tools/gen_*_schedule.py from placement tables; the committed sources must be exactly what the tables generate."""
    import subprocess
    import sys
    for gen in ("gen_gemm_v4_schedule.py", "gen_gemm_v5_schedule.py", "gen_gemm_v6_schedule.py", "gen_gemm_fp8_schedule.py", "gen_attn_w4_schedule.py"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen), "--check"], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr


def test_isa_fingerprint_reads_streams_and_metadata():
    """tools/isa_fingerprint.py: the stream filter keeps memory / matrix / wait / barrier / branch instructions in order, with
    operands only for s_waitcnt and s_nop, and the metadata reader takes a kernel's own fields, not its arguments'; then one
    small translation unit end to end (hipcc cross-compiles without a GPU)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_fingerprint as fp
    finally:
        sys.path.pop(0)
    asm = "\n".join([
        "\t.text", "helper:", "\ts_nop 3", ".Lfunc_end0:",
        "k1:", "\ts_load_dwordx2 s[2:3], s[0:1], 0x0", "\ts_waitcnt lgkmcnt(0)  ; wait", "\tv_mov_b32_e32 v1, 0",
        "\tbuffer_load_dwordx4 v[0:3], v4, s[4:7], 0 offen lds", ".LBB1_2:", "\tv_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]",
        "\ts_nop  15", "\tds_read_b128 v[8:11], v12 offset:2048", "\ts_cbranch_scc1 .LBB1_2", "\ts_barrier", "\ts_endpgm", ".Lfunc_end1:",
        "\t.amdgpu_metadata", "---", "amdhsa.kernels:",
        "  - .agpr_count:     128", "    .args:", "      - .name:           p", "        .size:           8",
        "    .group_segment_fixed_size: 0", "    .name:           k1", "    .private_segment_fixed_size: 16",
        "    .sgpr_count:     106", "    .sgpr_spill_count: 5", "    .vgpr_count:     384", "    .vgpr_spill_count: 3",
        "amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...",
    ])
    streams = fp.kernel_streams(asm)
    assert streams["k1"] == ["s_waitcnt lgkmcnt(0)", "buffer_load_dwordx4", "v_mfma_f32_16x16x32_bf16", "s_nop 15", "ds_read_b128",
                             "s_cbranch_scc1", "s_barrier", "s_endpgm"]
    assert streams["helper"] == ["s_nop 3"]
    meta = fp.kernel_metadata(asm)
    assert list(meta) == ["k1"]
    assert meta["k1"][".vgpr_count"] == "384" and meta["k1"][".agpr_count"] == "128" and meta["k1"][".sgpr_spill_count"] == "5"
    assert meta["k1"][".private_segment_fixed_size"] == "16" and meta["k1"][".group_segment_fixed_size"] == "0"
    lines = fp.fingerprint("calib.hip")
    assert len(lines) == 1 and lines[0].startswith("calib.hip ") and "mfma_calibration_kernel" in lines[0]
    fields = dict(f.split("=") for f in lines[0].split()[2:])
    assert fields["agpr_count"] == "256" and int(fields["stream_len"]) > 256 and len(fields["stream_sha1"]) == 16


def test_valu_only_kernels_hold_no_packed_fp32(lib_path):
    """packed-fp32 VALU arithmetic (v_pk_mul / fma / add / mov) in the VALU-only kernels returned
    wrong lanes whenever another process kept MFMA workgroups resident; build.py compiles those translation units
    without the SLP vectoriser.  Guard it on the built device code (and check the disassembly is really read: the
    router's tiny-attention kernels hold MFMAs, the MFMA GEMM holds both)."""
    import shutil
    import subprocess
    import tempfile
    from bind_your_avatar_implementation_amd import build
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = [os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(t) for t in tools):
        pytest.skip("ROCm llvm binutils not found")
    packed = re.compile(r"\bv_pk_(mul|fma|add|mov)_(f32|b32)\b")

    def device_asm(src, tmp):
        obj = os.path.join(build.PKG_DIR, "build", src.replace(".hip", ".o"))
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([tools[0], f"--dump-section=.hip_fatbin={fat}", obj], check=True, stdin=subprocess.DEVNULL)
        subprocess.run([tools[1], "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                        f"--output={co}", "--unbundle"], check=True, stdin=subprocess.DEVNULL)
        return subprocess.run([tools[2], "-d", co], check=True, capture_output=True, text=True,
                              stdin=subprocess.DEVNULL).stdout

    tmp = tempfile.mkdtemp()
    try:
        for src in sorted(build.NO_SLP_SOURCES):
            asm = device_asm(src, tmp)
            assert "s_endpgm" in asm, f"{src}: no device code disassembled"
            hits = packed.findall(asm)
            assert not hits, f"{src}: {len(hits)} packed-fp32 instructions in a VALU-only translation unit"
        assert "v_mfma" in device_asm("router.hip", tmp)
        # The MFMA translation units DO hold packed-fp32 instructions (epilogues, softmax): if the multi-process finding of
        # DESIGN.md section 5 is what it looks like, they are exposed in the same setting (several processes on one GPU).
        # That finding is a workaround, not a closed root cause; the exposure is recorded here so that it is a number and
        # not a guess (profiles/history/r3_packed_fp32_counts.json, rewritten with BYA_RECORD_PACKED_COUNTS=1), and must not grow
        # unnoticed.
        import json
        rec_path = os.path.join(ROOT, "profiles", "history", "r3_packed_fp32_counts.json")
        counts = {src: len(packed.findall(device_asm(src, tmp))) for src in ("gemm.hip", "gemm_v4.hip", "gemm_fp8_v4.hip", "attn.hip", "rowgemm.hip")}
        print("packed-fp32 instructions in the MFMA translation units:", counts)
        if os.environ.get("BYA_RECORD_PACKED_COUNTS") == "1":
            with open(rec_path, "w") as f:
                json.dump(counts, f, indent=1, sort_keys=True)
        assert counts["gemm.hip"] > 0                               # the pattern does match where packed ops exist
        recorded = json.load(open(rec_path))
        for src, n in counts.items():
            assert src in recorded and n <= 1.25 * recorded[src] + 16, (src, n, recorded.get(src))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_library_path_override_fails_loudly_when_the_file_is_missing(tmp_path):
    """BYA_HIP_LIB points the loader at another build of the library (A/B runs of two builds in one call); a path that does
    not exist must fail like a missing in-tree build does -- there is no fallback to look for."""
    import subprocess
    import sys
    code = ("import torch\n"
            "from bind_your_avatar_implementation_amd import _hip\n"
            "try:\n    _hip.load()\nexcept Exception as e:\n    print(type(e).__name__, str(e)[:200]); raise SystemExit(3)\n"
            "print('loaded')\n")
    env = dict(os.environ, BYA_HIP_LIB=str(tmp_path / "nope.so"), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=300)
    assert r.returncode == 3 and "nope.so" in r.stdout and "no fallback" in r.stdout, (r.stdout, r.stderr[-500:])


def test_options_are_set_through_the_abi_and_never_through_the_environment(lib_path):
    """(r6) The C entry points read no environment: `grep getenv csrc/` finds nothing.  Options go through bya_set_option /
    bya_get_option: defaults, ranges, unknown keys; the Python host maps its BYA_* variables onto them when the library is
    loaded (``_hip.apply_env_options``) and ``ops.options`` scopes a change."""
    import subprocess
    import sys
    from bind_your_avatar_implementation_amd import _hip
    csrc = os.path.join(ROOT, "bind_your_avatar_implementation_amd", "csrc")
    for f in os.listdir(csrc):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f"{f}: the C ABI must not read the environment"
    src = open(os.path.join(ROOT, "include", "bya.h")).read()
    keys = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"BYA_OPT_(\w+) = (\d+)", src))
    count = keys.pop("count")
    assert keys == _hip.OPTIONS and count == len(keys)                   # header enum = the Python table
    refs = dict((m.group(1).lower(), int(m.group(2))) for m in re.finditer(r"BYA_REF_(\w+) = (\d+)", src))
    assert refs == _hip.REFERENCE_FORMS
    lib = _hip.load()
    for name, default in _hip.OPTION_DEFAULTS.items():
        _hip.set_option(name, default)
        assert _hip.get_option(name) == default
    assert lib.bya_set_option(99, 0) == -1 and lib.bya_set_option(-1, 0) == -1            # unknown key
    assert lib.bya_set_option(_hip.OPTIONS["gemm_splitk"], 3) == -1                       # out of range: nothing changes
    assert lib.bya_set_option(_hip.OPTIONS["p2p_groups"], 8) == -1 and lib.bya_set_option(_hip.OPTIONS["p2p_groups"], 64) == 0
    assert _hip.get_option("gemm_splitk") == 0 and _hip.get_option("p2p_groups") == 64
    _hip.set_option("p2p_groups", 0)
    assert lib.bya_get_option(_hip.OPTIONS["gemm_tile"], None) == -1
    # the environment reaches the table once, at load time, in a fresh process
    code = ("from bind_your_avatar_implementation_amd import _hip; _hip.load(); "
            "print(_hip.get_option('gemm_splitk'), _hip.get_option('gemm_variant'), _hip.get_option('gemm_tile'), _hip.get_option('attn_streamk'))")
    env = dict(os.environ, BYA_GEMM_SPLITK="0", BYA_GEMM_VARIANT="w8", BYA_GEMM_TILE="4", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.stdout.split() == ["0", "1", "4", "1"], out.stdout + out.stderr[-500:]
