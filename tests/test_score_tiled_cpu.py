"""The tiled importance + top-k path (more tokens than one workgroup's LDS holds) without a GPU: the ABI additions, the scratch
size query, every argument check of rajni_score_select_ws, the new configs, and a numpy fp32 restatement of the tiled
summation order held to the project's importance budget."""
import ctypes as C

import numpy as np
import pytest

import numerics as nm
import numerics_tiled as nt
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

NEW_SYMBOLS = ("rajni_score_select_workspace_bytes", "rajni_score_select_ws", "rajni_debug_force_score_tiled")
FITS = [(197, 12, 64), (577, 16, 64)]
TILED = [(626, 2, 64), (1374, 6, 64), (1025, 16, 64), (577, 16, 80), (320, 2, 128)]
CODES = (nat.RAJNI_BF16, nat.RAJNI_F16, nat.RAJNI_F32)


def _err(lib):
    return lib.rajni_last_error().decode()


def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = nat.load_library()
    for sym in NEW_SYMBOLS:
        assert sym in nat.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    assert nat.SCORE_TILE_TOKENS == nt.TILE and nat.SCORE_TILED_MAX_TOKENS == nt.MAX_N


def test_workspace_is_zero_wherever_one_workgroup_holds_the_shape():
    lib = nat.load_library()
    for N, H, D in FITS + [(2, 1, 8), (33, 2, 32), (61, 4, 80), (300, 2, 128), (595, 16, 64)]:
        assert nt.single_workgroup_lds_bytes(N, H, D) <= 160 * 1024
        for B in (1, 7, 256):
            for code in CODES:
                assert lib.rajni_score_select_workspace_bytes(B, N, H, D, code) == 0, (B, N, H, D, code)


@pytest.mark.parametrize("N,H,D", TILED + [(4097, 2, 64), (610, 12, 64), (nt.MAX_N, 1, 8)])
def test_workspace_size_is_the_documented_layout(N, H, D):
    """> 0 for what the single-workgroup layout refuses, and exactly the four fp32 regions of DESIGN.md - a size that moves with
    32-token tiles (N and N + 1 across a tile boundary differ by one tile's partials)"""
    lib = nat.load_library()
    assert nt.single_workgroup_lds_bytes(N, H, D) > 160 * 1024
    for B in (1, 2, 5):
        for code in CODES:
            got = lib.rajni_score_select_workspace_bytes(B, N, H, D, code)
            assert got == nt.workspace_bytes(B, N, H, D) > 0 and got % 256 == 0, (B, N, H, D, code, got)
    assert lib.rajni_score_select_workspace_bytes(0, N, H, D, nat.RAJNI_BF16) == 0
    assert lib.rajni_score_select_workspace_bytes(1, N, H, D, 7) == 0


def test_the_threshold_is_the_single_workgroup_layout():
    """the first N that needs scratch is the first N whose layout exceeds 160 KiB: a shape that fits today keeps its kernel"""
    lib = nat.load_library()
    for H, D in ((2, 64), (6, 64), (12, 64), (16, 64), (16, 80), (2, 128), (4, 32), (3, 8)):
        first = next(N for N in range(8, 6000) if nt.single_workgroup_lds_bytes(N, H, D) > 160 * 1024)
        assert lib.rajni_score_select_workspace_bytes(1, first - 1, H, D, nat.RAJNI_BF16) == 0, (H, D, first)
        assert lib.rajni_score_select_workspace_bytes(1, first, H, D, nat.RAJNI_BF16) > 0, (H, D, first)
    # beyond the cap, and head dims no kernel takes: nothing to size (the call itself refuses)
    assert lib.rajni_score_select_workspace_bytes(1, nt.MAX_N + 1, 2, 64, nat.RAJNI_BF16) == 0
    assert lib.rajni_score_select_workspace_bytes(1, 4097, 2, 60, nat.RAJNI_BF16) == 0
    assert lib.rajni_score_select_workspace_bytes(1, 4097, 2, 136, nat.RAJNI_BF16) == 0


def test_force_hook_sizes_scratch_for_small_shapes_and_resets():
    lib = nat.load_library()
    lib.rajni_debug_force_score_tiled(1)
    try:
        for N, H, D in FITS + [(2, 1, 8), (33, 3, 32)]:
            assert lib.rajni_score_select_workspace_bytes(3, N, H, D, nat.RAJNI_F16) == nt.workspace_bytes(3, N, H, D)
    finally:
        lib.rajni_debug_force_score_tiled(0)
    assert lib.rajni_score_select_workspace_bytes(3, 197, 12, 64, nat.RAJNI_F16) == 0


def test_score_select_ws_argument_checks_run_without_a_device():
    """rajni_score_select_ws(qkv, B, N, H, D, eps, num_prefix, keep, scores_out, keep_idx, next_scores, dtype, workspace,
    workspace_bytes, stream): every refusal is RAJNI_ERR_INVALID with the function's name, before anything touches a device"""
    lib = nat.load_library()
    buf = (C.c_char * 1024)()
    p = (C.addressof(buf) + 255) // 256 * 256            # a 256-byte aligned non-null pointer no check dereferences
    BF = nat.RAJNI_BF16
    need = lib.rajni_score_select_workspace_bytes(1, 626, 2, 64, BF)
    assert need > 0
    bad = [
        (None, 1, 626, 2, 64, 1e-6, 1, 5, p, p, p, BF, p, need),            # qkv null
        (p, 1, 626, 2, 64, 1e-6, 1, 5, p, None, p, BF, p, need),            # keep_idx null with keep > 0
        (p, 1, 626, 2, 64, 1e-6, 1, 0, None, None, None, BF, p, need),      # scores only, scores_out null
        (p, 1, 626, 2, 64, 1e-6, 0, 5, p, p, p, BF, p, need),               # prefix range
        (p, 1, 626, 2, 64, 1e-6, 33, 5, p, p, p, BF, p, need),
        (p, 1, 5, 2, 64, 1e-6, 5, 1, p, p, p, BF, None, 0),                 # no patch token
        (p, 0, 626, 2, 64, 1e-6, 1, 5, p, p, p, BF, p, need),               # B
        (p, 1, 626, 2, 64, 1e-6, 1, -1, p, p, p, BF, p, need),              # keep range
        (p, 1, 626, 2, 64, 1e-6, 1, 626, p, p, p, BF, p, need),
        (p, 1, 626, 2, 64, 1e-6, 5, 622, p, p, p, BF, p, need),
        (p, 1, 626, 2, 64, 1e-6, 1, 5, p, p, p, 9, p, need),                # dtype
        (p, 1, 626, 2, 64, 1e-6, 1, 5, p, p, p, BF, None, need),            # workspace null where scratch is needed
        (p, 1, 626, 2, 64, 1e-6, 1, 5, p, p, p, BF, p + 16, need),          # 256-byte alignment
        (p, 1, 626, 2, 64, 1e-6, 1, 5, p, p, p, BF, p, need - 1),           # workspace_bytes too small
        (p, 1, 626, 2, 64, 1e-6, 1, 0, p, None, None, BF, p, 0),
        (p, 1, 197, 12, 64, 1e-6, 1, 5, p, p, p, BF, p + 8, 0),             # (alignment holds for a scratch that is not needed too)
    ]
    for args in bad:
        assert lib.rajni_score_select_ws(*args, None) == 1, args
        assert "rajni_score_select_ws" in _err(lib), (_err(lib), args)
    # beyond the cap: unsupported, and the message states the cap (no launch is reached: the refusal is the launcher's first act)
    assert lib.rajni_score_select_workspace_bytes(1, nt.MAX_N + 1, 2, 64, BF) == 0
    assert lib.rajni_score_select_ws(p, 1, nt.MAX_N + 1, 2, 64, 1e-6, 1, 5, p, p, p, BF, None, 0, None) == 2
    assert str(nt.MAX_N) in _err(lib)
    # the entry points without scratch keep their refusal and may name the new one
    assert lib.rajni_importance(p, p, 1, 1374, 6, 64, 1e-6, BF, None) == 2
    assert "LDS" in _err(lib) and "rajni_score_select_ws" in _err(lib)
    assert lib.rajni_score_select(p, 1, 626, 2, 64, 1e-6, 5, p, p, p, BF, None) == 2 and "LDS" in _err(lib)
    assert lib.rajni_score_select_prefix(p, 1, 630, 2, 64, 1e-6, 5, 5, p, p, p, BF, None) == 2 and "LDS" in _err(lib)


def test_new_configs():
    m = ts.CONFIGS["vit_micro_patch16_400"]
    assert (m.img_size, m.patch_size, m.embed_dim, m.num_heads, m.depth, m.num_classes) == (400, 16, 128, 2, 4, 10)
    assert m.num_patches + 1 == 626 and m.reg_tokens == 0
    # 42 056 words of LDS in the single-workgroup layout against 40 960
    assert nt.single_workgroup_lds_bytes(626, 2, 64) == 4 * 42056
    r = ts.CONFIGS["vit_micro_reg4_patch16_400"]
    assert r.reg_tokens == 4 and r.no_embed_class and r.layer_scale and r.num_patches + 5 == 630
    assert (r.img_size, r.embed_dim, r.num_heads, r.depth) == (400, 128, 2, 4)
    d, d224 = ts.CONFIGS["vit_small_patch14_reg4_dinov2_518"], ts.CONFIGS["vit_small_patch14_reg4_dinov2"]
    assert d.num_patches + 5 == 1374
    assert {**d.to_dict(), "img_size": 224} == d224.to_dict()
    lib = nat.load_library()
    for cfg in (m, r, d):
        n0 = cfg.num_patches + 1 + cfg.reg_tokens
        assert lib.rajni_score_select_workspace_bytes(2, n0, cfg.num_heads, cfg.embed_dim // cfg.num_heads, nat.RAJNI_BF16) > 0


def test_wrapper_accepts_the_long_configs():
    sched = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
    for name, P in (("vit_micro_patch16_400", 1), ("vit_micro_reg4_patch16_400", 5)):
        d = rajni_amd.RAJNIViTWrapper(ts.create_model(name), sched).check_supported()
        assert d["num_prefix"] == P


def test_plan_workspace_grows_by_exactly_the_score_scratch():
    """rajni_vit_workspace_bytes: unchanged wherever the scratch is zero bytes (the hook shows the region is there), and a long
    plan is a short plan's buffers plus the scratch of (B, n0, H, D)"""
    lib = nat.load_library()
    plan = nat.VitPlan()
    plan.dtype, plan.B, plan.in_chans, plan.img_size, plan.patch_size = nat.RAJNI_BF16, 3, 3, 64, 16
    plan.C, plan.H, plan.D, plan.depth, plan.hidden, plan.num_classes = 128, 2, 64, 4, 512, 10
    base = lib.rajni_vit_workspace_bytes(C.byref(plan))
    lib.rajni_debug_force_score_tiled(1)
    try:
        assert lib.rajni_vit_workspace_bytes(C.byref(plan)) == base + nt.workspace_bytes(3, 17, 2, 64)
    finally:
        lib.rajni_debug_force_score_tiled(0)
    assert lib.rajni_vit_workspace_bytes(C.byref(plan)) == base
    plan.img_size = 400
    long_ = lib.rajni_vit_workspace_bytes(C.byref(plan))
    rows, a = 3 * 626, nt.align256
    buffers = (2 * a(rows * 128 * 4) + a(rows * 128 * 2) + a(rows * 384 * 2) + a(rows * 128 * 2) + a(rows * 512 * 2) + a(3 * 128 * 2)
               + a(rows * 2))
    assert long_ == buffers + nt.workspace_bytes(3, 626, 2, 64)


# ---------------------------------------------------------------------------------------------------------------
# the tiled summation order against the project's budget
# ---------------------------------------------------------------------------------------------------------------

# the GPU test's shapes: the stress shapes it forces through the tiled kernels, and its natural long ones
ORDER_SHAPES = [(4, 197, 12, 64), (3, 61, 4, 80), (2, 626, 2, 64), (1, 1374, 6, 64), (1, 4097, 2, 64)]


@pytest.mark.parametrize("B,N,H,D", ORDER_SHAPES)
def test_tiled_summation_order_is_inside_the_importance_budget(B, N, H, D):
    """numerics.importance_budget is |err| <= (u_out + 4 e32) |want| with e32 measured per input from numpy's own fp32 run.  The
    fp32 restatement of the TILED order (tests/numerics_tiled.py: per-tile partial sums joined in tile order for the softmax
    sum and the token mean, norms against that mean) must use at most HALF of the 4 e32 allowance before the output rounding,
    and its rounded result must sit inside the whole budget - for every stress kind, every output type, at the GPU test's
    shapes.  So the budget is satisfiable by the new order with room to spare, with no device in the loop."""
    for kind in nm.IMP_KINDS:
        for dt in ("bf16", "fp16", "fp32"):
            qkv = nm.importance_qkv(kind, B, N, H, D, dt)
            want, bud, e32 = nm.importance_budget(qkv, H, dt)
            got32 = nt.tiled_scores_f32(qkv, H).astype(np.float64)
            order = float((np.abs(got32 - want) / np.abs(want)).max())
            print(f"[tiled order] {kind} {dt} {(B, N, H, D)}: e32 {e32:.3g}, tiled-order fp32 error {order:.3g} = {order / e32:.2f} e32")
            assert order <= 2 * e32, (kind, dt, order, e32)
            nm.assert_within(nm.round_to(got32.astype(np.float32), dt), want, bud, f"tiled order {kind} {dt} {(B, N, H, D)}")

