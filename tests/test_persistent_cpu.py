"""The persistent-kernel tests (tests/test_gpu_persistent.py) checked on the CPU: the grid hook and what the plan reports
under it, that the chosen caps drive some workgroup through every kind of tile-to-tile step, and that the inputs are such
that a tile or item computed from the WRONG operands (another tile's rows, another item's K/V) would leave its budget -
a bit-equality between two launches that share a bug proves nothing, the budgets against fp64 have to be able to tell.
No GPU: nothing is launched."""

import numpy as np
import pytest
import torch

import numerics as nm
import numerics_fp8 as n8
import numerics_persistent as pz
from rajni_amd import _native as nat
from test_linear_plan_cpu import args, plan

OK = 0
WIDE, MID, F8_STREAM, F8_WIDE, SMALL, T_F32 = (nat.TILING_WIDE, nat.TILING_MID, nat.TILING_F8_STREAM, nat.TILING_F8_WIDE,
                                               nat.TILING_SMALL, nat.TILING_F32)
NBLK_DEFAULT = 1600 * 1024


@pytest.fixture
def hooks():
    lib = nat.lib()

    def set_hooks(force=0, force_f8=0, nblk=NBLK_DEFAULT, cap=0):
        lib.rajni_debug_force_gemm_tiling(force)
        lib.rajni_debug_force_f8_tiling(force_f8)
        lib.rajni_debug_set_gemm_nblock_bytes(nblk)
        lib.rajni_debug_set_persistent_workgroups(cap)
    yield set_hooks
    set_hooks()


def fields(p):
    return (p.tiling, p.tiles_n, p.total_tiles, p.nblk, p.lds_bytes)


def test_hook_is_exported_and_the_abi_version_stays():
    lib = nat.lib()
    assert "rajni_debug_set_persistent_workgroups" in nat.EXPORTED_SYMBOLS and hasattr(lib, "rajni_debug_set_persistent_workgroups")
    assert lib.rajni_abi_version() == nat.ABI_VERSION == 8


# (what the launch is, hooks, arguments, tiling expected)
PAD = dict(ldc=pz.LD, ldr=pz.LD)
PLAN_CASES = [
    ("wide by shape, more tiles than CUs", {}, args(M=20000, N=2304, K=768), WIDE),
    ("mid by shape, more tiles than CUs", {}, args(M=20000, N=768, K=768), MID),
    ("wide forced, the test shape", dict(force=4), args(M=pz.M, N=pz.N, K=192, **PAD), WIDE),
    ("mid forced, the test shape", dict(force=5), args(M=pz.M, N=pz.N, K=832, **PAD), MID),
    ("mid forced, fp16 fp32-stream RESID", dict(force=5), args(M=pz.M, N=pz.N, K=256, dtype=nat.RAJNI_F16, epilogue=nat.EPI_BIAS_RESID,
                                                              resid=True, stream_f32=1, **PAD), MID),
    ("wide forced, fp8 weights", dict(force=4), args(M=pz.M, N=pz.N, K=832, w_scale=True, **PAD), WIDE),
    ("wide forced, N blocks of one column tile", dict(force=4, nblk=-1), args(M=pz.M, N=pz.N, K=192, **PAD), WIDE),
    ("mid forced, N blocks of two column tiles", dict(force=5, nblk=-2), args(M=pz.M, N=pz.N, K=256, **PAD), MID),
    ("fp8 x fp8 256x128", dict(force_f8=1), args(M=pz.M, N=pz.N, K=512, w_scale=True, x_scale=True, **PAD), F8_STREAM),
    ("fp8 x fp8 256x256", dict(force_f8=2), args(M=pz.M, N=pz.N, K=1280, w_scale=True, x_scale=True, **PAD), F8_WIDE),
    ("fp8 x fp8 by shape, more tiles than CUs", {}, args(M=20000, N=3072, K=768, w_scale=True, x_scale=True), F8_WIDE),
    ("fp8 x fp8 RESID", {}, args(M=20000, N=768, K=3072, w_scale=True, x_scale=True, epilogue=nat.EPI_BIAS_RESID, resid=True,
                                stream_f32=1), F8_STREAM),
]


@pytest.mark.parametrize("what,hk,a,tiling", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_plan_reports_the_capped_grid_and_nothing_else_changes(what, hk, a, tiling, hooks):
    hooks(**hk)
    rc, base, msg = plan(a)
    assert rc == OK, msg
    assert base.tiling == tiling and base.grid == min(base.total_tiles, 256)
    for cap in (1, 2, 3, 4, 5, 7, 100, 256, 1000):
        hooks(cap=cap, **hk)
        rc, p, msg = plan(a)
        assert rc == OK, msg
        assert p.grid == min(cap, base.grid), (what, cap)
        assert fields(p) == fields(base), (what, cap)
    hooks(cap=0, **hk)
    rc, p, _ = plan(a)
    assert rc == OK and p.grid == base.grid and fields(p) == fields(base)
    hooks(cap=-3, **hk)                                    # anything below 1 is "no cap"
    assert plan(a)[1].grid == base.grid


def test_one_workgroup_per_tile_launches_are_not_capped(hooks):
    for a, force, tiling in ((args(M=200, N=768, K=768), 1, SMALL), (args(M=2048, N=768, K=768, dtype=nat.RAJNI_F32), 0, T_F32)):
        hooks(force=force)
        base = plan(a)[1]
        hooks(force=force, cap=2)
        p = plan(a)[1]
        assert p.tiling == base.tiling == tiling and p.grid == base.grid == base.total_tiles > 2


# ---------------------------------------------------------------------------------------------------------------
# the caps reach the transitions
# ---------------------------------------------------------------------------------------------------------------

def gemm_plans(hooks, caps):
    """(label, M, N, bn, [(total, tiles_n, nblk, grid) per cap]) for every GEMM tiling and shape of the GPU tests, the
    linear ones as rajni_debug_linear_plan reports them"""
    out = []
    seen = set()
    for fmt, tiling, K in pz.GEMM16_CASES:
        if (tiling, K) in seen:
            continue        # the plan does not depend on the operand format (checked per format above)
        seen.add((tiling, K))
        a = args(M=pz.M, N=pz.N, K=K, **PAD)
        for nblk in (NBLK_DEFAULT,) + tuple(pz.NBLOCK_UNDER_CAP[1]):
            used = []
            for cap in (caps if nblk == NBLK_DEFAULT else (pz.NBLOCK_UNDER_CAP[0],)):
                hooks(force=tiling, nblk=nblk, cap=cap)
                rc, p, msg = plan(a)
                assert rc == OK and p.tiling == tiling, msg
                used.append((p.total_tiles, p.tiles_n, p.nblk, p.grid))
            out.append((f"tiling {tiling} K {K} nblock {nblk}", pz.M, pz.N, pz.BN[tiling], used))
    for tiling, K in pz.F8_CASES:
        used = []
        for cap in caps:
            hooks(force_f8=tiling, cap=cap)
            rc, p, msg = plan(args(M=pz.M, N=pz.N, K=K, w_scale=True, x_scale=True, **PAD))
            assert rc == OK and p.tiling == (F8_STREAM if tiling == 1 else F8_WIDE), msg
            used.append((p.total_tiles, p.tiles_n, p.nblk, p.grid))
        out.append((f"fp8 tiling {tiling} K {K}", pz.M, pz.N, pz.BN_F8[tiling], used))
    return out


def patch_plans():
    """patch embed has no dry run: its W (at most 320 x 768 x 2 bytes) fits one N block, so nblk = tiles_n, grid = min(cap, tiles)"""
    out = []
    for tiling, P in sorted({(t, P) for _, _, t, P in pz.PATCH_CASES}):
        rows, bn = pz.PATCH_B * (pz.PATCH_S // P) ** 2, pz.BN[tiling]
        tiles_n = -(-pz.PATCH_C // bn)
        total = -(-rows // pz.BM) * tiles_n
        out.append((f"patch tiling {tiling} P {P}", rows, pz.PATCH_C, bn, [(total, tiles_n, tiles_n, min(cap, total)) for cap in pz.PATCH_CAPS]))
    return out


def test_every_tile_is_visited_exactly_once_in_every_walk_used(hooks):
    combos = set()
    for _, _, _, _, used in gemm_plans(hooks, (0,) + pz.GEMM_CAPS) + patch_plans():
        combos.update(used)
    assert len(combos) >= 20
    for total, tiles_n, nblk, grid in sorted(combos):
        assert 1 <= grid <= total
        seen = sorted(t for seq in pz.walk(total, tiles_n, nblk, grid) for t in seq)
        assert seen == sorted((tm, tn) for tm in range(total // tiles_n) for tn in range(tiles_n)), (total, tiles_n, nblk, grid)


def test_the_caps_drive_some_workgroup_through_every_kind_of_step(hooks):
    """interior -> interior, interior -> ragged, ragged -> interior, ragged -> ragged for every GEMM tiling and shape (the
    caps of a case together); an N-block crossing in the runs with forced N blocks"""
    for label, rows, cols, bn, used in gemm_plans(hooks, pz.GEMM_CAPS) + patch_plans():
        kinds, crosses = set(), False
        for total, tiles_n, nblk, grid in used:
            assert total == -(-rows // pz.BM) * -(-cols // bn) and tiles_n == -(-cols // bn), label
            k, c = pz.steps_taken(rows, cols, bn, nblk, grid)
            kinds |= k
            crosses |= c
        if "nblock -" in label:
            assert crosses, f"{label}: no workgroup crosses an N block"
        else:
            assert kinds == {"ii", "ir", "ri", "rr"}, f"{label}: steps taken {sorted(kinds)}"


def test_uncapped_launches_of_the_small_shapes_run_one_tile_per_workgroup(hooks):
    for label, _, _, _, used in gemm_plans(hooks, (0,)):
        for total, _, _, grid in used:
            if "nblock -" not in label:
                assert grid == total, label


# ---------------------------------------------------------------------------------------------------------------
# the tests can tell: wrong operands leave the budget
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,K", sorted({(f, K) for f, _, K in pz.GEMM16_CASES}))
def test_gemm_tiles_from_another_tiles_operands_leave_the_budget(fmt, K):
    case = pz.gemm16_case(fmt, K)
    for tiling in (4, 5):
        if (fmt, tiling, K) not in pz.GEMM16_CASES:
            continue
        for form in case["forms"]:
            frac = pz.swapped_fraction(form, case["pre"], case["b"].astype(np.float64), pz.M, pz.N, pz.BN[tiling], case["m0"])
            assert frac > 0.5, f"{fmt} K {K} tiling {tiling} {form.name}: only {frac:.3f} of a swapped tile's elements leave the budget"


@pytest.mark.parametrize("K", sorted({K for _, K in pz.F8_CASES}))
def test_fp8_gemm_tiles_from_another_tiles_operands_leave_the_bound(K):
    case = pz.f8_case(K)
    for tiling in (1, 2):
        for form in pz.f8_forms(case, tiling):
            frac = pz.swapped_fraction(form, case["pre"], case["b"].astype(np.float64), pz.M, pz.N, pz.BN_F8[tiling], case["m0"])
            assert frac > 0.5, f"fp8 K {K} tiling {tiling} {form.name}: {frac:.3f}"


@pytest.mark.parametrize("dt,out_f32,tiling,P", pz.PATCH_CASES)
def test_patch_tiles_from_another_tiles_operands_leave_the_budget(dt, out_f32, tiling, P):
    case = pz.patch_case(dt, out_f32, P)
    frac = pz.swapped_fraction(case["forms"][0], case["pre"], case["b"].astype(np.float64), case["rows"], case["cols"],
                               pz.BN[tiling], case["m0"])
    assert frac > 0.5, frac


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n_kept", pz.ATTN_NP)
def test_attention_items_differ_by_more_than_their_budgets(n_kept, dt):
    """item i's expected output fails item j's budget in more than half of the elements, for every i != j - so an item
    computed from another item's Q or K/V (a stale buffer, a stale prefetch) cannot pass; the e4m3-output bound likewise"""
    for kind in pz.ATTN_KINDS:
        for gathered in (True, False):
            _, _, want, bud = pz.attention_case(kind, n_kept, gathered, dt)
            w, b = pz.items_of(want), pz.items_of(bud)
            budgets = [("budget", b)]
            if dt == "bf16" and n_kept <= 224:
                scale = float(np.float32(np.abs(want).max() / 448.0))
                budgets.append(("e4m3 bound", pz.items_of(n8.attention_fp8_bound(want, want, scale))))
            for name, bb in budgets:
                over = np.abs(w[:, None] - w[None, :]) > bb[None, :]                # [i, j, np, D]: item i's values under j's budget
                frac = over.mean(axis=(2, 3))
                np.fill_diagonal(frac, 1.0)
                assert frac.min() > 0.5, f"{kind} np {n_kept} gathered {gathered} {dt} {name}: {frac.min():.3f}"


# ---------------------------------------------------------------------------------------------------------------
# the torch restatements used for references computed on the GPU equal the numpy budgets
# ---------------------------------------------------------------------------------------------------------------

def test_torch_budgets_equal_the_numpy_budgets():
    x, w, b = nm.gemm_operands(70, 50, 128, "bf16")
    pre, S, g = nm.gemm_pre(x, w, b)
    t = torch.from_numpy
    pre_t, S_t, g_t = pz.gemm_pre_t(t(x), t(w), t(b))
    assert g_t == g
    np.testing.assert_allclose(pre_t.numpy(), pre, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(S_t.numpy(), S, rtol=1e-13)
    np.testing.assert_allclose(pz.budget_gelu_t(pre_t, S_t, g, "bf16", nm.A_GELU_16).numpy(),
                               nm.budget_gelu(pre, S, g, "bf16", nm.A_GELU_16), rtol=1e-12)
    r, gam, _ = nm.resid_operands(1, 70, 70, 50, "bf16", "fp32")
    want, bud = nm.budget_resid(pre, S, g, r[0].astype(np.float64), gam.astype(np.float64), "fp32")
    want_t, bud_t = pz.budget_resid_t(pre_t, S_t, g, t(r[0]).double(), t(gam).double(), "fp32")
    np.testing.assert_allclose(want_t.numpy(), want, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(bud_t.numpy(), bud, rtol=1e-12)
    for dt in ("bf16", "fp16"):
        qkv = nm.attention_qkv("peaked", 2, 45, 3, 64, dt)
        want, bud = nm.attention_budget(qkv, 3, 0.125, dt)
        want_t, bud_t = pz.attention_budget_t(t(qkv), 3, 0.125, dt)
        np.testing.assert_allclose(want_t.numpy(), want, rtol=1e-11, atol=1e-14)
        np.testing.assert_allclose(bud_t.numpy(), bud, rtol=1e-11)
    got = pre + 0.3 * nm.budget_bias(pre, S, g, "bf16")
    assert abs(pz.worst_ratio_t(t(got), pre_t, t(nm.budget_bias(pre, S, g, "bf16"))) - nm.worst_ratio(got, pre, nm.budget_bias(pre, S, g, "bf16"))[0]) < 1e-9
    assert pz.factor_tiles(517) == (47, 11) and pz.factor_tiles(13) == (13, 1)
