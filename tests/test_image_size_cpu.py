"""Any input size without a device: the resample rule restated (tests/numerics_image.py) against torch's own bicubic-antialias
interpolation, the kernel's error budget against an emulation of the kernel's order, the pins the design rests on (an additive
header, nothing else moves), every refusal of the image record before the first launch, what the wrapper recognises, and for each
forward fixture of tests/test_gpu_image_size.py the proof that it can tell a wrong embedding from the right one.

The refusal tests use the fake-pointer plans of tests/test_features_cpu.py: workspace = NULL, so "workspace too small" means every
check in front of it passed, and nothing is launched either way."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import numerics as nm
import numerics_image as ni
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from test_features_cpu import FAKE, ERR_INVALID, ERR_UNSUPPORTED, IMAGES, LOGITS, _plan, _ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((4, 4), (5, 3)), ((4, 4), (3, 2)), ((4, 4), (2, 6)), ((3, 5), (1, 1)), ((14, 14), (16, 24)), ((37, 37), (16, 16)),
          ((37, 37), (20, 30)), ((16, 16), (37, 37))]
IMAGE_SYMBOLS = ("rajni_resample_pos_embed", "rajni_patch_embed_image", "rajni_patch_embed_workspace_bytes_image",
                 "rajni_vit_workspace_bytes_image", "rajni_vit_forward_image")


def _source(src, C_, seed=0):
    return np.random.default_rng([seed, src[0], src[1], C_]).standard_normal((src[0] * src[1], C_))


# ---- 1. the restatement is torch's rule -------------------------------------------------------------------------------------

@pytest.mark.parametrize("src, dst", SHAPES)
def test_the_restatement_equals_torch_bicubic_antialias_in_fp64(src, dst):
    x = _source(src, 8)
    t = torch.from_numpy(x).reshape(1, src[0], src[1], 8).permute(0, 3, 1, 2)
    want = torch.nn.functional.interpolate(t, size=dst, mode="bicubic", antialias=True, align_corners=False)
    want = want.permute(0, 2, 3, 1).reshape(dst[0] * dst[1], 8).numpy()
    got = ni.resample_grid(x, src, dst)
    err = float(np.abs(got - want).max())
    print(f"[image] {src} -> {dst}: restatement vs F.interpolate fp64, max |diff| {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("g", [(4, 4), (3, 5), (37, 37)])
def test_equal_grids_have_weights_of_exactly_zero_and_one(g):
    for n in g:
        assert np.array_equal(ni.axis_matrix(n, n), np.eye(n))
    x = _source(g, 8)
    assert np.array_equal(ni.resample_grid(x, g, g), x)
    pos = np.concatenate([np.full((3, 8), 7.0), x])
    assert np.array_equal(ni.resample_pos_embed(pos, g, g, 3), pos)


def test_prefix_rows_pass_through_the_restatement():
    x = _source((4, 4), 8)
    pos = np.concatenate([np.arange(40.0).reshape(5, 8), x])
    out = ni.resample_pos_embed(pos, (4, 4), (5, 3), 5)
    assert out.shape == (5 + 15, 8) and np.array_equal(out[:5], pos[:5])
    assert np.array_equal(out[5:], ni.resample_grid(x, (4, 4), (5, 3)))


# ---- 2. the budget holds the kernel's own order with room to spare -------------------------------------------------------------

@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("src, dst", SHAPES)
def test_the_emulation_uses_at_most_half_the_budget(src, dst, dt):
    """tests/test_score_tiled_cpu.py's discipline: the fp32 emulation of the kernel's order uses at most HALF of the allowance
    for the fp32 arithmetic before the output rounding (that rounding may take all of its own term: it is exact, not estimated),
    and its rounded result sits inside the whole budget"""
    x = nm.round_to(_source(src, 8, seed=1), dt)
    want, budget = ni.resample_budget(x, src, dst, dt)
    raw = ni.emul_resample(x, src, dst, dt, rounded=False)
    part = budget - nm.UNIT[dt] * np.abs(want) - nm.FLOOR[dt]
    r32 = float((np.abs(raw.astype(np.float64) - want) / part).max())
    ratio, _ = nm.worst_ratio(nm.round_to(raw, dt), want, budget)
    print(f"[image] {src} -> {dst} {dt}: fp32 part of the emulation {r32:.3f} of its allowance; rounded, err / budget {ratio:.3f}")
    assert r32 <= 0.5 and ratio <= 1.0


@pytest.mark.parametrize("src, dst", [((37, 37), (16, 16)), ((16, 16), (37, 37)), ((4, 4), (5, 3))])
def test_the_budget_can_tell_the_neighbouring_rules_apart(src, dst, monkeypatch):
    """the interpolations a resample could be mistaken for leave the budget, in bf16 already: bicubic without antialiasing
    (down-sampling only: up-sampling has no antialiasing to lose), torch's own a = -0.75 cubic, and bilinear"""
    x = nm.round_to(_source(src, 8, seed=2), "bf16")
    want, budget = ni.resample_budget(x, src, dst, "bf16")
    t = torch.from_numpy(x.astype(np.float64)).reshape(1, src[0], src[1], 8).permute(0, 3, 1, 2)
    back = lambda y: nm.round_to(y.permute(0, 2, 3, 1).reshape(dst[0] * dst[1], 8).numpy(), "bf16")
    mutants = {"bilinear, antialias": back(torch.nn.functional.interpolate(t, size=dst, mode="bilinear", antialias=True))}
    if src[0] > dst[0]:
        mutants["bicubic, no antialias"] = back(torch.nn.functional.interpolate(t, size=dst, mode="bicubic", antialias=False))
    monkeypatch.setattr(ni, "A", -0.75)
    mutants["a = -0.75"] = nm.round_to(ni.resample_grid(x, src, dst), "bf16")
    for what, got in mutants.items():
        ratio, _ = nm.worst_ratio(got, want, budget)
        print(f"[image] {src} -> {dst} mutant '{what}': err / budget {ratio:.1f}")
        assert ratio > 1.0, what


# ---- 3. pins -----------------------------------------------------------------------------------------------------------------

def test_the_image_header_is_additive_and_nothing_else_moves():
    assert nat.IMAGE_SYMBOLS == IMAGE_SYMBOLS
    header = open(os.path.join(ROOT, "include", "rajni_hip_image.h")).read()
    assert set(re.findall(r"\b(rajni_[a-z0-9_]+)\s*\(", header)) - {"rajni_stream_t"} == set(IMAGE_SYMBOLS)
    lib = nat.lib()
    for s in IMAGE_SYMBOLS:
        assert getattr(lib, s) is not None
    assert C.sizeof(nat.VitImage) == 8 and [f[0] for f in nat.VitImage._fields_] == ["height", "width"]
    assert re.search(r"typedef struct \{\s*int height, width;[^}]*\} rajni_vit_image;", header)
    # the old counts, sizes and versions
    assert lib.rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    assert len(nat.EXPORTED_SYMBOLS) == 45 and nat.LAYERS_SYMBOLS == ("rajni_vit_forward_layers",)
    assert not set(IMAGE_SYMBOLS) & (set(nat.EXPORTED_SYMBOLS) | set(nat.LAYERS_SYMBOLS))
    assert C.sizeof(nat.VitExt) == 72 and C.sizeof(nat.VitPrefix) == 16 and C.sizeof(nat.VitLayers) == 40
    main = open(os.path.join(ROOT, "include", "rajni_hip.h")).read()
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", main) and re.search(r"RAJNI_NUM_KCLASS\s*=\s*17\b", main)
    for h in ("rajni_hip.h", "rajni_hip_debug.h", "rajni_hip_layers.h"):
        assert "rajni_vit_image" not in open(os.path.join(ROOT, "include", h)).read()
    assert lib.rajni_profile_class_name(17) == b"" and lib.rajni_profile_class_name(16) != b""


def test_the_square_size_queries_are_what_the_image_ones_say_for_a_square():
    lib = nat.lib()
    for dt in (nat.RAJNI_BF16, nat.RAJNI_F32):
        for S, P in ((64, 16), (56, 14), (70, 10)):
            assert lib.rajni_patch_embed_workspace_bytes_image(3, 3, S, S, P, dt) == lib.rajni_patch_embed_workspace_bytes(3, 3, S, P, dt)
    assert lib.rajni_patch_embed_workspace_bytes_image(2, 3, 48, 96, 16, nat.RAJNI_BF16) == 0          # fused loader
    assert lib.rajni_patch_embed_workspace_bytes_image(2, 3, 42, 70, 14, nat.RAJNI_BF16) == 2 * 15 * 640 * 2
    assert lib.rajni_patch_embed_workspace_bytes_image(2, 3, 70, 42, 14, nat.RAJNI_F32) == 2 * 15 * 640 * 4
    assert lib.rajni_patch_embed_workspace_bytes_image(2, 3, 42, 71, 14, nat.RAJNI_BF16) == 0          # not a multiple: refused at the call
    p, keep = _plan()
    sq, none = nat.VitImage(64, 64), None
    base = lib.rajni_vit_workspace_bytes_prefix(C.byref(p), None)
    assert lib.rajni_vit_workspace_bytes_image(C.byref(p), None, C.byref(sq)) == base == lib.rajni_vit_workspace_bytes_image(C.byref(p), None, none)
    wide = nat.VitImage(64, 128)
    assert lib.rajni_vit_workspace_bytes_image(C.byref(p), None, C.byref(wide)) > base
    del keep


# ---- 4. refusals of the image record -----------------------------------------------------------------------------------------

def _forward_image(p, img, ext=None, prefix=None, layers=None):
    lib = nat.lib()
    ref = lambda r: C.byref(r) if r is not None else None
    rc = lib.rajni_vit_forward_image(C.byref(p), ref(ext), ref(prefix), ref(layers), ref(img), IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _reaches_the_workspace_check(p, img, **kw):
    rc, msg = _forward_image(p, img, **kw)
    assert rc == ERR_INVALID and "workspace too small" in msg, (rc, msg)
    return int(re.search(r"< (\d+)\)", msg).group(1))


def test_a_clean_record_a_square_record_and_no_record_reach_the_workspace_check():
    p, keep = _plan(keeps=(0, 8, 6, 0), buffers=(1, 2))
    none = _reaches_the_workspace_check(p, None)
    assert _reaches_the_workspace_check(p, nat.VitImage(64, 64)) == none
    p.img_size = 48
    need = _reaches_the_workspace_check(p, nat.VitImage(48, 96))              # 3 x 6 = 18 patch tokens: keep 8 and 6 still fit
    assert need == nat.lib().rajni_vit_workspace_bytes_image(C.byref(p), None, C.byref(nat.VitImage(48, 96))) > none
    _reaches_the_workspace_check(p, nat.VitImage(48, 96), ext=_ext(nat.POOL_DENSE), prefix=nat.VitPrefix(5, FAKE))
    del keep


def test_the_schedule_is_checked_against_the_records_grid():
    p, keep = _plan(keeps=(0, 8, 6, 0), buffers=(1, 2))
    p.img_size = 32
    rc, msg = _forward_image(p, nat.VitImage(32, 48))                        # 2 x 3 = 6 patch tokens, keep = 8
    assert rc == ERR_INVALID and "keep=8 but only 6 patch tokens" in msg, msg
    del keep


@pytest.mark.parametrize("h, w", [(0, 64), (64, 0), (-16, 64), (64, -16), (72, 64), (64, 72), (8, 8)])
def test_sizes_that_are_no_positive_multiple_of_the_patch_are_refused(h, w):
    p, keep = _plan()
    p.img_size = h
    rc, msg = _forward_image(p, nat.VitImage(h, w))
    assert rc == ERR_INVALID and "positive multiples of the patch size 16" in msg and f"({h} x {w})" in msg, (rc, msg)
    assert nat.lib().rajni_vit_workspace_bytes_image(C.byref(p), None, C.byref(nat.VitImage(h, w))) == 0
    del keep


def test_the_plans_image_size_must_be_the_records_height():
    p, keep = _plan()
    rc, msg = _forward_image(p, nat.VitImage(48, 96))
    assert rc == ERR_INVALID and "plan.img_size must equal image.height (64 != 48)" in msg, (rc, msg)
    rc, msg = _forward_image(p, nat.VitImage(96, 64))                         # the width is not the height
    assert rc == ERR_INVALID and "(64 != 96)" in msg, (rc, msg)
    del keep


def test_more_tokens_than_the_cap_are_refused_in_the_existing_wording():
    p, keep = _plan(keeps=(0, 0, 0, 0), buffers=())
    p.img_size = 2048
    _reaches_the_workspace_check(p, nat.VitImage(2048, 2048))                 # 16384 + 1 tokens: the cap holds them
    _reaches_the_workspace_check(p, nat.VitImage(2048, 2048), prefix=nat.VitPrefix(32, FAKE))      # 16416
    rc, msg = _forward_image(p, nat.VitImage(2048, 2064))
    assert rc == ERR_UNSUPPORTED and "is beyond the tiled path's cap of 16416 tokens" in msg and "N=16513" in msg, (rc, msg)
    del keep


def test_the_record_is_refused_before_the_other_records_and_the_plan():
    """in front of every other refusal: a bad layers record, a bad plan and a bad ext record do not get a word in"""
    p, keep = _plan()
    p.C = 100                                                                  # check_plan would refuse
    lay = nat.VitLayers()
    lay.n = 0                                                                  # check_layers would refuse
    rc, msg = _forward_image(p, nat.VitImage(64, 72), ext=_ext(pool=4), layers=lay)
    assert rc == ERR_INVALID and "positive multiples of the patch size" in msg, (rc, msg)
    rc, msg = _forward_image(p, nat.VitImage(64, 64), layers=lay)
    assert rc == ERR_INVALID and "layers.n must be" in msg, (rc, msg)
    del keep


def test_resample_refusals_state_the_cap():
    lib = nat.lib()
    for grids in ((129, 4, 4, 4), (4, 129, 4, 4), (4, 4, 129, 4), (4, 4, 4, 129), (0, 4, 4, 4), (4, 4, 4, 0)):
        rc = lib.rajni_resample_pos_embed(FAKE, grids[0], grids[1], FAKE, grids[2], grids[3], 64, 1, nat.RAJNI_BF16, None)
        assert rc == ERR_UNSUPPORTED and "1..128 per axis" in lib.rajni_last_error().decode(), lib.rajni_last_error()
    assert lib.rajni_resample_pos_embed(FAKE, 4, 4, FAKE, 5, 3, 60, 1, nat.RAJNI_BF16, None) == ERR_UNSUPPORTED
    assert b"C % 8 == 0" in lib.rajni_last_error()
    assert lib.rajni_resample_pos_embed(FAKE, 4, 4, FAKE, 5, 3, 64, 33, nat.RAJNI_BF16, None) == ERR_INVALID
    assert lib.rajni_resample_pos_embed(FAKE, 4, 4, FAKE, 5, 3, 64, -1, nat.RAJNI_BF16, None) == ERR_INVALID
    assert lib.rajni_resample_pos_embed(FAKE, 4, 4, FAKE, 5, 3, 64, 1, 7, None) == ERR_INVALID
    assert lib.rajni_resample_pos_embed(FAKE + 8, 4, 4, FAKE, 5, 3, 64, 1, nat.RAJNI_BF16, None) == ERR_INVALID
    assert b"src must be 16-byte aligned" in lib.rajni_last_error()
    assert lib.rajni_resample_pos_embed(FAKE, 4, 4, FAKE + 4, 5, 3, 64, 1, nat.RAJNI_F32, None) == ERR_INVALID
    assert b"dst must be 16-byte aligned" in lib.rajni_last_error()
    assert lib.rajni_resample_pos_embed(None, 4, 4, FAKE, 5, 3, 64, 1, nat.RAJNI_BF16, None) == ERR_INVALID


def test_patch_embed_image_refusals():
    lib = nat.lib()
    call = lambda H, W, P=16, npre=1, reg=None, ws=None, nws=0: lib.rajni_patch_embed_image(
        FAKE, FAKE, FAKE, FAKE, reg, npre, FAKE, 1, FAKE, 0, 2, 3, H, W, P, 64, nat.RAJNI_BF16, ws, nws, None)
    for H, W in ((48, 100), (50, 96), (0, 96), (48, 0)):
        assert call(H, W) == ERR_INVALID and b"the patch size must divide the image" in lib.rajni_last_error()
    assert call(42, 70, P=14) == ERR_INVALID and b"column workspace" in lib.rajni_last_error()        # H x W parsed, workspace missing
    assert call(48, 96, npre=5) == ERR_INVALID and b"reg is null" in lib.rajni_last_error()
    assert call(48, 96, npre=0) == ERR_INVALID


# ---- 5. the wrapper ------------------------------------------------------------------------------------------------------------

def _wrapped(name="vit_micro_patch16_64", **attrs):
    m = ts.create_model(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    return rajni_amd.RAJNIViTWrapper(m, {})


def test_the_setter_returns_self_drops_plans_and_follows_the_base_model():
    w = _wrapped()
    assert w.dynamic_img_size is False
    w._plan, w._plans = ("stale",), {"k": 1}
    assert w.set_dynamic_img_size() is w and w.dynamic_img_size is True and w._plan is None and w._plans == {}
    assert w.set_dynamic_img_size(False).dynamic_img_size is False
    assert _wrapped(dynamic_img_size=True).dynamic_img_size is True
    assert _wrapped(dynamic_img_size=False).dynamic_img_size is False


def test_the_source_grid_rule():
    w = _wrapped()
    assert w._pos_source_grid(17, 1) == (1, (4, 4))                       # a class row + 4 x 4
    assert w._pos_source_grid(16, 1) == (0, (4, 4))                       # no_embed_class
    assert w._pos_source_grid(5 + 37 * 37, 5) == (5, (37, 37))            # registers
    assert w._pos_source_grid(37 * 37, 5) == (0, (37, 37))
    w.m.patch_embed.grid_size = (3, 5)
    assert w._pos_source_grid(16, 1) == (1, (3, 5))                       # grid_size names a 15-row embedding behind the class row
    assert w._pos_source_grid(15, 1) == (0, (3, 5))
    assert w._pos_source_grid(17, 1) == (1, (4, 4))                       # its product is not the count: the square root
    w.m.patch_embed.grid_size = None
    assert w._pos_source_grid(16, 2) == (0, (4, 4))                       # 14 is no square, 16 is: an embedding without prefix rows
    with pytest.raises(NotImplementedError, match="cannot tell the grid of a pos_embed of 15 rows"):
        w._pos_source_grid(15, 1)                                          # 14 and 15: a non-square count and no grid_size
    w.m.patch_embed.grid_size = (3, "5")
    with pytest.raises(NotImplementedError, match="not square"):
        w._pos_source_grid(13, 1)                                          # 12 and 13: neither is a square, grid_size is no pair of ints


def test_a_model_with_a_3_by_5_grid_and_a_15_row_embedding_is_recognised():
    m = ts.create_model("vit_micro_patch16_64")
    m.patch_embed.grid_size = (3, 5)
    m.pos_embed = torch.nn.Parameter(torch.randn(1, 16, 128))
    w = rajni_amd.RAJNIViTWrapper(m, {}).set_dynamic_img_size()
    assert w._pos_source_grid(m.pos_embed.shape[1], 1) == (1, (3, 5))
    m.pos_embed = torch.nn.Parameter(torch.randn(1, 15, 128))             # non-square count, and now no grid_size either
    m.patch_embed.grid_size = None
    with pytest.raises(NotImplementedError, match="15 rows"):
        w._pos_source_grid(15, 1)


def test_off_mode_errors_keep_their_text_and_name_the_setter():
    w = _wrapped()
    with pytest.raises(ValueError) as e:
        w._check_input_shape(torch.zeros(2, 3, 48, 96))
    assert str(e.value).startswith("expected images [B, C, S, S], got (2, 3, 48, 96)") and "set_dynamic_img_size" in str(e.value)
    w._check_input_shape(torch.zeros(2, 3, 48, 48))
    with pytest.raises(ValueError) as e:
        w._build_plan(2, 96, torch.device("cpu"), torch.float32)
    assert str(e.value).startswith("pos_embed has 17 rows but the input yields 37 tokens (1 of them prefix tokens)")
    assert "set_dynamic_img_size" in str(e.value)
    with pytest.raises(ValueError, match="image size 40 is not a multiple of the patch size 16"):
        w._build_plan(2, 40, torch.device("cpu"), torch.float32)
    w.set_dynamic_img_size()
    w._check_input_shape(torch.zeros(2, 3, 48, 96))
    with pytest.raises(ValueError, match=r"expected images \[B, C, S, S\], got \(3, 48, 96\)"):
        w._check_input_shape(torch.zeros(3, 48, 96))
    with pytest.raises(ValueError, match="is not a multiple of the patch size 16"):
        w._build_plan(2, (48, 100), torch.device("cpu"), torch.float32)
    m = ts.create_model("vit_micro_patch16_64")
    m.dynamic_img_size, m.dynamic_img_pad = True, True
    with pytest.raises(NotImplementedError, match="dynamic_img_pad"):
        rajni_amd.RAJNIViTWrapper(m, {})._build_plan(2, (48, 96), torch.device("cpu"), torch.float32)


# ---- 6. the forward fixtures can tell ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, size, dt, fmt", ni.FORWARD_CASES)
def test_wrong_embeddings_move_the_logits_by_five_times_the_bar(name, size, dt, fmt):
    for how, (moved, need) in ni.wrong_answers_move(name, size, dt, fmt).items():
        print(f"[image] {name} {size[0]}x{size[1]} {dt} {fmt}: the {how} embedding moves the logits by {moved:.4g} = "
              f"{5 * moved / need:.1f}x the bar (need 5x)")
        assert moved >= need, (how, moved, need)


def test_cli_flags():
    from rajni_amd import run
    d = run.get_args([])
    assert d.img_size is None and d.dynamic_img_size is False
    a = run.get_args(["--img_size", "48", "96", "--dynamic_img_size"])
    assert a.img_size == [48, 96] and a.dynamic_img_size is True
    assert run.get_args(["--img_size", "96"]).img_size == [96]
    with pytest.raises(SystemExit):
        run.get_args(["--img_size", "1", "2", "3"])
    assert tuple(run.SyntheticLoader(1, 2, (48, 96), "cpu", torch.float32, 0).images.shape) == (2, 3, 48, 96)
    assert tuple(run.SyntheticLoader(1, 2, 32, "cpu", torch.float32, 0).images.shape) == (2, 3, 32, 32)
