"""Any input size on the device (include/rajni_hip_image.h): the position-embedding resample kernel, the patch embedding of
H x W images, the forward with an image record, and the wrapper's dynamic_img_size.  GPU box only (`-m gpu`).

Yardsticks, never the code under test:
  resample      tests/numerics_image.py's fp64 restatement of timm's resample_abs_pos_embed (shown equal to torch's own
                bicubic-antialias interpolation in tests/test_image_size_cpu.py), inside its per-element budget;
  patch embed   oracle.patch_embed in fp64 at tests/test_gpu_kernels.py::test_patch_embed's tolerances (1e-2 of the scale into a
                16-bit stream, 1e-5 into the fp32 stream of a 16-bit model; 3e-6 for fp32, tests/test_gpu_fp32.py);
  forwards      the restated pruned graphs (tests/numerics_prefix.py, numerics_distilled.py, oracle.vit_forward) on the H x W images
                with the fp64-resampled embedding, their selections injected; bars 1e-2 x max|logit| for 16-bit models, 1e-3 for
                fp32, and tests/test_gpu_fp8_mfma.py's own check for the fp8_mfma format.  tests/test_image_size_cpu.py shows for
                every one of these fixtures that the transposed grid and the un-resampled embedding move the logits by >= 5x the bar.
Identity claims (a NULL record, a square record, a square `size=`, the cache) are bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm
import numerics_image as ni
import rajni_amd
from guarded import Guarded
from oracle import rajni_oracle as orc
from rajni_amd import _native as nat
from rajni_amd import ops
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = nm.TORCH


def lib():
    return nat.lib()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def close(got, want, rel, what):
    scale, err = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"[image] {what}: max |diff| {err:.4g} (scale {scale:.4g}, bar {rel * scale:.4g})")
    assert err <= rel * scale, f"{what}: max |diff| {err:.4g} vs scale {scale:.4g}"


# ---- 1. the resample kernel ------------------------------------------------------------------------------------------------------

def pos_case(src, C_, prefix, dt, seed=0):
    """[prefix + sh * sw, C] values of type dt: patch rows standard normal over three decades of row scale; prefix rows with the
    bit patterns a copy must keep and arithmetic would not (-0, a denormal, inf)"""
    rng = np.random.default_rng([seed, src[0], src[1], C_, prefix])
    rows = rng.standard_normal((src[0] * src[1], C_)) * 10.0 ** rng.uniform(-2, 1, size=(src[0] * src[1], 1))
    pre = rng.standard_normal((prefix, C_))
    if prefix:
        pre[0, :4] = [-0.0, np.inf, -np.inf, 1e-39]
    return nm.round_to(np.concatenate([pre, rows]), dt)


def run_resample(pos, src, dst, prefix, dt, misalign=0):
    """the kernel on guarded buffers (tests/guarded.py): guards of both intact, every output element written, src unchanged"""
    align = 16 if misalign else 256
    t = torch.from_numpy(pos).to(TORCH[dt])
    sg = Guarded(tuple(t.shape), TORCH[dt], DEV, misalign=misalign, align=align).fill_(t)
    dg = Guarded((prefix + dst[0] * dst[1], t.shape[1]), TORCH[dt], DEV, misalign=misalign, align=align)
    if misalign:
        assert sg.ptr() % 256 == misalign and dg.ptr() % 256 == misalign
    nat.check(lib().rajni_resample_pos_embed(sg.ptr(), src[0], src[1], dg.ptr(), dst[0], dst[1], t.shape[1], prefix,
                                             nat.dtype_code(TORCH[dt]), nat.stream_ptr()), "rajni_resample_pos_embed")
    torch.cuda.synchronize()
    dg.check(f"resample dst {src} -> {dst} {dt}")
    sg.check(f"resample src {src} -> {dst} {dt}", written=False)
    assert same_bytes(sg.t.cpu(), t), "the source was written"
    return dg.t.clone()


RESAMPLE_CASES = [((4, 4), (5, 3), 128, 1, "bf16"), ((4, 4), (2, 6), 128, 0, "fp16"), ((3, 5), (1, 1), 64, 5, "fp32"),
                  ((37, 37), (16, 16), 384, 5, "bf16"), ((16, 16), (37, 37), 384, 0, "fp32")]


@pytest.mark.parametrize("src, dst, C_, prefix, dt", RESAMPLE_CASES)
def test_resample_kernel_against_the_restatement(src, dst, C_, prefix, dt):
    pos = pos_case(src, C_, prefix, dt)
    got = run_resample(pos, src, dst, prefix, dt)
    assert same_bytes(got[:prefix].cpu(), torch.from_numpy(pos[:prefix]).to(TORCH[dt])), "prefix rows are copied bit for bit"
    want, budget = ni.resample_budget(pos[prefix:], src, dst, dt)
    nm.assert_within(got[prefix:].float().cpu().numpy(), want, budget, f"resample {src} -> {dst} C={C_} {dt}")
    assert same_bytes(run_resample(pos, src, dst, prefix, dt), got), "two runs differ"


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_resample_to_the_same_grid_returns_the_sources_bits(dt):
    pos = pos_case((4, 4), 128, 2, dt, seed=1)
    pos[5, :3] = [-0.0, np.inf, 1e-39]                       # a patch row too: the weights are exactly 0 and 1, and 0 * inf is not 0
    pos = nm.round_to(pos, dt)
    got = run_resample(pos, (4, 4), (4, 4), 2, dt)
    assert same_bytes(got.cpu(), torch.from_numpy(pos).to(TORCH[dt]))
    assert same_bytes(ops.resample_pos_embed(torch.from_numpy(pos).to(TORCH[dt]).to(DEV), (4, 4), (4, 4), 2), got)


@pytest.mark.parametrize("src, dst, C_, prefix, dt", [((4, 4), (5, 3), 128, 1, "bf16"), ((4, 4), (3, 2), 72, 3, "fp32")])
def test_resample_at_sixteen_byte_alignment(src, dst, C_, prefix, dt):
    """src and dst 16 bytes past a 256-byte boundary - the ABI's minimum - give the bits of the 256-byte aligned call"""
    pos = pos_case(src, C_, prefix, dt, seed=2)
    assert same_bytes(run_resample(pos, src, dst, prefix, dt, misalign=16), run_resample(pos, src, dst, prefix, dt))


def test_ops_resample_binds_the_entry_point():
    pos = torch.from_numpy(pos_case((4, 4), 128, 1, "bf16", seed=3)).to(torch.bfloat16).to(DEV)
    got = ops.resample_pos_embed(pos, (4, 4), (5, 3), prefix_rows=1)
    assert got.shape == (16, 128) and got.dtype == torch.bfloat16
    assert same_bytes(got, run_resample(pos.float().cpu().numpy(), (4, 4), (5, 3), 1, "bf16"))
    out = torch.empty_like(got)
    assert ops.resample_pos_embed(pos, (4, 4), (5, 3), 1, out=out) is out and same_bytes(out, got)
    with pytest.raises(ValueError, match="pos must be"):
        ops.resample_pos_embed(pos, (4, 5), (5, 3), 1)
    with pytest.raises(NotImplementedError, match="1..128 per axis"):
        ops.resample_pos_embed(pos, (4, 4), (129, 3), 1)


# ---- 2. the patch embedding of H x W images ----------------------------------------------------------------------------------------

def embed_case(H, W, P, Cc, B, dt, regs, seed):
    rng = np.random.default_rng([seed, H, W, P])
    r = lambda a: nm.round_to(a, dt)
    img = r(rng.standard_normal((B, 3, H, W), dtype=np.float32))
    w = r(rng.standard_normal((Cc, 3, P, P), dtype=np.float32) * 0.05)
    b = r(rng.standard_normal(Cc, dtype=np.float32) * 0.1)
    cls = r(rng.standard_normal(Cc, dtype=np.float32))
    reg = r(rng.standard_normal((regs, Cc), dtype=np.float32)) if regs else None
    pos = r(rng.standard_normal(((H // P) * (W // P) + 1 + regs, Cc), dtype=np.float32))
    return img, w, b, cls, reg, pos


def embed(img, w, b, cls, reg, pos, P, dt, out_f32, size):
    d = lambda a: None if a is None else torch.from_numpy(a).to(TORCH[dt]).to(DEV)
    Cc = w.shape[0]
    return ops.patch_embed(d(img), ops.pack_weight(d(w), TORCH[dt], k_multiple=64), torch.from_numpy(b).to(DEV), d(cls), d(pos), True,
                           P, Cc, out_f32=out_f32, reg=d(reg), size=size)


def embed_want(img, w, b, cls, reg, pos):
    tok = orc.patch_embed(img.astype(np.float64), w.astype(np.float64), b.astype(np.float64))
    B, Cc = img.shape[0], w.shape[0]
    prefix = [np.broadcast_to(cls, (B, 1, Cc))] + ([np.broadcast_to(reg, (B,) + reg.shape)] if reg is not None else [])
    return np.concatenate(prefix + [tok], axis=1) + pos[None]


@pytest.mark.parametrize("H, W, P, dt, regs, out_f32", [
    (48, 96, 16, "bf16", 0, False), (48, 96, 16, "bf16", 0, True), (96, 48, 16, "bf16", 4, False), (96, 48, 16, "bf16", 4, True),
    (16, 32, 16, "bf16", 0, False), (16, 32, 16, "bf16", 4, True), (32, 48, 16, "fp32", 0, True),         # the fused loader
    (42, 70, 14, "bf16", 0, False), (42, 70, 14, "bf16", 4, True), (14, 28, 14, "bf16", 0, False), (14, 28, 14, "bf16", 0, True)])
def test_patch_embed_of_rectangular_images(H, W, P, dt, regs, out_f32):
    B, Cc = 3, 128
    nbytes = lib().rajni_patch_embed_workspace_bytes_image(B, 3, H, W, P, nat.dtype_code(TORCH[dt]))
    assert (nbytes == 0) == (P == 16), "patch 16 is the fused loader, patch 14 the column matrix"
    case = embed_case(H, W, P, Cc, B, dt, regs, seed=1)
    x = embed(*case, P, dt, out_f32, (H, W))
    assert x.shape == (B, 1 + regs + (H // P) * (W // P), Cc)
    rel = 3e-6 if dt == "fp32" else (1e-5 if out_f32 else 1e-2)
    got, want = x.float().cpu().numpy().astype(np.float64), embed_want(*case)
    close(got, want, rel, f"patch embed {H}x{W} p{P} {dt} regs={regs} out_f32={out_f32}")
    # an H / W swap must not pass: the same bytes read as [B, 3, W, H] are another image, many bars away
    img = case[0]
    swapped = embed_want(img.reshape(B, 3, W, H), *case[1:])
    assert swapped.shape == want.shape
    assert float(np.abs(got - swapped).max()) > 10 * rel * float(np.abs(want).max()), "the test cannot tell H x W from W x H"


@pytest.mark.parametrize("S, P, dt, regs, out_f32", [(64, 16, "bf16", 0, False), (64, 16, "bf16", 4, True), (56, 14, "bf16", 0, True),
                                                      (32, 16, "fp32", 0, True), (56, 14, "fp16", 4, False)])
def test_a_square_size_gives_the_bits_of_the_square_entry_point(S, P, dt, regs, out_f32):
    case = embed_case(S, S, P, 128, 3, dt, regs, seed=2)
    assert same_bytes(embed(*case, P, dt, out_f32, (S, S)), embed(*case, P, dt, out_f32, None))


def test_patch_embed_size_must_be_the_images():
    case = embed_case(48, 96, 16, 128, 2, "bf16", 0, seed=3)
    with pytest.raises(ValueError, match="size="):
        embed(*case, 16, "bf16", False, (96, 48))
    with pytest.raises(ValueError, match="pass size="):
        embed(*case, 16, "bf16", False, None)


# ---- 3. the forward with a NULL record and with a square one ---------------------------------------------------------------------

def plan_of(name, fmt="model", layers=False):
    """(wrapper, plan entry, images) after one forward of the wrapper: the plan, records and weights it built"""
    w = rajni_amd.RAJNIViTWrapper(ni.build_model(name), ni.SCHED).to(DEV).to(torch.bfloat16).eval().set_weight_format(fmt)
    x = torch.from_numpy(ni.images_of((64, 64))).to(DEV).to(torch.bfloat16)
    if layers:
        w.forward_intermediates(x, indices=[1, 3], norm=True, fill="last", intermediates_only=True)
    else:
        w(x)
    return w, w._plan, x


@pytest.mark.parametrize("name, fmt, layers", [("vit_micro_patch16_64", "model", False), ("vit_micro_reg4_patch16_64", "model", False),
                                               ("vit_micro512_patch16_64", "fp8", True)])
def test_a_null_record_and_a_square_record_are_the_existing_entry_point(name, fmt, layers):
    w, entry, x = plan_of(name, fmt, layers)
    plan, ext, pre = entry[1], entry[2][4], entry[2][6]
    assert (pre is not None) == ("reg4" in name) and plan.img_size == 64
    ref = lambda r: C.byref(r) if r is not None else None

    def records():
        out = torch.full(entry[6], float("nan"), dtype=torch.bfloat16, device=DEV)
        lay = slabs = None
        if layers:
            cap_arr, lnorm, lfill, slab_shape = entry[7]
            slabs = torch.full(slab_shape, float("nan"), dtype=torch.bfloat16, device=DEV)
            lay = nat.VitLayers()
            lay.n, lay.blocks, lay.norm, lay.fill, lay.out, lay.slab_stride = len(cap_arr), cap_arr, lnorm, lfill, slabs.data_ptr(), 0
        return out, lay, slabs

    def existing():
        out, lay, slabs = records()
        if layers:
            rc = lib().rajni_vit_forward_layers(C.byref(plan), ref(ext), ref(pre), C.byref(lay), x.data_ptr(), out.data_ptr(), nat.stream_ptr())
        elif pre is not None:
            rc = lib().rajni_vit_forward_ext_prefix(C.byref(plan), ref(ext), C.byref(pre), x.data_ptr(), out.data_ptr(), nat.stream_ptr())
        else:
            assert ext is None
            rc = lib().rajni_vit_forward(C.byref(plan), x.data_ptr(), out.data_ptr(), nat.stream_ptr())
        nat.check(rc, "existing entry point")
        torch.cuda.synchronize()
        return out, slabs

    def with_record(img):
        out, lay, slabs = records()
        nat.check(lib().rajni_vit_forward_image(C.byref(plan), ref(ext), ref(pre), ref(lay), ref(img), x.data_ptr(), out.data_ptr(),
                                                nat.stream_ptr()), "rajni_vit_forward_image")
        torch.cuda.synchronize()
        return out, slabs

    want, want_slabs = existing()
    assert not bool(torch.isnan(want[:, :plan.num_classes].float()).any())
    for img in (None, nat.VitImage(64, 64)):
        got, got_slabs = with_record(img)
        assert same_bytes(got, want), f"record {img and (img.height, img.width)}: the output differs"
        if layers:
            assert same_bytes(got_slabs, want_slabs) and not bool(torch.isnan(want_slabs.float()).any())
    sq = nat.VitImage(64, 64)
    assert (lib().rajni_vit_workspace_bytes_image(C.byref(plan), ref(pre), C.byref(sq)) == plan.workspace_bytes
            == lib().rajni_vit_workspace_bytes_image(C.byref(plan), ref(pre), None))


# ---- 4. forwards at new sizes -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture(name):
    """(config, fp32 state dict of the fixture with bf16-representable values) - built once, never modified"""
    return ts.CONFIGS[name], ts.state_dict_numpy(ni.build_model(name))


@functools.lru_cache(maxsize=None)
def yardstick(name, size, dt):
    """the restated graph on the resampled embedding (as the model dtype holds it), free-running in fp64: computed once"""
    cfg, sd = fixture(name)
    grid = (size[0] // cfg.patch_size, size[1] // cfg.patch_size)
    return ni.restated_logits(name, ni.sd_at_grid(sd, cfg, grid, dt=dt), ni.images_of(size))


def wrapped(name, dt, sched=None):
    return rajni_amd.RAJNIViTWrapper(ni.build_model(name), ni.SCHED if sched is None else sched).to(DEV).to(TORCH[dt]).eval()


@pytest.mark.parametrize("name, size, dt, fmt", [c for c in ni.FORWARD_CASES if c[3] == "model"])
def test_forward_at_a_new_size(name, size, dt, fmt):
    cfg, _ = fixture(name)
    P, (gh, gw) = cfg.num_prefix_tokens, (size[0] // cfg.patch_size, size[1] // cfg.patch_size)
    want, counts, tr = yardstick(name, size, dt)
    assert counts[0] == P + gh * gw
    w = wrapped(name, dt).set_dynamic_img_size()
    x = torch.from_numpy(ni.images_of(size)).to(DEV)
    w.force_keep_idx({i: torch.from_numpy(t["keep_idx"]).to(DEV) for i, t in tr.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts
    close(got, want, ni.BAR[dt], f"{name} {size[0]}x{size[1]} {dt}, selections injected")
    assert np.array_equal(w(x).float().cpu().numpy(), got)


def test_with_the_setter_off_new_sizes_are_refused_as_before():
    w = wrapped("vit_micro_patch16_64", "bf16")
    with pytest.raises(ValueError, match=r"expected images \[B, C, S, S\], got \(3, 3, 48, 96\)"):
        w(torch.from_numpy(ni.images_of((48, 96))).to(DEV))
    with pytest.raises(ValueError, match="pos_embed has 17 rows but the input yields 37 tokens"):
        w(torch.from_numpy(ni.images_of((96, 96))).to(DEV))
    w.set_dynamic_img_size()
    with pytest.raises(ValueError, match="is not a multiple of the patch size 16"):
        w(torch.zeros(2, 3, 48, 100, device=DEV))
    assert w(torch.from_numpy(ni.images_of((96, 96))).to(DEV)).shape[0] == ni.BATCH


def test_forward_at_a_new_size_fp8_mfma():
    """tests/test_gpu_fp8_mfma.py's check, at 48 x 96: the oracle with the device's dequantised weights and the activation rule,
    its selections injected"""
    from test_gpu_fp8_mfma import _check_against_rule
    (name, size, dt, fmt), = [c for c in ni.FORWARD_CASES if c[3] == "fp8_mfma"]
    cfg = ts.CONFIGS[name]
    model = ni.build_model(name)
    w = rajni_amd.RAJNIViTWrapper(model, ni.SCHED).to(DEV).to(torch.bfloat16).eval().set_weight_format(fmt).set_dynamic_img_size()
    imgs = ni.images_of(size)
    x = torch.from_numpy(imgs).to(DEV)
    w(x)                                                     # packs the weights: dequantized_state_dict needs them
    sd = ts.state_dict_numpy(ni.build_model(name))
    sd.update({k: v.cpu().numpy() for k, v in w.dequantized_state_dict().items()})
    sd = ni.sd_at_grid(sd, cfg, (size[0] // 16, size[1] // 16), dt=dt)
    with_act, counts, tr = ni.restated_logits(name, sd, imgs, act_fp8=True)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    weights_only, _ = orc.vit_forward(sd, imgs, ni.SCHED, depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps, forced_keep=forced)
    w.force_keep_idx({i: torch.from_numpy(np.asarray(k)).to(DEV) for i, k in forced.items()})
    got = w(x).float().cpu().numpy()
    assert w.get_last_stats()["token_counts"] == counts and counts[0] == 19
    assert np.array_equal(w(x).float().cpu().numpy(), got)
    _check_against_rule(f"micro512 {size[0]}x{size[1]}", got, with_act, weights_only, float(np.abs(weights_only).max()))


# ---- 5. features at 48 x 96 ---------------------------------------------------------------------------------------------------------

def test_feature_outputs_on_a_rectangular_grid():
    name, size = "vit_micro_patch16_64", (48, 96)
    w = wrapped(name, "bf16").set_dynamic_img_size()
    x = torch.from_numpy(ni.images_of(size)).to(DEV)
    B, Cc, n0 = ni.BATCH, 128, 1 + 18
    tokens = w.forward_features(x)
    src = w.get_last_stats()["source_idx"].long()
    assert tokens.shape[0] == B and tokens.shape[2] == Cc and tuple(src.shape) == tuple(tokens.shape[:2])
    assert int(src.max()) < n0 and bool((src[:, 0] == 0).all()) and bool((src[:, 1:] > 0).all())
    dense = w.forward_features(x, dense=True)
    assert tuple(dense.shape) == (B, n0, Cc)
    assert same_bytes(torch.gather(dense, 1, src[:, :, None].expand(-1, -1, Cc)), tokens)
    rest = torch.ones(B, n0, dtype=torch.bool, device=DEV).scatter_(1, src, False)
    assert int(rest.sum()) == B * (n0 - tokens.shape[1]) > 0 and bool((dense[rest].view(torch.int16) == 0).all())
    last = w.forward_features(x, dense=True, fill="last")
    assert tuple(last.shape) == (B, n0, Cc) and tuple(w.get_last_stats()["exit_block"].shape) == (B, n0)
    assert same_bytes(torch.gather(last, 1, src[:, :, None].expand(-1, -1, Cc)), tokens)
    # the NCHW reshape is (gh, gw) = (3, 6)
    for kw in (dict(norm=True), dict(norm=False, fill="last")):
        final, nlc = w.forward_intermediates(x, indices=[0, 2, 3], output_fmt="NLC", **kw)
        final2, nchw = w.forward_intermediates(x, indices=[0, 2, 3], output_fmt="NCHW", **kw)
        assert same_bytes(final, final2) and tuple(final.shape) == (B, n0, Cc)
        for a, b in zip(nlc, nchw):
            assert tuple(a.shape) == (B, 18, Cc) and tuple(b.shape) == (B, Cc, 3, 6)
            assert same_bytes(a.reshape(B, 3, 6, Cc).permute(0, 3, 1, 2).contiguous(), b)
    flat = w.get_intermediate_layers(x, n=2)
    grid = w.get_intermediate_layers(x, n=2, reshape=True, return_class_token=True)
    for a, (b, cls) in zip(flat, grid):
        assert tuple(b.shape) == (B, Cc, 3, 6) and tuple(cls.shape) == (B, Cc)
        assert same_bytes(a.reshape(B, 3, 6, Cc).permute(0, 3, 1, 2).contiguous(), b)


# ---- 6. the cache of resampled embeddings --------------------------------------------------------------------------------------------

def test_alternating_sizes_and_changed_weights_equal_a_fresh_wrapper():
    name = "vit_micro_reg4_patch16_64"
    sizes = [(48, 96), (96, 48), (48, 96), (64, 64), (96, 48)]
    xs = {s: torch.from_numpy(ni.images_of(s)).to(DEV) for s in set(sizes)}
    fresh = lambda s, model=None: (rajni_amd.RAJNIViTWrapper(model if model is not None else ni.build_model(name), ni.SCHED)
                                   .to(DEV).to(torch.bfloat16).eval().set_dynamic_img_size())(xs[s])
    w = wrapped(name, "bf16").set_dynamic_img_size()
    for s in sizes:
        assert same_bytes(w(xs[s]), fresh(s)), s
    assert w._plan[8][1] is not w._weights["pos"] and set(k[:2] for k in w._weights["pos_cache"]) == {(3, 6), (6, 3)}
    w(xs[(64, 64)])
    assert w._plan[8][1] is w._weights["pos"], "the source grid uses the packed embedding itself"
    # an in-place change of the embedding: the cache goes with the repacked weights
    with torch.no_grad():
        w.m.pos_embed.mul_(0.5)
    changed = ni.build_model(name)
    with torch.no_grad():
        changed.pos_embed.mul_(0.5)
    got = w(xs[(48, 96)])
    assert same_bytes(got, fresh((48, 96), changed)) and not same_bytes(got, fresh((48, 96)))
    # at most 8 grids are kept, oldest out
    for k in range(1, 11):
        w(torch.zeros(1, 3, 16 * k, 32, dtype=torch.bfloat16, device=DEV))
    keys = [k[:2] for k in w._weights["pos_cache"]]
    assert len(keys) == 8 and keys[-1] == (10, 2) and (1, 2) not in keys


def test_the_reference_slice_stays_when_the_setter_is_off():
    """a class-token-only model fed a smaller square image: pos_embed[:, :N], the reference's arithmetic, as before"""
    cfg, sd = fixture("vit_micro_patch16_64")
    w = wrapped("vit_micro_patch16_64", "bf16", sched={})
    imgs = ni.images_of((32, 32))
    sliced = dict(sd)
    sliced["pos_embed"] = sd["pos_embed"][:, :5]
    want, _ = orc.vit_forward(sliced, imgs, {}, depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps)
    got = w(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    close(got, want, 1e-2, "32x32, dynamic_img_size off: the reference's slice")
    resampled, _ = orc.vit_forward(ni.sd_at_grid(sd, cfg, (2, 2), dt="bf16"), imgs, {}, depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps)
    on = w.set_dynamic_img_size()(torch.from_numpy(imgs).to(DEV)).float().cpu().numpy()
    close(on, resampled, 1e-2, "32x32, dynamic_img_size on: the resampled embedding")
    assert float(np.abs(resampled - want).max()) > 5e-2 * float(np.abs(want).max()), "the two semantics do not differ on this fixture"


def test_cli_runs_at_a_rectangular_size():
    """`python -m rajni_amd.run --img_size H W --dynamic_img_size` on synthetic batches"""
    from rajni_amd import run
    acc, thr = run.main(["--model", "vit_micro_patch16_64", "--batch_size", "8", "--max_batches", "2", "--warmup", "1",
                         "--synthetic", "--img_size", "48", "96", "--dynamic_img_size"])
    assert thr > 0 and 0.0 <= acc <= 100.0
    with pytest.raises(ValueError, match="set_dynamic_img_size"):
        run.main(["--model", "vit_micro_patch16_64", "--batch_size", "8", "--max_batches", "1", "--warmup", "0", "--synthetic",
                  "--img_size", "48", "96"])
