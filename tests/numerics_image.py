"""Yardsticks for inputs of any size (include/rajni_hip_image.h): the position-embedding resample restated in fp64, the
error budget of the kernel that computes it, an fp32 emulation of that kernel's own order, and the state dicts the restated
forward graphs read at a new token grid.  Pure numpy, shared by tests/test_image_size_cpu.py and tests/test_gpu_image_size.py.

The rule (timm's resample_abs_pos_embed = F.interpolate(mode="bicubic", antialias=True, align_corners=False) on the patch rows,
prefix rows passed through) is separable.  Per axis with scale = n_in / n_out:
    support = 2 * scale if scale >= 1 else 2;  inv = 1 / scale if scale >= 1 else 1
    output i:  c = scale * (i + 0.5);  taps j in [max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in))
    w_j = k((j - c + 0.5) * inv) / sum_j,   k = the Keys cubic with a = -0.5
and out[i, l, :] = sum_j sum_k wy[i, j] wx[l, k] src[j, k, :].  With equal sizes the weights are exactly 0 and 1."""
from __future__ import annotations

import numpy as np

import numerics as nm

F32 = np.float32
A = -0.5


def keys_cubic(t):
    t = abs(float(t))
    if t < 1.0:
        return ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * A
    return 0.0


def axis_taps(n_in: int, n_out: int):
    """[(lo, normalised fp64 weights of the taps lo, lo + 1, ...)] for every output of one axis"""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    out = []
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(int(c + support + 0.5), n_in)
        raw = np.array([keys_cubic((j - c + 0.5) * inv) for j in range(lo, hi)], np.float64)
        total = 0.0
        for v in raw:                 # ascending, as the kernel sums them
            total += v
        out.append((lo, raw / total))
    return out


def axis_matrix(n_in: int, n_out: int, dtype=np.float64):
    """[n_out, n_in] dense: row i holds output i's weights (rounded once to `dtype`), zeros outside its taps"""
    m = np.zeros((n_out, n_in), dtype)
    for i, (lo, w) in enumerate(axis_taps(n_in, n_out)):
        m[i, lo:lo + len(w)] = w.astype(dtype)
    return m


def resample_grid(src, src_grid, dst_grid):
    """src [sh * sw, C] -> [dh * dw, C] in fp64, the rule above"""
    (sh, sw), (dh, dw) = src_grid, dst_grid
    s = np.asarray(src, np.float64).reshape(sh, sw, -1)
    return np.einsum("ij,lk,jkc->ilc", axis_matrix(sh, dh), axis_matrix(sw, dw), s).reshape(dh * dw, -1)


def resample_pos_embed(pos, src_grid, dst_grid, prefix_rows):
    """pos [prefix + sh * sw, C] -> fp64 [prefix + dh * dw, C]: prefix rows as they are, patch rows resampled"""
    pos = np.asarray(pos, np.float64)
    return np.concatenate([pos[:prefix_rows], resample_grid(pos[prefix_rows:], src_grid, dst_grid)], axis=0)


def tap_counts(src_grid, dst_grid):
    """[dh * dw] taps (ny * nx) of every output"""
    ny = [len(w) for _, w in axis_taps(src_grid[0], dst_grid[0])]
    nx = [len(w) for _, w in axis_taps(src_grid[1], dst_grid[1])]
    return np.outer(ny, nx).reshape(-1)


def resample_budget(src, src_grid, dst_grid, dt: str):
    """(want, budget) [dh * dw, C] for the patch rows `src` (values of type dt).  Per element, with T = ny * nx taps and
    S = sum_jk |wy_j| |wx_k| |src_jk|:
        T u32 S        T fused multiply-adds in fp32, any order (gamma_T of the standard analysis, to first order);
        1 u32 S        the fp32 product wy_j * wx_k, rounded before it enters the FMA;
        2 u32 S        the weight tables: each fp64 weight rounded once to fp32, two of them per tap;
        u_dt |want|    one rounding to the output type (+ half its smallest subnormal).
    Derived from what the kernel does; nothing here is fitted to its output."""
    (sh, sw), (dh, dw) = src_grid, dst_grid
    s = np.asarray(src, np.float64).reshape(sh, sw, -1)
    wy, wx = axis_matrix(sh, dh), axis_matrix(sw, dw)
    want = np.einsum("ij,lk,jkc->ilc", wy, wx, s).reshape(dh * dw, -1)
    S = np.einsum("ij,lk,jkc->ilc", np.abs(wy), np.abs(wx), np.abs(s)).reshape(dh * dw, -1)
    T = tap_counts(src_grid, dst_grid)[:, None].astype(np.float64)
    return want, (T + 3.0) * nm.U32 * S + nm.UNIT[dt] * np.abs(want) + nm.FLOOR[dt]


def emul_resample(src, src_grid, dst_grid, dt: str, rounded: bool = True):
    """the kernel's own arithmetic in numpy: fp64 tables rounded once to fp32, w = fp32(wy_j * wx_k), fp32 FMA with source
    rows outer and columns inner, ascending, from 0; one rounding to dt.  src [sh * sw, C] fp32 values of type dt."""
    (sh, sw), (dh, dw) = src_grid, dst_grid
    s = np.asarray(src, F32).reshape(sh, sw, -1)
    ty, tx = axis_taps(sh, dh), axis_taps(sw, dw)
    out = np.zeros((dh, dw, s.shape[-1]), F32)
    for i, (y0, wy) in enumerate(ty):
        wy = wy.astype(F32)
        for l, (x0, wx) in enumerate(tx):
            wx = wx.astype(F32)
            acc = np.zeros(s.shape[-1], F32)
            for j in range(len(wy)):
                for k in range(len(wx)):
                    w = F32(wy[j] * wx[k])
                    acc = (np.float64(w) * s[y0 + j, x0 + k].astype(np.float64) + acc.astype(np.float64)).astype(F32)
            out[i, l] = acc
    out = out.reshape(dh * dw, -1)
    return nm.round_to(out, dt) if rounded else out


# ---- the restated forward graphs at a new token grid ---------------------------------------------------------------------------
# tests/numerics_variants.py, numerics_prefix.py, numerics_distilled.py and oracle.vit_forward take H x W images as they stand
# and read the position embedding from the state dict: these give them the embedding for the grid.

def pos_prefix_rows(cfg) -> int:
    """rows of the config's pos_embed in front of the patch rows"""
    return 0 if cfg.no_embed_class else cfg.num_prefix_tokens


def source_grid(cfg):
    g = cfg.img_size // cfg.patch_size
    return (g, g)


def sd_at_grid(sd, cfg, grid, how: str = "resampled", dt: str = None):
    """the state dict with pos_embed [1, prefix + gh * gw, C] for the token grid (gh, gw), rounded to the model dtype `dt` as
    timm's resample_abs_pos_embed returns it (`posemb.to(orig_dtype)`; None: left in fp64).  That rounding is part of the
    function restated, not of the device: a bf16 model adds the rounded rows, and the fp8_mfma format's chaotic quantiser turns
    those 2^-9 into 8 % of the logit scale on its fixture (0.09 % without the activation rule), so the yardstick has to hold them.
    "resampled"   the rule above (what dynamic_img_size computes);
    "transposed"  the wrong answer of a grid whose axes are swapped: resampled to (gw, gh) and read row-major as (gh, gw)
                  (a square target, where that is the right answer: the source grid transposed before resampling);
    "tiled"       the wrong answer of no resampling: the source's patch rows repeated (or cut) to gh * gw rows."""
    pr, src = pos_prefix_rows(cfg), source_grid(cfg)
    pos = np.asarray(sd["pos_embed"], np.float64)[0]
    gh, gw = grid
    if how == "resampled":
        new = resample_pos_embed(pos, src, (gh, gw), pr)
    elif how == "transposed" and gh != gw:
        new = resample_pos_embed(pos, src, (gw, gh), pr)
    elif how == "transposed":         # a square target: the swap shows as the transposed source grid
        t = pos[pr:].reshape(src[0], src[1], -1).transpose(1, 0, 2).reshape(src[0] * src[1], -1)
        new = resample_pos_embed(np.concatenate([pos[:pr], t], axis=0), (src[1], src[0]), (gh, gw), pr)
    elif how == "tiled":
        patch = pos[pr:]
        new = np.concatenate([pos[:pr], np.resize(patch, (gh * gw, patch.shape[1]))], axis=0)
    else:
        raise ValueError(how)
    out = dict(sd)
    out["pos_embed"] = (new if dt is None else nm.round_to(new, dt).astype(np.float64))[None].astype(np.float64)
    return out


def scaled_pos(sd, factor: float):
    """the state dict with pos_embed multiplied by `factor` and kept bf16-representable (a fixture whose embedding is too faint
    for the wrong answers to show is made to speak up, never the bar lowered)"""
    from rajni_amd import timm_shaped as ts
    out = dict(sd)
    out["pos_embed"] = ts.bf16_round_np((np.asarray(sd["pos_embed"], np.float32) * np.float32(factor)))
    return out


# ---- the forwards held to a bar at new sizes (tests/test_gpu_image_size.py), and what makes them able to tell --------------------
SCHED = {1: {"keep_ratio": 0.75, "update": True}, 2: {"keep_ratio": 0.6, "update": False}}
BATCH = 3
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}      # tests/test_gpu_prefix_forward.py's, per dtype
# (model, (H, W), dtype, weight format)
FORWARD_CASES = [
    ("vit_micro_patch16_64", (48, 96), "bf16", "model"), ("vit_micro_patch16_64", (96, 48), "bf16", "model"),
    ("vit_micro_patch16_64", (32, 32), "bf16", "model"), ("vit_micro_patch16_64", (96, 96), "bf16", "model"),
    ("vit_micro_patch16_64", (48, 96), "fp32", "model"),
    ("vit_micro_patch14_56", (42, 70), "bf16", "model"),
    ("vit_micro_reg4_patch16_64", (48, 80), "bf16", "model"),
    ("deit3_micro_patch16_64", (80, 48), "bf16", "model"),
    ("vit_micro_distilled_patch16_64", (48, 96), "bf16", "model"),
    ("vit_micro512_patch16_64", (48, 96), "bf16", "fp8_mfma"),
]
# the fixtures the existing forward tests of these configs use (smoke / test_gpu_prefix_forward / numerics_distilled /
# test_gpu_fp8_mfma), and the factor on pos_embed at which both wrong answers move the logits by 5x the bar in every case
# above (tests/test_image_size_cpu.py prints the ratios; DESIGN.md section 1 records them)
FIX = {
    "vit_micro_patch16_64": dict(seed=0, std=0.08, bias_std=0.02),
    "vit_micro_patch14_56": dict(seed=0, std=0.08, bias_std=0.02),
    "vit_micro_reg4_patch16_64": dict(seed=11, std=0.08, bias_std=0.1),
    "deit3_micro_patch16_64": dict(seed=0, std=0.08, bias_std=0.02),
    "vit_micro_distilled_patch16_64": dict(seed=3, std=0.08, bias_std=0.02),
    "vit_micro512_patch16_64": dict(seed=4, std=0.06, bias_std=0.02),
}
# As drawn (std 0.08, like every other weight) the embedding is too faint: the transposed grid moves the 32 x 32 logits of
# vit_micro_patch16_64 by 2.4x the bar, and both wrong answers stay below 1x the fp8_mfma bar.  With these factors the smallest
# ratio is 12.6x (16-bit and fp32 cases) and 6.4x (fp8_mfma, on the rms statistic of that format's check).
POS_SCALE = {name: 4.0 for name in FIX}
POS_SCALE["vit_micro512_patch16_64"] = 24.0


def build_model(name):
    """the timm-shaped model of a fixture: bf16-representable weights, pos_embed scaled by POS_SCALE (bf16-representable too)"""
    import torch
    from rajni_amd import timm_shaped as ts
    model = ts.create_model(ts.CONFIGS[name], round_bf16=True, **FIX[name])
    if POS_SCALE[name] != 1.0:
        with torch.no_grad():
            model.pos_embed.copy_((model.pos_embed * POS_SCALE[name]).to(torch.bfloat16).to(torch.float32))
    return model


def images_of(size, B=BATCH, seed=5):
    from rajni_amd import timm_shaped as ts
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, size[0], size[1]), dtype=np.float32))


def restated_logits(name, sd, images, forced_keep=None, act_fp8=False):
    """(logits, token counts, trace) of the restated pruned graph of the config on H x W images: numerics_distilled's for the
    distilled model, oracle.vit_forward for the act_fp8 format (as tests/test_gpu_fp8_mfma.py), numerics_prefix's otherwise"""
    from oracle import rajni_oracle as orc
    from rajni_amd import timm_shaped as ts
    import numerics_distilled as nd
    import numerics_prefix as npx
    cfg = ts.CONFIGS[name]
    if cfg.distilled:
        return nd.vit_forward_restated(sd, images, SCHED, cfg, forced_keep=forced_keep)
    if act_fp8:
        logits, stats, tr = orc.vit_forward(sd, images, SCHED, depth=cfg.depth, num_heads=cfg.num_heads, ln_eps=cfg.ln_eps,
                                            forced_keep=forced_keep, act_fp8=True, return_trace=True)
        return logits, stats["token_counts"], tr
    return npx.vit_forward_restated(sd, images, SCHED, cfg, forced_keep=forced_keep)


def dequantized_sd(sd, cfg):
    """the state dict with the four block Linear weights as the fp8 formats hold them (ops.quantize_rows_fp8 of the bf16
    weight, dequantised), computed on the host"""
    import torch
    from rajni_amd import ops
    out = dict(sd)
    for i in range(cfg.depth):
        for k in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
            key = f"blocks.{i}.{k}.weight"
            q, s = ops.quantize_rows_fp8(torch.from_numpy(np.asarray(sd[key], np.float32)).to(torch.bfloat16))
            out[key] = (q.to(torch.float32) * s[:, None]).numpy()
    return out


def wrong_answers_move(name, size, dt, fmt):
    """{wrong answer: (moved, need)}: how far the transposed grid and the un-resampled embedding move the logits of the
    restated graph (the right answer's selections kept), and 5x the bar the GPU test of the case applies"""
    from oracle import rajni_oracle as orc
    from rajni_amd import timm_shaped as ts
    cfg = ts.CONFIGS[name]
    sd = ts.state_dict_numpy(build_model(name))
    f8 = fmt == "fp8_mfma"
    if f8:
        sd = dequantized_sd(sd, cfg)
    grid = (size[0] // cfg.patch_size, size[1] // cfg.patch_size)
    imgs = images_of(size)
    right, _, tr = restated_logits(name, sd_at_grid(sd, cfg, grid, dt=dt), imgs, act_fp8=f8)
    forced = {i: t["keep_idx"] for i, t in tr.items()}
    scale = float(np.abs(right).max())
    rms = lambda a: float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))
    if f8:
        # tests/test_gpu_fp8_mfma.py::_check_against_rule holds two statistics, and a wrong answer fails the test when it breaks
        # either.  The one that "catches a wiring bug" (its words) is the rms over all logits, r_err <= 1.35 r_cost + 2e-3 scale,
        # r_cost the rms of the rule's own effect; the maximum, err <= 1.6 cost + 1e-2 scale, is the chaotic statistic.  The
        # fixture is held to 5x the rms bar; the maximum's ratio is printed beside it (8.4x and 4.8x at POS_SCALE 24).
        plain, _ = orc.vit_forward(sd_at_grid(sd, cfg, grid, dt=dt), imgs, SCHED, depth=cfg.depth, num_heads=cfg.num_heads,
                                   ln_eps=cfg.ln_eps, forced_keep=forced)
        scale = float(np.abs(plain).max())
        bar, bar_max = 1.35 * rms(right - plain) + 2e-3 * scale, 1.6 * float(np.abs(right - plain).max()) + 1e-2 * scale
    else:
        bar = BAR[dt] * scale
    out = {}
    for how in ("transposed", "tiled"):
        wrong, _, _ = restated_logits(name, sd_at_grid(sd, cfg, grid, how, dt=dt), imgs, forced_keep=forced, act_fp8=f8)
        if f8:
            print(f"[image] fp8_mfma, {how}: the maximum moves by {np.abs(wrong - right).max() / bar_max:.2f}x its bar")
        out[how] = (rms(wrong - right) if f8 else float(np.abs(wrong - right).max()), 5 * bar)
    return out
