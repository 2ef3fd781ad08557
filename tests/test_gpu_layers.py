"""`forward_intermediates` / `get_intermediate_layers` on the device (rajni_vit_forward_layers): the states behind several blocks
from ONE forward, each on the unpruned grid.  GPU box only (`-m gpu`).  Batch 3: the selections differ per image.

Exact yardstick (bit for bit, no tolerance), against merged code: with norm=True, the slab of captured block c is what
`forward_features(x, dense=True, fill=fill)` of a SECOND wrapper writes whose base model is a deep copy cut to blocks[:c + 1],
scheduled in the blocks <= c, with the full run's selections forced - the merged kernels at the same shapes, and a row of a
LayerNorm or GEMM result does not depend on the launch it is in.  `final` is the same wrapper's forward_features.
Parity yardstick (norm=False, which no merged code computes): tests/numerics_layers.py in fp64 with the native selections
forced, max|err| / max|want| per slab against the project's bar max(BAR[dt], 1.5 x d16), d16 measured
here by the restatement in the model's 16-bit dtype on the CPU."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guarded
import numerics_layers as ny
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts

DEV = "cuda"
TORCH = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
BAR = {"bf16": 1e-2, "fp16": 1e-2, "fp32": 1e-3}
FIX = dict(seed=11, std=0.08, bias_std=0.1)
FIX512 = dict(seed=4, std=0.06, bias_std=0.02)
SCHED = {1: {"keep_ratio": 0.7}, 2: {"keep_ratio": 0.5}}
WIDE = ts.ViTConfig(img_size=32, embed_dim=1280, num_heads=20, depth=2)      # more than 1024 channels: four chunks per lane
DEEP = ts.ViTConfig(img_size=128, embed_dim=128, num_heads=2, depth=10)      # ten scheduled blocks: the level table chains


def cfg_of(name_or_cfg):
    return ts.config_of(name_or_cfg) if isinstance(name_or_cfg, str) else name_or_cfg


def images_of(cfg, seed, B=3):
    return ts.bf16_round_np(np.random.default_rng(seed).standard_normal((B, 3, cfg.img_size, cfg.img_size), dtype=np.float32))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def random_selections(cfg, sched, B=3, seed=0):
    """{block: keep_idx [B, P + keep]} drawn at random per image (prefix slots, then ascending patch indices)"""
    rng = np.random.default_rng(seed)
    P, N = cfg.num_prefix_tokens, cfg.num_patches + cfg.num_prefix_tokens
    out = {}
    for i in sorted(sched):
        keep = max(1, int(sched[i]["keep_ratio"] * (N - P)))
        out[i] = np.stack([np.concatenate([np.arange(P), P + np.sort(rng.choice(N - P, keep, replace=False))]) for _ in range(B)])
        N = P + keep
    return out


class Setup:
    """one base model and how its wrappers are configured (tests/test_gpu_features_last.py's, restated): `wrap(sched, forced)`
    gives the full wrapper, `blocks=i` a twin whose base is a deep copy cut to blocks[:i]"""

    def __init__(self, name_or_cfg, dt="bf16", fix=FIX, stream=False, weights="model"):
        self.cfg, self.dt, self.stream, self.weights = cfg_of(name_or_cfg), dt, stream, weights
        self.base = ts.create_model(self.cfg, round_bf16=True, **fix)

    def wrap(self, sched, forced=None, blocks=None):
        base = copy.deepcopy(self.base)
        if blocks is not None:
            base.blocks = base.blocks[:blocks]
        w = rajni_amd.RAJNIViTWrapper(base, sched).to(DEV).to(TORCH[self.dt]).eval()
        if self.stream:
            w.set_residual_dtype(TORCH[self.dt])
        if self.weights != "model":
            w.set_weight_format(self.weights)
        if forced:
            w.force_keep_idx({i: torch.as_tensor(v).to(DEV) for i, v in forced.items()})
        return w


def slabs_of(inter):
    """[(spatial [B, n, C], prefix [B, P, C])] -> [L, B, P + n, C]"""
    return torch.stack([torch.cat([prefix, spatial], dim=1) for spatial, prefix in inter])


def check_exact(setup, sched, x, caps, forced=None):
    """norm=True, both fills: every slab against its cut twin, `final` against forward_features, the alive mask against
    exit_block, and the logits plan's slabs (intermediates_only=True) against the feature plan's.  Returns (wrapper, exit_block)"""
    cfg = setup.cfg
    B, depth, P, n0 = x.shape[0], cfg.depth, cfg.num_prefix_tokens, cfg.num_patches + cfg.num_prefix_tokens
    w = setup.wrap(sched, forced)
    got = {}
    for fill in ("zero", "last"):
        final, inter = w.forward_intermediates(x, indices=caps, norm=True, output_fmt="NLC", return_prefix_tokens=True, fill=fill)
        stats = w.get_last_stats()
        assert sorted(stats) == ["exit_block", "source_idx", "token_counts"]
        assert w._plan[5] == ("layers", "dense_last" if fill == "last" else "dense", tuple(caps), True, fill)
        assert len(inter) == len(caps)
        slabs = slabs_of(inter)
        assert tuple(slabs.shape) == (len(caps), B, n0, cfg.embed_dim) and slabs.dtype == TORCH[setup.dt]
        assert not torch.isnan(slabs.float()).any()
        only = w.forward_intermediates(x, indices=caps, norm=True, output_fmt="NLC", return_prefix_tokens=True, fill=fill,
                                       intermediates_only=True)
        assert w._plan[5][1] == "logits" and same_bits(slabs_of(only), slabs), "the logits plan's slabs differ"
        assert sorted(w.get_last_stats()) == ["exit_block", "source_idx", "token_counts"]
        assert same_bits(final, w.forward_features(x, dense=True, fill=fill)), f"final differs from forward_features (fill={fill})"
        got[fill] = (slabs.clone(), stats["exit_block"].clone(), stats["token_counts"])
    ex, counts = got["last"][1], got["last"][2]
    assert torch.equal(ex, got["zero"][1]) and ex.dtype == torch.int32 and tuple(ex.shape) == (B, n0) and bool((ex[:, :P] == depth).all())
    sel = {i: t["keep_idx"].cpu().numpy() for i, t in w.get_last_trace().items()}
    assert sorted(sel) == sorted(int(k) for k in sched)
    for l, c in enumerate(caps):
        alive = ex > c
        zero, last = got["zero"][0][l], got["last"][0][l]
        assert not zero[~alive].contiguous().view(torch.uint8).any(), f"slab of block {c}: a pruned row is not zero"
        rows_zero = (last.contiguous().view(torch.uint8).view(B, n0, -1) == 0).all(dim=-1)
        assert int(rows_zero.sum()) == 0, f"slab of block {c}, fill=last: a row is zero"
        assert same_bits(zero[alive], last[alive])
        twin = setup.wrap({k: v for k, v in sched.items() if int(k) <= c}, {k: v for k, v in sel.items() if k <= c}, blocks=c + 1)
        for fill, mine in (("zero", zero), ("last", last)):
            want = twin.forward_features(x, dense=True, fill=fill)
            assert twin.get_last_stats()["token_counts"] == counts[:c + 1]
            assert same_bits(mine, want), f"slab of block {c} (fill={fill}) differs from the cut model's forward_features"
        assert float(last.float().abs().max()) > 0.1
    return w, ex.cpu().numpy()


# ---- exact, against the cut twins -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("caps", [[0, 1, 2, 3], [1, 3], [2]], ids=lambda c: "c" + "".join(map(str, c)))
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_slabs_are_the_cut_models_dense_features(name, caps):
    setup = Setup(name)
    x = torch.from_numpy(images_of(setup.cfg, seed=4)).to(DEV)
    w, ex = check_exact(setup, SCHED, x, caps)
    assert sorted(np.unique(ex)) == [1, 2, setup.cfg.depth]
    assert len({tuple(r) for r in ex}) > 1, "the maps must differ between the images"


def _corner(cfg, patches, B=3):
    """one stage at block 1 that keeps exactly `patches` (the same for every image)"""
    P = cfg.num_prefix_tokens
    ratio = (len(patches) + 0.5) / cfg.num_patches
    return {1: {"keep_ratio": ratio}}, {1: np.tile(np.concatenate([np.arange(P), P + np.asarray(patches)]), (B, 1))}


@pytest.mark.parametrize("what", ["ratio_one", "first_patch", "last_patch", "c1280", "deep_chain", "fp32", "fp16", "stream_bf16",
                                  "stream_fp16", "fp8_weights", "distilled"])
def test_across_schedules_widths_depths_and_types(what):
    setup, sched, forced, caps = None, SCHED, None, [1, 3]
    if what == "ratio_one":            # a captured scheduled block that drops nothing
        setup, sched, caps = Setup("vit_micro_patch16_64"), {1: {"keep_ratio": 1.0}, 2: {"keep_ratio": 0.5}}, [1, 2, 3]
    elif what in ("first_patch", "last_patch"):      # the searches' corners
        setup = Setup("vit_micro_reg4_patch16_64")
        sched, forced = _corner(setup.cfg, [0] if what == "first_patch" else [setup.cfg.num_patches - 1])
        caps = [0, 1, 3]
    elif what == "c1280":
        setup, sched, caps = Setup(WIDE, fix=dict(seed=4, std=0.03, bias_std=0.02)), {1: {"keep_ratio": 0.5}}, [0, 1]
    elif what == "deep_chain":         # a row dropped at block 0 goes to ten targets, and the level table chains
        setup, sched, caps = Setup(DEEP), {i: {"keep_ratio": 0.9} for i in range(10)}, list(range(10))
        forced = random_selections(setup.cfg, sched, seed=9)
    elif what == "fp8_weights":
        setup = Setup("vit_micro512_patch16_64", fix=FIX512, weights="fp8")
    elif what == "distilled":
        setup = Setup("vit_micro_distilled_patch16_64")
    else:
        dt = {"stream_bf16": "bf16", "stream_fp16": "fp16", "fp32": "fp32", "fp16": "fp16"}[what]
        setup = Setup("vit_micro_reg4_patch16_64", dt=dt, stream=what.startswith("stream"))
    x = torch.from_numpy(images_of(setup.cfg, seed=6)).to(DEV)
    w, ex = check_exact(setup, sched, x, caps, forced)
    counts = w.get_last_stats()["token_counts"]
    if what == "ratio_one":
        assert counts == [17, 17, 17, 9] and not (ex == 1).any() and (ex == 2).sum() == 3 * 8
    elif what == "deep_chain":
        assert counts == [65, 58, 52, 46, 41, 37, 33, 29, 26, 23] and sorted(np.unique(ex)) == list(range(11))
    elif what in ("first_patch", "last_patch"):
        P = setup.cfg.num_prefix_tokens
        assert counts == [P + 16, P + 16, P + 1, P + 1] and (ex == 4).sum() == 3 * (P + 1)
    elif what == "distilled":          # the head still reads its two rows: the logits do not move
        logits = w(x)
        assert same_bits(logits, setup.wrap(sched)(x))


# ---- final, logits, launches ------------------------------------------------------------------------------------------------

def _launches(fn):
    nat.profile_reset()
    nat.profile_enable((1 << nat.NUM_KCLASS) - 1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        nat.profile_enable(0)
    out = {k: v["launches"] for k, v in nat.profile_collect().items()}
    nat.profile_reset()
    return out


def test_logits_and_features_before_and_after_and_the_added_launches():
    setup = Setup("vit_micro_patch16_64")
    w = setup.wrap(SCHED)
    x = torch.from_numpy(images_of(setup.cfg, seed=12)).to(DEV)
    logits, dense = w(x).clone(), w.forward_features(x, dense=True).clone()
    last = w.forward_features(x, dense=True, fill="last").clone()
    n_logits, n_dense = _launches(lambda: w(x)), _launches(lambda: w.forward_features(x, dense=True))
    n_last = _launches(lambda: w.forward_features(x, dense=True, fill="last"))
    total = lambda d: sum(d.values())
    # per captured block one map launch (no chain at this depth) and one dense launch; with fill="last" one more for every
    # scheduled block i with a capture >= i - and, where the plan is not the dense_last one, the map those rows need
    for caps, later in (([0, 2], 2), ([0], 0), ([1, 2, 3], 2), ([0, 1, 2, 3], 2)):
        fi = lambda **kw: w.forward_intermediates(x, indices=caps, **dict(dict(norm=True), **kw))
        n = _launches(lambda: fi())
        assert total(n) == total(n_dense) + 2 * len(caps), (caps, n, n_dense)
        n = _launches(lambda: fi(fill="last"))
        assert total(n) == total(n_last) + 2 * len(caps) + later, (caps, n, n_last)
        if caps[-1] != 3:      # (capturing the last block changes the last block's form as well: held by bits below)
            n = _launches(lambda: fi(intermediates_only=True))
            assert total(n) == total(n_logits) + 2 * len(caps), (caps, n, n_logits)
            n = _launches(lambda: fi(intermediates_only=True, fill="last"))
            assert total(n) == total(n_logits) + 2 * len(caps) + 2 * later, (caps, n, n_logits)
            n = _launches(lambda: fi(intermediates_only=True, fill="last", norm=False))
            assert total(n) == total(n_logits) + 2 * len(caps) + 2 * later, (caps, n, n_logits)
        # the other outputs, interleaved with the new one: the same bits and the same launches (the optimistic launch must
        # never send a logits or feature plan into slabs, nor the other way round)
        assert same_bits(w(x), logits) and w.get_last_stats() == {"token_counts": [17, 17, 12, 6]}
        fi(intermediates_only=True)
        assert same_bits(w(x), logits)
        assert same_bits(w.forward_features(x, dense=True), dense) and sorted(w.get_last_stats()) == ["source_idx", "token_counts"]
        fi(fill="last")
        assert same_bits(w.forward_features(x, dense=True, fill="last"), last)
    assert _launches(lambda: w(x)) == n_logits and _launches(lambda: w.forward_features(x, dense=True)) == n_dense
    assert _launches(lambda: w.forward_features(x, dense=True, fill="last")) == n_last


@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_a_null_record_is_the_merged_entry_point(name):
    setup = Setup(name)
    w = setup.wrap(SCHED)
    x = torch.from_numpy(images_of(setup.cfg, seed=13)).to(DEV).to(torch.bfloat16).contiguous()
    want = w(x).clone()
    plan, keep = w._plan[1], w._plan[2]
    ext, pre = keep[4], keep[6]
    args = (C.byref(plan), C.byref(ext) if ext is not None else None, C.byref(pre) if pre is not None else None)
    # (zeros: the head writes num_classes of the logits_ld columns of a row)
    outs = [torch.zeros((x.shape[0], plan.logits_ld), dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    old = lambda: nat.check(nat.lib().rajni_vit_forward_ext_prefix(*args, x.data_ptr(), outs[0].data_ptr(), nat.stream_ptr(x.device)), "old")
    new = lambda: nat.check(nat.lib().rajni_vit_forward_layers(*args, None, x.data_ptr(), outs[1].data_ptr(), nat.stream_ptr(x.device)), "new")
    n_old, n_new = _launches(old), _launches(new)
    assert n_old == n_new and sum(n_old.values()) > 0
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0][:, :plan.num_classes], want)


# ---- output bounds -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["zero", "last"])
@pytest.mark.parametrize("misalign", [0, 16], ids=["aligned256", "min_alignment"])
@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_every_slab_byte_is_written_once_and_nothing_beyond(name, misalign, fill):
    """slabs 64 elements further apart than the dense size, at 256-byte alignment and at the ABI's minimum (16 bytes past a
    256-byte boundary): every slab byte written, the gaps and the guard zones untouched, the same bits - both norm values"""
    setup = Setup(name)
    w = setup.wrap(SCHED)
    caps = [0, 1, 2, 3]
    x = torch.from_numpy(images_of(setup.cfg, seed=10)).to(DEV).to(torch.bfloat16).contiguous()
    for norm in (True, False):
        final, inter = w.forward_intermediates(x, indices=caps, norm=norm, output_fmt="NLC", return_prefix_tokens=True, fill=fill)
        want = slabs_of(inter)
        entry = w._plan
        plan, keep, (cap_arr, lnorm, lfill, shape) = entry[1], entry[2], entry[7]
        ext, pre = keep[4], keep[6]
        assert (lnorm, lfill) == (int(norm), int(fill == "last")) and shape == tuple(want.shape)
        dense = shape[1] * shape[2] * shape[3]
        g = guarded.Guarded((len(caps), dense), torch.bfloat16, device=DEV, row_stride=dense + 64, misalign=misalign,
                            align=16 if misalign else guarded.ALIGN)
        lay = nat.VitLayers()
        lay.n, lay.blocks, lay.norm, lay.fill, lay.out, lay.slab_stride = len(caps), cap_arr, lnorm, lfill, g.ptr(), dense + 64
        out = torch.empty(entry[6], dtype=torch.bfloat16, device=DEV)
        nat.check(nat.lib().rajni_vit_forward_layers(C.byref(plan), C.byref(ext), C.byref(pre) if pre is not None else None,
                                                     C.byref(lay), x.data_ptr(), out.data_ptr(), nat.stream_ptr(x.device)),
                  "rajni_vit_forward_layers")
        torch.cuda.synchronize()
        g.check(f"{name} slabs norm={norm} fill={fill}", written=True)
        assert not torch.isnan(g.t.float()).any()
        assert same_bits(g.t.reshape(shape), want) and same_bits(out, final)
        zero_rows = (g.t.contiguous().view(torch.uint8).view(shape[0] * shape[1] * shape[2], -1) == 0).all(dim=-1)
        if fill == "last":
            assert int(zero_rows.sum()) == 0, "no row is zero-filled"
        else:
            ex = w.get_last_stats()["exit_block"]
            assert int(zero_rows.sum()) == sum(int((ex <= c).sum()) for c in caps)


# ---- norm=False: the cast-only rows, against the restated graph ------------------------------------------------------------------

@pytest.mark.parametrize("name, dt, stream", [
    ("vit_micro_patch16_64", "bf16", False), ("vit_micro_patch16_64", "fp16", False), ("vit_micro_patch16_64", "fp32", False),
    ("vit_micro_reg4_patch16_64", "bf16", False), ("vit_micro_reg4_patch16_64", "fp32", False),
    ("vit_micro_reg4_patch16_64", "bf16", True), ("vit_micro_reg4_patch16_64", "fp16", True),
    ("vit_micro_fcnorm_patch16_64", "bf16", False), ("vit_micro_fcnorm_patch16_64", "fp32", False),
])
def test_unnormalised_slabs_against_the_restated_graph(name, dt, stream):
    cfg = cfg_of(name)
    setup = Setup(name, dt=dt, stream=stream)
    caps = [0, 1, 2, 3]
    x_np = images_of(cfg, seed=5)
    x = torch.from_numpy(x_np).to(DEV)
    sd = ts.state_dict_numpy(setup.base)
    if cfg.use_fc_norm:       # no final norm: norm=True is out of scope and says so; norm=False is what such a model gives
        with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
            setup.wrap(SCHED).forward_intermediates(x, norm=True, intermediates_only=True)
        with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
            setup.wrap(SCHED).forward_intermediates(x, norm=False)      # `final` is forward_features, which needs the norm
    forced = None
    for fill in ("zero", "last"):
        want = ny.layers_restated(sd, x_np, SCHED, cfg, caps, False, fill, forced_keep=forced)
        forced = {i: t["keep_idx"] for i, t in want["trace"].items()}
        w = setup.wrap(SCHED, forced)
        inter = w.forward_intermediates(x, indices=caps, norm=False, output_fmt="NLC", return_prefix_tokens=True, fill=fill,
                                        intermediates_only=True)
        got = slabs_of(inter).float().cpu().numpy()
        stats = w.get_last_stats()
        assert stats["token_counts"] == want["counts"]
        np.testing.assert_array_equal(stats["exit_block"].cpu().numpy(), want["exit_block"])
        np.testing.assert_array_equal(stats["source_idx"].cpu().numpy(), want["source_idx"])
        r16 = ny.layers_restated(sd, x_np, SCHED, cfg, caps, False, fill, forced_keep=forced, dtype=TORCH[dt]) if dt != "fp32" else None
        for l, c in enumerate(caps):
            scale = float(np.abs(want["slabs"][l]).max())
            d16 = float(np.abs(r16["slabs"][l] - want["slabs"][l]).max() / scale) if r16 is not None else 0.0
            bar = max(BAR[dt], 1.5 * d16)
            err = float(np.abs(got[l] - want["slabs"][l]).max()) / scale
            print(f"[layers] {name} {dt}{' stream' if stream else ''} fill={fill} block {c}: max|err| / max|want| {err:.3g} "
                  f"(d16 {d16:.3g}, bar {bar:.3g})")
            assert err <= bar, (name, dt, fill, c, err, bar)
            if fill == "zero":
                assert not got[l][want["exit_block"] <= c].any()
        if dt == "fp32" and not cfg.use_fc_norm and fill == "last":
            # the fp64 LayerNorm of the cast-only slab is the norm=True slab (no row is zero with this fill)
            normed = slabs_of(w.forward_intermediates(x, indices=caps, norm=True, output_fmt="NLC", return_prefix_tokens=True,
                                                      fill=fill, intermediates_only=True)).float().cpu().numpy()
            again = ny.layernorm64(got, sd, cfg.ln_eps)
            err = float(np.abs(again - normed).max() / np.abs(normed).max())
            print(f"[layers] {name} fp32: LayerNorm64(norm=False slab) vs norm=True slab: {err:.3g} (bar {BAR['fp32']:.3g})")
            assert err <= BAR["fp32"], err


# ---- formats ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_formats_are_views_of_one_result(name):
    setup = Setup(name)
    cfg = setup.cfg
    B, P, g, Cd = 3, cfg.num_prefix_tokens, cfg.img_size // cfg.patch_size, cfg.embed_dim
    w = setup.wrap(SCHED)
    x = torch.from_numpy(images_of(cfg, seed=14)).to(DEV)
    final, nlc = w.forward_intermediates(x, indices=[1, 3], output_fmt="NLC")
    assert tuple(final.shape) == (B, P + g * g, Cd) and [tuple(t.shape) for t in nlc] == [(B, g * g, Cd)] * 2
    assert nlc[0].untyped_storage().data_ptr() == nlc[1].untyped_storage().data_ptr(), "one allocation"
    final2, nchw = w.forward_intermediates(x, indices=[1, 3])                  # timm's defaults: NCHW, norm=False
    assert same_bits(final, final2) and [tuple(t.shape) for t in nchw] == [(B, Cd, g, g)] * 2 and all(t.is_contiguous() for t in nchw)
    for a, b in zip(nlc, nchw):
        assert same_bits(a.reshape(B, g, g, Cd).permute(0, 3, 1, 2).contiguous(), b)
    _, pairs = w.forward_intermediates(x, indices=[1, 3], return_prefix_tokens=True)
    for (spatial, prefix), b in zip(pairs, nchw):
        assert same_bits(spatial, b) and tuple(prefix.shape) == (B, P, Cd)
    only = w.forward_intermediates(x, indices=[1, 3], intermediates_only=True)
    assert isinstance(only, list) and all(same_bits(a, b) for a, b in zip(only, nchw))
    # indices: None is every block, an int the last k, negatives count from the end
    assert len(w.forward_intermediates(x, intermediates_only=True)) == cfg.depth
    last2 = w.forward_intermediates(x, indices=2, intermediates_only=True)
    neg = w.forward_intermediates(x, indices=[-1, -2], intermediates_only=True)
    assert len(last2) == 2 and all(same_bits(a, b) for a, b in zip(last2, neg))
    # DINOv2's call
    dino = w.get_intermediate_layers(x, n=2, reshape=True, return_class_token=True)
    ref = w.forward_intermediates(x, indices=2, norm=True, return_prefix_tokens=True, intermediates_only=True)
    assert isinstance(dino, tuple) and len(dino) == 2
    for (patches, cls), (spatial, prefix) in zip(dino, ref):
        assert same_bits(patches, spatial) and same_bits(cls, prefix[:, 0]) and tuple(cls.shape) == (B, Cd)
    flat = w.get_intermediate_layers(x, n=[1, 3])
    assert isinstance(flat, tuple) and [tuple(t.shape) for t in flat] == [(B, g * g, Cd)] * 2
    want = w.forward_intermediates(x, indices=[1, 3], norm=True, output_fmt="NLC", intermediates_only=True)
    assert all(same_bits(a, b) for a, b in zip(flat, want))
