"""`forward_intermediates` / rajni_vit_forward_layers without a device: the new symbol and header beside the pins that must not
move, every refusal of the layers record before the first launch (the fake-pointer plans of tests/test_features_cpu.py:
workspace = NULL, so "workspace too small" means every check in front of it passed), the index rule, what the wrapper refuses,
and the restatement of tests/numerics_layers.py against the base model's own blocks and against the merged yardsticks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import numerics_features as nf
import numerics_last as nl
import numerics_layers as ny
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper.model import take_indices
from test_features_cpu import ERR_INVALID, ERR_UNSUPPORTED, FAKE, FIX, IMAGES, LOGITS, SCHED, _ext, _plan, images_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = "rajni_vit_forward_layers"
OUT = FAKE + 0x400
DENSE = 4 * 17 * 128        # B * (P + n) * C of the fake plan with one prefix token


# ---- pins ---------------------------------------------------------------------------------------------------------------------

def test_the_new_symbol_resolves_and_the_header_declares_it_alone():
    assert nat.LAYERS_SYMBOLS == ("rajni_vit_forward_layers",)
    fn = nat.lib().rajni_vit_forward_layers
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    header = open(os.path.join(ROOT, "include", "rajni_hip_layers.h")).read()
    assert set(re.findall(r"\b(rajni_[a-z0-9_]+)\s*\(", header)) - {"rajni_stream_t"} == set(nat.LAYERS_SYMBOLS)
    assert re.search(r"#define RAJNI_MAX_LAYERS 64\b", header) and nat.MAX_LAYERS == 64
    assert C.sizeof(nat.VitLayers) == 40 and nat.VitLayers.out.offset == 24 and nat.VitLayers.slab_stride.offset == 32


def test_the_old_pins_hold():
    assert len(nat.EXPORTED_SYMBOLS) == 45 and not set(nat.LAYERS_SYMBOLS) & set(nat.EXPORTED_SYMBOLS)
    assert nat.lib().rajni_abi_version() == nat.ABI_VERSION == 8 and nat.NUM_KCLASS == 17
    assert C.sizeof(nat.VitExt) == 72 and C.sizeof(nat.VitPrefix) == 16
    header = open(os.path.join(ROOT, "include", "rajni_hip.h")).read()
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", header) and re.search(r"RAJNI_NUM_KCLASS\s*=\s*17\b", header)
    header += open(os.path.join(ROOT, "include", "rajni_hip_debug.h")).read()
    assert set(re.findall(r"\b(rajni_[a-z0-9_]+)\s*\(", header)) - {"rajni_stream_t"} == set(nat.EXPORTED_SYMBOLS)


# ---- the record's refusals ------------------------------------------------------------------------------------------------------

def _layers(blocks=(1, 3), norm=1, fill=0, out=OUT, stride=0, n=None):
    arr = (C.c_int * max(1, len(blocks)))(*blocks) if blocks is not None else None
    y = nat.VitLayers()
    y.n = len(blocks) if n is None else n
    y.blocks, y.norm, y.fill, y.out, y.slab_stride = arr, norm, fill, out, stride
    return y, arr


def _forward(p, layers, ext=None, prefix=None):
    lib = nat.lib()
    rc = lib.rajni_vit_forward_layers(C.byref(p), C.byref(ext) if ext is not None else None,
                                      C.byref(prefix) if prefix is not None else None,
                                      C.byref(layers) if layers is not None else None, IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _reaches_the_workspace_check(p, layers, ext=None, prefix=None):
    rc, msg = _forward(p, layers, ext, prefix)
    assert rc == ERR_INVALID and "workspace too small" in msg, (rc, msg)


@pytest.mark.parametrize("headless", [True, False])
def test_a_clean_record_and_a_null_record_reach_the_workspace_check(headless):
    for keeps, buffers in (((0, 8, 6, 0), (1, 2)), ((0, 0, 0, 0), ()), ((8, 6, 4, 2), (0, 1, 2, 3))):
        p, keep_alive = _plan(keeps, buffers, headless=headless)
        _reaches_the_workspace_check(p, None)
        _reaches_the_workspace_check(p, None, _ext(mlp_act=nat.MLP_QUICK_GELU), nat.VitPrefix(5, FAKE))
        for blocks in ((0, 1, 2, 3), (1, 3), (2,), (0,)):
            for norm in (0, 1):
                for fill in (0, 1):
                    y, arr = _layers(blocks, norm, fill)
                    _reaches_the_workspace_check(p, y)
                    _reaches_the_workspace_check(p, y, _ext(mlp_act=nat.MLP_SWIGLU, norm_pre_w=FAKE))
        y, arr = _layers(stride=DENSE + 64)
        _reaches_the_workspace_check(p, y)
        y, arr = _layers(stride=4 * 21 * 128, out=OUT + 16)        # five prefix tokens: a larger dense size
        _reaches_the_workspace_check(p, y, None, nat.VitPrefix(5, FAKE))
        if headless:
            for pool in (nat.POOL_NONE, nat.POOL_DENSE, nat.POOL_DENSE_LAST):
                y, arr = _layers()
                _reaches_the_workspace_check(p, y, _ext(pool))
        y, arr = _layers(norm=0)                                    # cast only: a plan without a final norm is served
        _reaches_the_workspace_check(p, y, _ext(nat.POOL_AVG, fc_norm_w=FAKE, norm_absent=1))
        del keep_alive


@pytest.mark.parametrize("kw, code, what", [
    (dict(n=0), ERR_INVALID, "layers.n must be 1..64 (0)"),
    (dict(n=65), ERR_INVALID, "layers.n must be 1..64 (65)"),
    (dict(n=-1), ERR_INVALID, "layers.n must be 1..64 (-1)"),
    (dict(blocks=None, n=2), ERR_INVALID, "null pointer (layers.blocks)"),
    (dict(out=None), ERR_INVALID, "null pointer (layers.out)"),
    (dict(blocks=(1, 1)), ERR_INVALID, "strictly ascending"),
    (dict(blocks=(2, 1)), ERR_INVALID, "strictly ascending"),
    (dict(blocks=(1, 4)), ERR_INVALID, "in [0, 4) (blocks[1] = 4)"),
    (dict(blocks=(-1, 2)), ERR_INVALID, "in [0, 4) (blocks[0] = -1)"),
    (dict(norm=2), ERR_INVALID, "layers.norm must be 0 or 1 (2)"),
    (dict(norm=-1), ERR_INVALID, "layers.norm must be 0 or 1 (-1)"),
    (dict(fill=2), ERR_INVALID, "layers.fill must be 0 (zero rows) or 1 (last state) (2)"),
    (dict(fill=-1), ERR_INVALID, "layers.fill must be 0"),
    (dict(stride=DENSE - 8), ERR_INVALID, f"layers.slab_stride must be 0 or a multiple of 8 that is >= B * (P + n) * C = {DENSE}"),
    (dict(stride=DENSE + 4), ERR_INVALID, "layers.slab_stride"),
    (dict(stride=-8), ERR_INVALID, "layers.slab_stride"),
    (dict(out=OUT + 8), ERR_INVALID, "layers.out"),
])
def test_every_refusal_of_the_record_comes_before_the_workspace_check(kw, code, what):
    p, keep_alive = _plan()
    y, arr = _layers(**kw)
    rc, msg = _forward(p, y)
    assert rc == code and WHO in msg and what in msg and "workspace" not in msg, (rc, msg)
    del keep_alive


def test_the_refusals_that_depend_on_the_plan_and_the_ext_record():
    p, keep_alive = _plan()
    y, arr = _layers(norm=1)
    rc, msg = _forward(p, y, _ext(nat.POOL_AVG, fc_norm_w=FAKE, norm_absent=1))
    assert rc == ERR_UNSUPPORTED and WHO in msg and "norm_absent" in msg, msg
    p.act_fp8 = 1                                  # (on a plan the fp8 checks would refuse anyway: this refusal is in front)
    rc, msg = _forward(p, y)
    assert rc == ERR_UNSUPPORTED and WHO in msg and "act_fp8" in msg, msg
    p.act_fp8 = 0
    p.cls_only_last_block = 1
    rc, msg = _forward(p, y)
    assert rc == ERR_INVALID and WHO in msg and "cls_only_last_block" in msg and "block 3" in msg, msg
    y2, arr2 = _layers(blocks=(0, 2))              # earlier captures leave the opt-in alone
    _reaches_the_workspace_check(p, y2)
    p.cls_only_last_block = 0
    # the prefix record is checked under the entry point's name, and the dense size counts its tokens
    rc, msg = _forward(p, y, None, nat.VitPrefix(40, FAKE))
    assert rc == ERR_INVALID and WHO in msg and "num_prefix" in msg, msg
    y3, arr3 = _layers(stride=DENSE)
    rc, msg = _forward(p, y3, None, nat.VitPrefix(5, FAKE))
    assert rc == ERR_INVALID and WHO in msg and "layers.slab_stride" in msg and str(4 * 21 * 128) in msg, msg
    del keep_alive


# ---- the index rule -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("indices, want", [
    (None, tuple(range(12))), (1, (11,)), (4, (8, 9, 10, 11)), ([2, 5, 8, 11], (2, 5, 8, 11)), ([-1], (11,)),
    ((11, 2), (2, 11)), ([-12, -1], (0, 11)), (12, tuple(range(12))),
    ([0, 0], ValueError), ([12], ValueError), ([], ValueError), ([-13], ValueError), (0, ValueError), (13, ValueError),
    ([3, -9], ValueError), ([1.5], ValueError), (True, ValueError),
])
def test_the_index_rule(indices, want):
    if want is ValueError:
        with pytest.raises(ValueError):
            take_indices(12, indices)
    else:
        assert take_indices(12, indices) == want


# ---- wrapper ------------------------------------------------------------------------------------------------------------------

def test_what_the_wrapper_refuses():
    x = torch.zeros(1, 3, 64, 64)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_patch16_64"), SCHED)
    with pytest.raises(NotImplementedError, match="stop_early"):
        w.forward_intermediates(x, stop_early=True)
    for bad in ("first", "", None, 0):
        with pytest.raises(ValueError, match='"zero" or "last"'):
            w.forward_intermediates(x, fill=bad)
    with pytest.raises(ValueError, match="output_fmt"):
        w.forward_intermediates(x, output_fmt="NHWC")
    for bad in ([0, 0], [4], [], 5):
        with pytest.raises(ValueError):
            w.forward_intermediates(x, indices=bad)
        with pytest.raises(ValueError):
            w.get_intermediate_layers(x, n=bad)
    for kw in (dict(), dict(intermediates_only=True), dict(norm=True, fill="last", indices=[1, 3], output_fmt="NLC")):
        with pytest.raises(nat.NativeError):            # a legal call: no CPU fallback, as ever
            w.forward_intermediates(x, **kw)
    with pytest.raises(nat.NativeError):
        w.get_intermediate_layers(x, n=2, reshape=True, return_class_token=True)
    w.set_last_block_cls_only(True)
    with pytest.raises(ValueError, match="set_last_block_cls_only"):
        w.forward_intermediates(x, indices=[1, 3], intermediates_only=True)
    with pytest.raises(nat.NativeError):                # the last block is not captured: the opt-in stays
        w.forward_intermediates(x, indices=[0, 2], intermediates_only=True)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro_fcnorm_patch16_64"), {})
    with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
        w.forward_intermediates(x, norm=True, intermediates_only=True)
    with pytest.raises(NotImplementedError, match="norm is nn.Identity"):
        w.get_intermediate_layers(x)
    with pytest.raises(nat.NativeError):
        w.forward_intermediates(x, norm=False, intermediates_only=True)
    w = rajni_amd.RAJNIViTWrapper(ts.create_model("vit_micro512_patch16_64"), {}).set_weight_format("fp8_mfma")
    with pytest.raises(NotImplementedError, match="fp8_mfma"):
        w.forward_intermediates(x)


# ---- the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64", "vit_micro_prenorm_patch16_64"])
def test_without_a_schedule_the_restatement_is_the_base_models_own_blocks(name):
    cfg = ts.config_of(name)
    model = ts.create_model(name, round_bf16=True, **FIX).double().eval()
    sd = ts.state_dict_numpy(model)
    imgs = images_of(cfg, 3, seed=5)
    blocks = [0, 2, 3]
    with torch.no_grad():
        x = model.norm_pre(model._pos_embed(model.patch_embed(torch.from_numpy(imgs).double())))
        own = {}
        for i, blk in enumerate(model.blocks):
            x = blk(x)
            own[i] = (x.numpy().copy(), model.norm(x).numpy().copy())
    for norm in (False, True):
        for fill in ("zero", "last"):
            r = ny.layers_restated(sd, imgs, {}, cfg, blocks, norm, fill)
            assert r["slabs"].shape == (3, 3, cfg.num_patches + cfg.num_prefix_tokens, cfg.embed_dim)
            assert (r["exit_block"] == cfg.depth).all()
            for l, c in enumerate(blocks):
                want = own[c][int(norm)]
                assert float(np.abs(r["slabs"][l] - want).max()) <= 1e-9 * float(np.abs(want).max()), (norm, fill, c)
    # and the helper the device test normalises norm=False slabs with is the model's norm
    assert float(np.abs(ny.layernorm64(own[3][0], sd, cfg.ln_eps) - own[3][1]).max()) <= 1e-9 * float(np.abs(own[3][1]).max())


@pytest.mark.parametrize("name", ["vit_micro_patch16_64", "vit_micro_reg4_patch16_64"])
def test_with_a_schedule_the_last_slab_is_the_merged_yardsticks(name):
    cfg = ts.config_of(name)
    P, depth = cfg.num_prefix_tokens, cfg.depth
    sd = ts.state_dict_numpy(ts.create_model(name, round_bf16=True, **FIX))
    imgs = images_of(cfg, 3, seed=5)
    last = nl.features_last_restated(sd, imgs, SCHED, cfg)
    feat = nf.features_restated(sd, imgs, SCHED, cfg)
    blocks = [0, 1, 2, 3]
    zero = ny.layers_restated(sd, imgs, SCHED, cfg, blocks, True, "zero")
    full = ny.layers_restated(sd, imgs, SCHED, cfg, blocks, True, "last")
    assert np.array_equal(zero["slabs"][-1], feat["dense"]) and np.array_equal(zero["final"], feat["dense"])
    assert np.array_equal(full["slabs"][-1], last["dense_last"]) and np.array_equal(full["final"], last["dense_last"])
    np.testing.assert_array_equal(full["exit_block"], last["exit_block"])
    ex = full["exit_block"]
    for l, c in enumerate(blocks):
        alive = ex > c
        # alive rows do not depend on the fill; the others are zero, or the entry state of the block that dropped them
        assert np.array_equal(zero["slabs"][l][alive], full["slabs"][l][alive])
        assert not zero["slabs"][l][~alive].any()
        assert (np.abs(full["slabs"][l]).max(axis=-1) > 0.1).all(), "no row is zero"
        for i in (1, 2):
            rows = ex == i
            if i <= c:
                assert np.array_equal(full["slabs"][l][rows], last["entry"][i][rows])
        assert int(alive.sum()) == 3 * (last["counts"][c + 1] if c + 1 < depth else feat["tokens"].shape[1])
    # a block that is both scheduled and captured drops first: slab 1 holds block 1's output for what it kept only
    assert int((ex > 1).sum()) == 3 * last["counts"][2] < 3 * last["counts"][1]
    # norm=False: the same rows before the norm - normalising them in fp64 gives the norm=True slab
    raw = ny.layers_restated(sd, imgs, SCHED, cfg, blocks, False, "last")
    again = ny.layernorm64(raw["slabs"], sd, cfg.ln_eps)
    assert float(np.abs(again - full["slabs"]).max()) <= 1e-9 * float(np.abs(full["slabs"]).max())
    assert (ex[:, :P] == depth).all()
