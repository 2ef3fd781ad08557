"""SwiGLU MLPs (hidden = silu(gate) * value from one packed FC1: timm's GluMlp / SwiGLUPacked / SwiGLU, the DINOv2 giant ViTs)
without a GPU: the ABI the feature must not move, rajni_linear's gated epilogue through the dry run (the plan sees the GEMM that
is computed: 2N rows of W, BN / 2 output columns per tile), the refusals (before any launch: fake addresses nobody follows, the
pattern of tests/test_forward_refusals_cpu.py), the wrapper's recognition and packing of gated MLPs, the synthetic weights, the
restated graph, and the validity of every forward fixture tests/test_gpu_swiglu.py uses.

Two codes differ from the ones first proposed for them, because existing tests hold those values to be UNKNOWN:
tests/test_activations_cpu.py refuses epilogue 17 and mlp_act 2.  The gated epilogue is therefore RAJNI_EPI_BIAS_SWIGLU = 18 and
the forward's value RAJNI_MLP_SWIGLU = 3; 17 and 2 stay unknown, which this file checks too.  For the same reason (the key list
of timm_shaped.CONFIGS is held fixed by tests/test_distilled_cpu.py) the gated configs live in timm_shaped.SWIGLU_CONFIGS."""
import ctypes as C
import dataclasses
import hashlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics_swiglu as ns
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import ops
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper.model import classify_mlp_act, gated_mlp_form

OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 0x10000           # fake addresses, 16-byte aligned, never followed
SW = nat.EPI_BIAS_SWIGLU
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- constants and the header text ----------------------------------------------------------------------------------------

def test_codes_and_the_abi():
    assert nat.ABI_VERSION == 8 and nat.lib().rajni_abi_version() == 8 and nat.NUM_KCLASS == 17
    assert (nat.EPI_BIAS_SWIGLU, nat.MLP_SWIGLU) == (18, 3)
    assert C.sizeof(nat.VitExt) == 72 and nat.VitExt.mlp_act.offset == 68
    text = open(os.path.join(ROOT, "include", "rajni_hip.h")).read()
    assert re.search(r"RAJNI_EPI_BIAS_SWIGLU\s*=\s*18\b", text) and re.search(r"RAJNI_MLP_SWIGLU\s*=\s*3\b", text)
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", text)
    native = open(os.path.join(ROOT, "rajni-vit_amd", "rajni_amd", "_native.py")).read()
    assert re.search(r"EPI_BIAS_SWIGLU\s*=\s*18\b", native) and re.search(r"MLP_SWIGLU\s*=\s*3\b", native)


# ---- rajni_linear: the dry run ----------------------------------------------------------------------------------------------

def linear_args(M, N, K, epilogue, dtype=nat.RAJNI_BF16, w_scale=False, x_scale=False, y_scale=False):
    a = nat.LinearArgs()
    a.x, a.w, a.y, a.bias = PTR, 2 * PTR, 3 * PTR, 4 * PTR
    a.lda, a.ldw, a.ldc, a.ldr = K, K, (N + 15) // 16 * 16, N
    a.M, a.N, a.K, a.epilogue, a.dtype = M, N, K, epilogue, dtype
    a.w_scale = 6 * PTR if w_scale else None
    a.x_scale = 7 * PTR if x_scale else None
    a.y_scale = 8 * PTR if y_scale else None
    return a


def dry_run(a, cus=256, force=0):
    lib = nat.lib()
    out = nat.LinearPlan()
    lib.rajni_debug_force_gemm_tiling(force)
    try:
        rc = lib.rajni_debug_linear_plan(C.byref(a), cus, C.byref(out))
    finally:
        lib.rajni_debug_force_gemm_tiling(0)
    return rc, out, lib.rajni_last_error().decode()


FORMATS = {"bf16": dict(dtype=nat.RAJNI_BF16), "fp16": dict(dtype=nat.RAJNI_F16), "w8": dict(dtype=nat.RAJNI_BF16, w_scale=True)}
cdiv = lambda a, b: (a + b - 1) // b


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("force,tiling,bm,bn", [(1, nat.TILING_SMALL, 128, 128), (4, nat.TILING_WIDE, 256, 256),
                                                (5, nat.TILING_MID, 256, 128)])
def test_a_gated_launch_is_planned_in_tiles_of_half_the_w_rows(force, tiling, bm, bn, fmt):
    """N = 1160, K = 768, M = 394: a tile stages bn rows of W and covers bn / 2 output columns"""
    M, N, K = 394, 1160, 768
    rc, p, msg = dry_run(linear_args(M, N, K, SW, **FORMATS[fmt]), force=force)
    assert rc == OK, msg
    assert p.tiling == tiling and p.tiles_n == cdiv(N, bn // 2) and p.total_tiles == cdiv(N, bn // 2) * cdiv(M, bm)
    # the same W as an ungated [2N, K] launch: as many column tiles (2N / bn = N / (bn / 2) rounded up alike) and N blocks
    rc, q, msg = dry_run(linear_args(M, 2 * N, K, nat.EPI_BIAS_GELU, **FORMATS[fmt]), force=force)
    assert rc == OK and (q.tiling, q.tiles_n, q.total_tiles, q.nblk, q.grid) == (p.tiling, p.tiles_n, p.total_tiles, p.nblk, p.grid)


def test_the_fp32_kernel_plans_half_width_tiles_too():
    rc, p, msg = dry_run(linear_args(394, 1160, 768, SW, dtype=nat.RAJNI_F32))
    assert rc == OK and p.tiling == nat.TILING_F32 and p.tiles_n == cdiv(1160, 64) and p.total_tiles == cdiv(1160, 64) * 4, msg


def test_the_shape_rule_sees_2n_columns_of_w():
    # micro512 FC1 at batch 64: 1088 rows, hidden 1024 -> 2048 rows of W: wide by the N >= 1536 rule, which N = 1024 alone misses
    rc, p, msg = dry_run(linear_args(64 * 17, 1024, 512, SW))
    assert rc == OK and p.tiling == nat.TILING_WIDE and p.tiles_n == 8, msg
    rc, q, _ = dry_run(linear_args(64 * 17, 1024, 512, nat.EPI_BIAS_GELU))
    assert rc == OK and q.tiling == nat.TILING_MID
    # the giant's FC1 (C 1536, hidden 4096) at one 518 px image's 1374 rows
    rc, p, msg = dry_run(linear_args(1374, 4096, 1536, SW))
    assert rc == OK and p.tiling == nat.TILING_WIDE and p.tiles_n == 32 and p.total_tiles == 32 * 6, msg


def test_gated_refusals_of_rajni_linear():
    ok = linear_args(2048, 3072, 1024, nat.EPI_BIAS_GELU, w_scale=True, x_scale=True, y_scale=True)
    assert dry_run(ok)[0] == OK                         # the same call with exact GELU is served
    for y_scale in (False, True):
        rc, _, msg = dry_run(linear_args(2048, 3072, 1024, SW, w_scale=True, x_scale=True, y_scale=y_scale))
        assert rc == UNSUPPORTED and "SwiGLU" in msg and "unsupported" in msg and "x_scale" in msg, msg
    rc, _, msg = dry_run(linear_args(300, 192, 500, SW))
    assert rc == INVALID and "K % 64 == 0" in msg
    rc, _, msg = dry_run(linear_args(300, 192, 512, SW, dtype=nat.RAJNI_F16, w_scale=True))
    assert rc == UNSUPPORTED and "bf16 model" in msg
    for code in (17, 19):                               # the neighbours stay unknown
        rc, _, msg = dry_run(linear_args(300, 192, 512, code))
        assert rc == INVALID and msg == f"rajni_linear: unknown epilogue {code}", msg


# ---- the forward's refusals, before any launch ------------------------------------------------------------------------------

IMAGES, LOGITS = PTR + 0x100, PTR + 0x200


def _plan(act_fp8=0, C_=128, hidden=512, H=2):
    depth = 4
    blocks = (nat.Block * depth)()
    for i in range(depth):
        for name in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
            setattr(blocks[i], name, PTR)
        if act_fp8:
            blocks[i].qkv_s = blocks[i].proj_s = blocks[i].fc1_s = blocks[i].fc2_s = PTR
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = C_, H, 64, depth, hidden, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-6, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, PTR)
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    p.act_fp8 = act_fp8
    return p, blocks


def _forward_ext(p, ext, prefix=False):
    lib = nat.lib()
    if prefix:
        rc = lib.rajni_vit_forward_ext_prefix(C.byref(p), C.byref(ext), None, IMAGES, LOGITS, None)
    else:
        rc = lib.rajni_vit_forward_ext(C.byref(p), C.byref(ext), IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


@pytest.mark.parametrize("prefix", [False, True])
def test_forward_refusals_of_the_gated_mlp_come_before_any_launch(prefix):
    # control: the gated value passes every check up front and stops at the missing workspace - nothing was launched on the way
    p, keep = _plan()
    ext = nat.VitExt()
    ext.mlp_act = nat.MLP_SWIGLU
    rc, msg = _forward_ext(p, ext, prefix)
    assert rc == INVALID and "workspace too small" in msg, msg
    # ... and the workspace of a gated plan is the ungated plan's: the hidden buffer is [rows, hidden] either way
    assert nat.lib().rajni_vit_workspace_bytes(C.byref(p)) == nat.lib().rajni_vit_workspace_bytes(C.byref(_plan()[0]))
    for bad in (2, 4):                                   # unknown values on either side
        p, keep = _plan()
        ext = nat.VitExt()
        ext.mlp_act = bad
        rc, msg = _forward_ext(p, ext, prefix)
        assert rc == INVALID and "mlp_act" in msg and f"({bad})" in msg, msg
    p, keep = _plan(act_fp8=1, C_=512, hidden=2048, H=8)
    ext = nat.VitExt()
    ext.mlp_act = nat.MLP_SWIGLU
    rc, msg = _forward_ext(p, ext, prefix)
    assert rc == UNSUPPORTED and "SwiGLU" in msg and "act_fp8" in msg, msg


def test_last_block_eligibility_does_not_depend_on_the_gate():
    p, keep = _plan()
    ext = nat.VitExt()
    ext.mlp_act = nat.MLP_SWIGLU
    assert nat.lib().rajni_debug_last_block_cls_rows(C.byref(p), C.byref(ext), None) == 1


# ---- the wrapper recognises a gated MLP by structure plus what its activation computes ----------------------------------------

MICRO = "vit_micro_swiglu_patch16_64"


def _wrapped(name=MICRO, sched=None, **kw):
    return rajni_amd.RAJNIViTWrapper(ts.create_model(name, **kw), sched or {})


class MySilu(nn.Module):                    # not nn.SiLU by class, SiLU by what it computes
    def forward(self, x):
        return x * torch.sigmoid(x)


# (the giants are checked by their dims, test_giant_dims: building 1.1 G parameters costs a minute)
@pytest.mark.parametrize("name", [n for n, c in ts.SWIGLU_CONFIGS.items() if c.depth <= 4])
def test_gated_configs_are_accepted(name):
    d = _wrapped(name).check_supported()
    cfg = ts.config_of(name)
    assert d["mlp_act"] == "swiglu" and d["ext"] is True
    assert d["hidden"] == cfg.hidden_dim and d["hidden_pad"] == (cfg.hidden_dim + 63) // 64 * 64
    assert d["num_prefix"] == 1 + cfg.reg_tokens


def test_forms_and_their_refusals():
    w = _wrapped()
    assert gated_mlp_form(w.blocks[0].mlp) == "packed"
    assert gated_mlp_form(_wrapped("vit_micro_swiglu_split_patch16_64").blocks[0].mlp) == "split"
    assert gated_mlp_form(_wrapped("vit_micro_patch16_64").blocks[0].mlp) is None
    for blk in w.blocks:                                 # a module that computes SiLU under another name
        blk.mlp.act = MySilu()
    assert w.check_supported()["mlp_act"] == "swiglu"
    for blk in w.blocks:                                 # gate_last=True is timm's other order: accepted, packed swapped
        blk.mlp.gate_last = True
    assert w.check_supported()["mlp_act"] == "swiglu"
    # GEGLU: a gated MLP with another activation, the class named
    w = _wrapped()
    for blk in w.blocks:
        blk.mlp.act = nn.GELU()
    with pytest.raises(NotImplementedError, match=r"block 0: GluMlp: .*SiLU gate only.*GELU"):
        w.check_supported()
    # an active norm between the gate and fc2, named
    w = _wrapped()
    w.blocks[2].mlp.norm = nn.LayerNorm(256)
    with pytest.raises(NotImplementedError, match=r"block 2: GluMlp: mlp.norm \(LayerNorm\)"):
        w.check_supported()
    # mixed blocks
    w = _wrapped()
    plain = ts.Mlp(128, 256)
    w.blocks[1].mlp = plain
    with pytest.raises(NotImplementedError, match=r"block 1: mlp.act differs between blocks \(gelu after swiglu\)"):
        w.check_supported()
    # a plain (ungated) Mlp whose act is SiLU is still refused, and classify_mlp_act still does not know SiLU
    w = _wrapped("vit_micro_patch16_64")
    for blk in w.blocks:
        blk.mlp.act = nn.SiLU()
    with pytest.raises(NotImplementedError, match=r"block 0: .*SiLU"):
        w.check_supported()
    with pytest.raises(NotImplementedError):
        classify_mlp_act(nn.SiLU())


def test_weight_formats():
    w = _wrapped("vit_micro512_swiglu_patch16_64")
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        w.set_weight_format("fp8_mfma")
    assert w.set_weight_format("fp8")._weight_format == "fp8"
    # the late check: a model that turns gated after the setter accepted fp8_mfma
    w = _wrapped("vit_micro512_patch16_64").set_weight_format("fp8_mfma")
    for blk in w.blocks:
        blk.mlp = ts.GluMlp(512, 1024)
    with pytest.raises(NotImplementedError, match='"fp8_mfma" with a gated'):
        w._pack_weights("cpu", torch.bfloat16)


# ---- packing -------------------------------------------------------------------------------------------------------------------

def test_gate_and_value_rows_of_the_packed_tensor_are_the_source_rows():
    for name in (MICRO, "vit_micro_swiglu_split_patch16_64", "vit_micro_swiglu_h344_patch16_64"):
        w = _wrapped(name, seed=3, std=0.08, bias_std=0.02)
        W = w._pack_weights("cpu", torch.float32)
        hid, hpad = W["desc"]["hidden"], W["desc"]["hidden_pad"]
        for blk, bw in zip(w.blocks, W["blocks"]):
            if hasattr(blk.mlp, "fc1_g"):
                wg, wv, bg, bv = blk.mlp.fc1_g.weight, blk.mlp.fc1_x.weight, blk.mlp.fc1_g.bias, blk.mlp.fc1_x.bias
            else:
                wg, wv, bg, bv = blk.mlp.fc1.weight[:hid], blk.mlp.fc1.weight[hid:], blk.mlp.fc1.bias[:hid], blk.mlp.fc1.bias[hid:]
            f1, b1 = bw["fc1_w"], bw["fc1_b"]
            assert f1.shape == ((2 * hpad + 255) // 256 * 256, 128) and b1.shape == (2 * hpad,)
            assert torch.equal(f1[:hid], wg) and torch.equal(f1[hpad:hpad + hid], wv)
            assert torch.equal(b1[:hid], bg) and torch.equal(b1[hpad:hpad + hid], bv)
            # padding: zero rows and zero bias behind each half (silu(0) * 0 = 0 lands in the hidden buffer's padding columns)
            assert not f1[hid:hpad].any() and not f1[hpad + hid:].any() and not b1[hid:hpad].any() and not b1[hpad + hid:].any()
            assert bw["fc2_w"].shape[1] == hpad and not bw["fc2_w"][:, hid:].any()


def test_h344_fp8_pads_both_halves_with_zero_rows_and_unit_scales():
    w = _wrapped("vit_micro_swiglu_h344_patch16_64", seed=3, std=0.08, bias_std=0.02).to(torch.bfloat16).set_weight_format("fp8")
    W = w._pack_weights("cpu", torch.bfloat16)
    assert (W["desc"]["hidden"], W["desc"]["hidden_pad"]) == (344, 384)
    for blk, bw in zip(w.blocks, W["blocks"]):
        q, s = bw["fc1_w"], bw["fc1_s"]
        assert q.dtype == torch.uint8 and q.shape == (768, 128) and s.shape == (768,)
        assert not q[344:384].any() and not q[384 + 344:].any()
        assert bool((s[344:384] == 1).all()) and bool((s[384 + 344:] == 1).all())
        qg, sg = ops.pack_weight_fp8(blk.mlp.fc1.weight[:344], torch.bfloat16)
        qv, sv = ops.pack_weight_fp8(blk.mlp.fc1.weight[344:], torch.bfloat16)
        assert torch.equal(q[:344], qg[:344]) and torch.equal(q[384:384 + 344], qv[:344])
        assert torch.equal(s[:344], sg) and torch.equal(s[384:384 + 344], sv)
    sd = w.dequantized_state_dict()
    assert sd["blocks.0.mlp.fc1.weight"].shape == (688, 128) and sd["blocks.0.mlp.fc2.weight"].shape == (128, 344)


def test_gate_last_packs_to_the_bytes_of_the_swapped_weights():
    a = _wrapped(seed=3, std=0.08, bias_std=0.02)
    b = _wrapped(seed=3, std=0.08, bias_std=0.02)
    for blk in b.blocks:
        h = blk.mlp.fc2.in_features
        with torch.no_grad():
            blk.mlp.fc1.weight.copy_(torch.cat([blk.mlp.fc1.weight[h:], blk.mlp.fc1.weight[:h]]))
            blk.mlp.fc1.bias.copy_(torch.cat([blk.mlp.fc1.bias[h:], blk.mlp.fc1.bias[:h]]))
        blk.mlp.gate_last = True
    Wa, Wb = a._pack_weights("cpu", torch.float32), b._pack_weights("cpu", torch.float32)
    for x, y in zip(Wa["blocks"], Wb["blocks"]):
        assert torch.equal(x["fc1_w"], y["fc1_w"]) and torch.equal(x["fc1_b"], y["fc1_b"])
    # and timm's gate_last forward is x1 * act(x2): the two models compute different functions of one input unless swapped
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        assert torch.allclose(a.m(x), b.m(x), rtol=0, atol=1e-5)


# ---- configs and the synthetic weights ------------------------------------------------------------------------------------------

# sha256 (16 hex digits) over names and bytes of synth_state_dict(cfg, seed=3, std=0.08, bias_std=0.02) in draw order, computed on
# the parent commit (before `mlp` existed), for EVERY config that commit had (tests/test_distilled_cpu.py's digest)
PARENT = {
    "vit_tiny_patch16_224": "a4f955f0c9977d03",
    "vit_small_patch16_224": "2cf2fd17aaf8e678",
    "vit_base_patch16_224": "75e15e0f1cee5f28",
    "vit_large_patch16_224": "dde976e1fb237d21",
    "vit_large_patch16_384": "fec2a7d4f97895d2",
    "deit3_base_patch16_224": "3c2f272ff90e580f",
    "vit_huge_patch14_224": "807ab7f93141d86a",
    "vit_micro_patch16_64": "0b25e3a4f0eed014",
    "deit3_micro_patch16_64": "c2a3ade870131ac1",
    "vit_micro512_patch16_64": "76d51cf3475f0560",
    "vit_micro_patch14_56": "fdb7bc9ccf0a1882",
    "vit_micro_d80_patch16_64": "84b42027dc237f6e",
    "vit_base_patch16_clip_224": "386edb674a0d1313",
    "vit_base_patch16_qknorm_224": "71fe309bc5363cba",
    "vit_micro_qknorm_patch16_64": "abc4c3af0448ab5f",
    "vit_micro_prenorm_patch16_64": "c32de75e3cca9410",
    "vit_micro_gap_patch16_64": "48516a1362d0fc4c",
    "vit_micro_fcnorm_patch16_64": "48516a1362d0fc4c",
    "vit_micro_all_patch16_64": "72a7b0e3144ff4ff",
    "vit_micro512_qknorm_patch16_64": "b3cca53cd33aea80",
    "vit_micro_d80_qknorm_patch16_64": "c9caaa8122056269",
    "vit_micro_reg4_patch16_64": "094ee1c5866ac488",
    "deit3_micro_reg4_patch16_64": "4f600a2150cd962c",
    "vit_micro_reg1_gap_patch14_56": "3d481281f0f5e16d",
    "vit_micro512_reg4_patch16_64": "96f85af0065b443a",
    "vit_small_patch14_reg4_dinov2": "f677e4ad0825ea0c",
    "vit_small_patch14_reg4_dinov2_518": "ded8a733c35d87eb",
    "vit_micro_patch16_400": "f1f2e604265d268c",
    "vit_micro_reg4_patch16_400": "c5f5c2d5f35ab936",
    "vit_base_patch16_clip_quickgelu_224": "386edb674a0d1313",
    "vit_base_patch32_clip_quickgelu_224": "06ed4f6cec2776e2",
    "vit_large_patch14_clip_quickgelu_224": "aab0cac0f767537b",
    "vit_micro_quickgelu_patch16_64": "0b25e3a4f0eed014",
    "vit_micro_clip_quickgelu_patch16_64": "c32de75e3cca9410",
    "vit_micro512_quickgelu_patch16_64": "76d51cf3475f0560",
    "vit_micro_quickgelu_h344_patch16_64": "9dded809342dd903",
    "deit_tiny_distilled_patch16_224": "6efb4632b6437ab1",
    "deit_small_distilled_patch16_224": "f433094cbb8905ce",
    "deit_base_distilled_patch16_224": "23fb74ec36848434",
    "deit_base_distilled_patch16_384": "95ade2e9c44322e3",
    "vit_micro_distilled_patch16_64": "cc10fb8968b5dafd",
    "vit_micro512_distilled_patch16_64": "ce9b473de8925160",
}


def sd_hash(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def test_the_config_tables():
    assert list(ts.CONFIGS) == list(PARENT)
    assert list(ts.SWIGLU_CONFIGS) == ["vit_giant_patch14_dinov2", "vit_giant_patch14_reg4_dinov2", "vit_micro_swiglu_patch16_64",
                                       "vit_micro_swiglu_split_patch16_64", "vit_micro_swiglu_h344_patch16_64",
                                       "vit_micro512_swiglu_patch16_64", "vit_micro_reg4_swiglu_patch14_56"]
    assert all(c.mlp == "mlp" for c in ts.CONFIGS.values())
    assert all(c.mlp in ("swiglu_packed", "swiglu") and c.act == "gelu" for c in ts.SWIGLU_CONFIGS.values())
    fields = [f.name for f in dataclasses.fields(ts.ViTConfig)]
    assert fields[-4:] == ["mlp", "distilled", "act", "reg_tokens"] and ts.ViTConfig().mlp == "mlp"
    with pytest.raises(ValueError):
        ts.ViTConfig(mlp="geglu")
    with pytest.raises(KeyError):
        ts.config_of("no_such_model")


@pytest.mark.parametrize("name", list(PARENT))
def test_existing_configs_keep_their_weight_stream(name):
    sd = ts.synth_state_dict(ts.CONFIGS[name], seed=3, std=0.08, bias_std=0.02)
    assert sd_hash(sd) == PARENT[name]
    assert not any("fc1_g" in k or "fc1_x" in k for k in sd)


def test_giant_dims():
    for name, reg in (("vit_giant_patch14_dinov2", 0), ("vit_giant_patch14_reg4_dinov2", 4)):
        c = ts.config_of(name)
        assert (c.img_size, c.patch_size, c.embed_dim, c.depth, c.num_heads) == (518, 14, 1536, 40, 24)
        assert c.hidden_dim == 4096 and c.head_dim == 64 and c.layer_scale and c.mlp == "swiglu_packed" and c.reg_tokens == reg
        assert c.num_patches + c.num_prefix_tokens == 1369 + 1 + reg
    assert ts.config_of("vit_giant_patch14_reg4_dinov2").no_embed_class
    blk = ts.Block(ts.config_of("vit_giant_patch14_dinov2"))
    assert blk.mlp.fc1.weight.shape == (8192, 1536) and blk.mlp.fc2.weight.shape == (1536, 4096)


def test_micro_dims_and_modules():
    for name, hid in (("vit_micro_swiglu_patch16_64", 256), ("vit_micro_swiglu_split_patch16_64", 256),
                      ("vit_micro_swiglu_h344_patch16_64", 344), ("vit_micro_reg4_swiglu_patch14_56", 256)):
        c = ts.config_of(name)
        assert (c.embed_dim, c.depth, c.num_heads, c.num_classes, c.hidden_dim) == (128, 4, 2, 10, hid)
    c = ts.config_of("vit_micro512_swiglu_patch16_64")
    assert (c.embed_dim, c.num_heads, c.hidden_dim, c.num_patches + 1) == (512, 8, 1024, 17)
    c = ts.config_of("vit_micro_reg4_swiglu_patch14_56")
    assert c.patch_size == 14 and c.reg_tokens == 4 and c.layer_scale and c.no_embed_class
    m = ts.create_model(MICRO).blocks[0].mlp
    assert [n for n, _ in m.named_children()] == ["fc1", "act", "drop1", "norm", "fc2", "drop2"] and m.gate_last is False
    assert isinstance(m.act, nn.SiLU) and m.fc1.out_features == 512 and m.fc2.in_features == 256
    m = ts.create_model("vit_micro_swiglu_split_patch16_64").blocks[0].mlp
    assert [n for n, _ in m.named_children()] == ["fc1_g", "fc1_x", "act", "drop1", "norm", "fc2", "drop2"]
    sd = ts.synth_state_dict(ts.config_of("vit_micro_reg4_swiglu_patch14_56"), seed=1)
    assert list(sd)[-1] == "reg_token" and sd["blocks.0.mlp.fc1.weight"].shape == (512, 128)


# ---- the restated graph and the forward fixtures ------------------------------------------------------------------------------------

def test_silu_slope_and_the_functions():
    assert abs(ns.silu_slope() - 1.0998) < 1e-3
    x = np.float64([-800.0, -1.0, 0.0, 1.0, 800.0])
    got = ns.silu64(x)
    assert np.isfinite(got).all() and got[2] == 0.0 and got[0] == 0.0 and got[-1] == 800.0
    t = torch.linspace(-20, 20, 4001, dtype=torch.float64)
    assert np.abs(ns.silu64(t.numpy()) - torch.nn.functional.silu(t).numpy()).max() < 1e-14


@pytest.mark.parametrize("name", list(ns.FORWARD_CASES))
def test_restated_graph_agrees_with_the_module_in_fp64(name):
    cfg = ts.config_of(name)
    model = ts.create_model(cfg, round_bf16=True, **ns.fix_of(name)).double()
    sd = {k: v.detach().numpy() for k, v in model.state_dict().items()}
    imgs = ns.images_of(cfg, 3, 2)
    got, counts, _ = ns.vit_forward_restated(sd, imgs, {}, cfg)
    with torch.no_grad():
        stock = model(torch.from_numpy(imgs).double()).numpy()
    assert counts == [cfg.num_patches + cfg.num_prefix_tokens] * cfg.depth
    assert np.abs(got - stock).max() <= 1e-12 * np.abs(stock).max()


@pytest.mark.parametrize("name", list(ns.FORWARD_CASES))
def test_fixtures_can_tell_and_seeds_follow_the_rule(name):
    """every forward fixture of tests/test_gpu_swiglu.py, on the CPU: each mistake (halves swapped, gate dropped; selections held
    fixed) moves the fp32 logits by at least 5 x the fp32 bar, the bf16 format alone stays within 0.75 x the 1e-2 bar, and the
    recorded seed is the first from 1 up with both properties"""
    ok, figures = ns.seed_passes(name, ns.SEEDS[name])
    for (pruned, B, iseed), (a, b, c) in zip(ns.FORWARD_CASES[name], figures):
        print(f"[swiglu] {name} pruned={pruned} B={B} images {iseed}: swapped halves move the fp32 logits by {a:.3g} of their scale, "
              f"dropping the gate by {b:.3g} (need 5e-3); an ideal bf16 forward costs {c / 1e-2:.2f} x the 1e-2 bar")
        assert a >= 5e-3 and b >= 5e-3 and c <= ns.FORMAT_HEADROOM * 1e-2
    assert ok and ns.first_seed(name) == ns.SEEDS[name]
