"""The placement contract (include/rajni_hip.h, "placement") on the host: every entry point accepts each of its pointers at the
stated minimum alignment and refuses it at half of that, by name, before anything is launched; the table of tests/placement.py
is the header's; the forward refuses a misplaced workspace or weight ahead of "workspace too small"; the helper of
rajni_amd/ops.py moves a read-only operand that sits below the contract and refuses one it would have to write.

No GPU and nothing launched: the addresses are fakes nobody follows.  Every call is shaped so that, once its pointers pass,
it stops at a later refusal of its own (a head dim of 12, a row of 8 bytes, more scores than LDS holds, a missing
workspace); rajni_linear goes through its dry-run hook."""
import ctypes as C

import pytest
import torch

import placement as pl
from rajni_amd import _native as nat
from rajni_amd import ops

BASE = 0x100000        # 256-byte aligned; pointer k of a call sits at BASE + k * 0x1000
OK, INVALID, UNSUPPORTED = 0, 1, 2
BF16, F32 = nat.RAJNI_BF16, nat.RAJNI_F32
ELEM_BYTES = {BF16: 2, F32: 4}


def _err():
    return nat.lib().rajni_last_error().decode()


# ---- one call per entry point: p maps each pointer of placement.CONTRACT[entry] to its address ----------------------------------
def _linear(p, dtype):
    a = nat.LinearArgs()
    for name in pl.CONTRACT["rajni_linear"]:
        setattr(a, name, p[name])
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.ldr = 300, 328, 512, 512, 512, 336, 328
    a.r_np, a.r_nsrc = 75, 90
    a.epilogue, a.dtype = nat.EPI_BIAS_RESID, BF16      # fp8 x fp8 RESID: the one form that takes all but y_scale ...
    if p.get("want_y_scale"):
        a.epilogue, a.resid, a.gamma, a.r_idx = nat.EPI_BIAS_GELU, None, None, None    # ... and GELU -> e4m3 takes y_scale
    else:
        a.y_scale = None
    out = nat.LinearPlan()
    return nat.lib().rajni_debug_linear_plan(C.byref(a), 256, C.byref(out))


def _plan(p, dtype):
    """the micro plan of tests/test_forward_refusals_cpu.py with its pointers from p (plan, block 1, ext, prefix, images, logits)"""
    depth = 4
    blocks = (nat.Block * depth)()
    for i in range(depth):
        for name in pl.CONTRACT["rajni_block"]:
            setattr(blocks[i], name, p[name] if i == 1 else (BASE if name not in ("forced_keep_idx", "scores") else None))
        blocks[i].keep = (0, 8, 6, 0)[i]
    plan = nat.VitPlan()
    plan.dtype, plan.B, plan.in_chans, plan.img_size, plan.patch_size = dtype, 4, 3, 64, 16
    plan.C, plan.H, plan.D, plan.depth, plan.hidden, plan.num_classes = 128, 2, 64, depth, 512, 16
    plan.ln_eps, plan.attn_scale, plan.pos_has_cls = 1e-6, 0.125, 1
    for name in pl.CONTRACT["rajni_vit_plan"]:
        setattr(plan, name, p[name])
    plan.blocks, plan.workspace_bytes, plan.logits_ld = blocks, 0, 24
    qk = (nat.QkAffine * depth)()
    for i in range(depth):
        for name in pl.CONTRACT["rajni_qk_affine"]:
            setattr(qk[i], name, p[name] if i == 2 else BASE)
    ext = nat.VitExt()
    ext.qk_norm, ext.qk_eps = qk, 1e-6
    for name in pl.CONTRACT["rajni_vit_ext"]:
        setattr(ext, name, p[name])
    pre = nat.VitPrefix()
    pre.num_prefix, pre.reg_token = 5, p["reg_token"]
    return nat.lib().rajni_vit_forward_ext_prefix(C.byref(plan), C.byref(ext), C.byref(pre), p["images"], p["logits"], None)


L = nat.lib
CALLS = {
    # D = 12: "head dim 12 not supported"
    "rajni_importance": lambda p, dt: L().rajni_importance(p["qkv"], p["scores_out"], 1, 4, 2, 12, 1e-6, dt, None),
    "rajni_score_select": lambda p, dt: L().rajni_score_select(p["qkv"], 1, 4, 2, 12, 1e-6, 1, p["scores_out"], p["keep_idx"],
                                                               p["next_scores"], dt, None),
    "rajni_score_select_prefix": lambda p, dt: L().rajni_score_select_prefix(p["qkv"], 1, 8, 2, 12, 1e-6, 2, 1, p["scores_out"],
                                                                             p["keep_idx"], p["next_scores"], dt, None),
    "rajni_score_select_ws": lambda p, dt: L().rajni_score_select_ws(p["qkv"], 1, 8, 2, 12, 1e-6, 2, 1, p["scores_out"], p["keep_idx"],
                                                                     p["next_scores"], dt, p["workspace"], 1 << 30, None),
    # 200000 scores: more than one workgroup's LDS holds
    "rajni_select_topk": lambda p, dt: L().rajni_select_topk(p["scores"], 1, 200000, 1, p["keep_idx"], p["next_scores"], dt, None),
    "rajni_select_topk_prefix": lambda p, dt: L().rajni_select_topk_prefix(p["scores"], 1, 200000, 2, 1, p["keep_idx"],
                                                                           p["next_scores"], dt, None),
    # rows of 4 elements: not a multiple of 16 bytes
    "rajni_gather_rows": lambda p, dt: L().rajni_gather_rows(p["src"], p["idx"], p["dst"], 1, 4, 2, 2, dt, None),
    "rajni_attention": lambda p, dt: L().rajni_attention(p["qkv"], p["keep_idx"], p["out"], 1, 8, 4, 2, 12, 0.3, dt, None),
    "rajni_attention_fp8": lambda p, dt: L().rajni_attention_fp8(p["qkv"], p["keep_idx"], p["out_q"], 1.0, p["row_scale"], 1, 8, 4, 2,
                                                                 32, 0.2, None),
    # C = 12
    "rajni_layernorm": lambda p, dt: L().rajni_layernorm(p["x"], 16, p["w"], p["b"], p["y"], 3, 12, 1e-6, dt, 0, None),
    "rajni_layernorm_fp8": lambda p, dt: L().rajni_layernorm_fp8(p["x"], 16, p["w"], p["b"], p["y_q"], p["y_scale"], p["hid_scale"],
                                                                 1.0, 1.0, 3, 12, 1e-6, 0, None),
    "rajni_linear": _linear,
    # a 16-pixel patch does not divide a 60-pixel image
    "rajni_patch_embed": lambda p, dt: L().rajni_patch_embed(p["images"], p["w"], p["bias"], p["cls"], p["pos"], 1, p["x"], 0, 1, 3, 60,
                                                             16, 64, dt, p["workspace"], 1 << 20, None),
    "rajni_patch_embed_prefix": lambda p, dt: L().rajni_patch_embed_prefix(p["images"], p["w"], p["bias"], p["cls"], p["reg"], 3, p["pos"],
                                                                           1, p["x"], 0, 1, 3, 60, 16, 64, dt, p["workspace"], 1 << 20,
                                                                           None),
    "rajni_qk_norm": lambda p, dt: L().rajni_qk_norm(p["qkv"], p["q_w"], p["q_b"], p["k_w"], p["k_b"], 3, 2, 12, 1e-6, dt, None),
    "rajni_layernorm_stream": lambda p, dt: L().rajni_layernorm_stream(p["x"], p["w"], p["b"], 3, 12, 1e-6, dt, 0, None),
    "rajni_pool_norm": lambda p, dt: L().rajni_pool_norm(p["x"], 2, 5, 12, 0, p["norm_w"], p["norm_b"], 1e-6, p["fc_w"], p["fc_b"], 1e-6,
                                                         p["out"], dt, 0, None),
    "rajni_pool_norm_prefix": lambda p, dt: L().rajni_pool_norm_prefix(p["x"], 2, 9, 3, 12, 1, p["norm_w"], p["norm_b"], 1e-6, p["fc_w"],
                                                                       p["fc_b"], 1e-6, p["out"], dt, 0, None),
}
# the forward takes the pointers of five records in one call, with a NULL workspace: it stops at "workspace too small"
FORWARD = ("rajni_vit_forward", "rajni_vit_plan", "rajni_block", "rajni_qk_affine", "rajni_vit_ext", "rajni_vit_prefix")
LATER = {     # entry point -> (code, piece of the message) of the refusal a call with legal pointers stops at
    "rajni_importance": (UNSUPPORTED, "head dim 12"), "rajni_score_select": (UNSUPPORTED, "head dim 12"),
    "rajni_score_select_prefix": (UNSUPPORTED, "head dim 12"), "rajni_score_select_ws": (UNSUPPORTED, "head dim 12"),
    "rajni_select_topk": (UNSUPPORTED, "of LDS"), "rajni_select_topk_prefix": (UNSUPPORTED, "of LDS"),
    "rajni_gather_rows": (INVALID, "row bytes must be a multiple of 16"),
    "rajni_attention": (UNSUPPORTED, "head dim"), "rajni_attention_fp8": (UNSUPPORTED, "ead dim 64"),
    "rajni_layernorm": (UNSUPPORTED, "C=12"), "rajni_layernorm_fp8": (UNSUPPORTED, "C=12"),
    "rajni_linear": (OK, ""),
    "rajni_patch_embed": (INVALID, "the patch size must divide the image"),
    "rajni_patch_embed_prefix": (INVALID, "the patch size must divide the image"),
    "rajni_qk_norm": (UNSUPPORTED, "D=12"), "rajni_layernorm_stream": (UNSUPPORTED, "C=12"),
    "rajni_pool_norm": (UNSUPPORTED, "C=12"), "rajni_pool_norm_prefix": (UNSUPPORTED, "C=12"),
}


def _pointers(entry, dtype, shift=None):
    """every pointer of the call on its own 256-byte boundary; `shift` = (record, name, bytes) moves one of them"""
    records = FORWARD if entry in FORWARD else (entry,)
    p, k = {}, 0
    for rec in records:
        for name in pl.CONTRACT[rec]:
            k += 1
            p[name] = BASE + k * 0x1000 + (shift[2] if shift and shift[:2] == (rec, name) else 0)
    if entry in FORWARD and not (shift and shift[1] == "workspace"):
        p["workspace"] = None
    return p


def _call(entry, dtype, shift=None):
    p = _pointers(entry, dtype, shift)
    if entry == "rajni_linear" and shift and shift[1] == "y_scale":
        p["want_y_scale"] = True
    rc = (_plan if entry in FORWARD else CALLS[entry])(p, dtype)
    return rc, _err()


def _accepted(entry, rc, msg):
    if entry in FORWARD:
        assert rc == INVALID and "workspace too small" in msg, (entry, rc, msg)
    else:
        code, piece = LATER[entry]
        assert rc == code and piece in msg and "aligned" not in (msg if rc else ""), (entry, rc, msg)


CASES = [(entry, name, dtype) for entry, ptrs in pl.CONTRACT.items() for name, a in ptrs.items()
         for dtype in ((BF16, F32) if a == pl.ELEM else (BF16,))]


def test_the_table_is_the_headers():
    """tests/placement.py covers exactly the entry points and pointers of the header's table, at the same minimums"""
    header = pl.parse_header()
    assert list(header) == list(pl.CONTRACT)
    for entry, ptrs in header.items():
        assert ptrs == pl.CONTRACT[entry], entry
    assert set(CALLS) | set(FORWARD) == set(pl.CONTRACT)


def test_every_table_entry_is_an_exported_entry_point_or_a_plan_record():
    records = {"rajni_vit_plan", "rajni_block", "rajni_qk_affine", "rajni_vit_ext", "rajni_vit_prefix"}
    for entry in pl.CONTRACT:
        assert entry in records or entry in nat.EXPORTED_SYMBOLS, entry
    checked = {e for e in nat.EXPORTED_SYMBOLS if "debug" not in e and "profile" not in e and "bytes" not in e
               and e not in ("rajni_abi_version", "rajni_last_error", "rajni_device_check")}
    forwards = {"rajni_vit_forward", "rajni_vit_forward_ext", "rajni_vit_forward_ext_prefix"}      # one table line for the three
    assert checked - forwards == set(pl.CONTRACT) - records - forwards


@pytest.mark.parametrize("entry,name,dtype", CASES, ids=[f"{e}-{n}-{'f32' if d == F32 else 'bf16'}" for e, n, d in CASES])
def test_minimum_is_accepted_and_half_of_it_refused_by_name(entry, name, dtype):
    a = pl.min_align(entry, name, ELEM_BYTES[dtype])
    rc, msg = _call(entry, dtype)                                   # control: everything on a 256-byte boundary
    _accepted(entry, rc, msg)
    if name == "workspace" and entry == "rajni_vit_plan":
        # a non-null workspace at its minimum passes the placement check and is then too small (0 bytes)
        rc, msg = _call(entry, dtype, (entry, name, 0))
        assert rc == INVALID and "workspace too small" in msg, msg
    elif a < 256:
        rc, msg = _call(entry, dtype, (entry, name, a))             # a 256-byte boundary plus the minimum
        _accepted(entry, rc, msg)
    rc, msg = _call(entry, dtype, (entry, name, a // 2))
    assert rc == INVALID, (rc, msg)
    if entry == "rajni_linear" and name in ("x", "w", "y", "resid"):
        assert msg == f"rajni_linear: pointers must be 16-byte aligned ({name})", msg
    else:
        assert f"{name} must be {a}-byte aligned" in msg, msg
        if entry == "rajni_block":
            assert "block 1" in msg, msg
        if entry == "rajni_qk_affine":
            assert "block 2" in msg, msg


def test_forward_refuses_a_workspace_base_at_plus_16_up_front():
    rc, msg = _call("rajni_vit_plan", BF16, ("rajni_vit_plan", "workspace", 16))
    assert rc == INVALID and msg == "rajni_vit_forward: workspace must be 256-byte aligned", msg


def test_forward_refuses_an_unaligned_weight_ahead_of_the_workspace_size():
    """the plain rajni_vit_forward of tests/test_forward_refusals_cpu.py::_control with fc2_w of block 2 eight bytes off"""
    import test_forward_refusals_cpu as fr
    fr._control()
    p, blocks = fr._plan(keeps=(0, 8, 6, 0), buffers=(1, 2))
    blocks[2].fc2_w = fr.FAKE + 8
    rc, msg = fr._forward(p)
    assert rc == INVALID and msg == "rajni_vit_forward: block 2: fc2_w must be 16-byte aligned", msg
    blocks[2].fc2_w = fr.FAKE
    rc, msg = fr._forward(p)
    assert rc == INVALID and "workspace too small" in msg, msg


# ---- rajni_amd.ops._placed on CPU tensors --------------------------------------------------------------------------------------
def _offset_view(dtype=torch.float32, rows=6, cols=8):
    buf = torch.arange(1 + rows * cols, dtype=torch.float32).to(dtype)
    v = buf[1:].view(rows, cols)
    assert v.is_contiguous() and v.storage_offset() == 1 and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8])
def test_an_offset_view_is_cloned_to_the_contract(dtype):
    v = _offset_view(dtype)
    got = ops._placed(v, "x")
    assert got is not v and got.data_ptr() % 16 == 0 and got.is_contiguous() and torch.equal(got, v)
    assert got.untyped_storage().data_ptr() != v.untyped_storage().data_ptr()


def test_an_aligned_tensor_is_returned_as_it_is():
    t = torch.zeros(6, 8)
    assert t.data_ptr() % 16 == 0
    assert ops._placed(t, "x") is t and ops._placed(t, "qkv", in_place=True) is t
    assert ops._placed(None, "bias") is None
    i = torch.zeros(9, dtype=torch.int32)[1:]                       # 4 bytes past the allocation: legal for an index array
    assert ops._placed(i, "keep_idx", 4) is i


def test_an_offset_in_place_operand_raises():
    v = _offset_view()
    with pytest.raises(ValueError, match="qkv must be 16-byte aligned"):
        ops._placed(v, "qkv", in_place=True)
    with pytest.raises(ValueError, match="must be contiguous"):
        ops._placed(torch.zeros(4, 8).t(), "x", in_place=True)
