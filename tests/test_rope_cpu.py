"""Rotary position embeddings (include/rajni_hip_rope.h) without a GPU: the record's layout against the header and the ABI the
feature must not move, the refusals of the forward and of rajni_rope_qk (before any launch: every plan here has workspace = NULL
and fake addresses nobody follows, the pattern of tests/test_rmsnorm_cpu.py), the timm-shaped Attention against the rule, the
wrapper's recognition of a rotary module, the synthetic weights, and the validity of the forward fixtures: on every fixture the
GPU forward tests use, each mutant of the restated forward moves the logits by at least 4 x the GPU tests' bar."""
import ctypes as C
import dataclasses
import hashlib
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import numerics_rope as nrp
import rajni_amd
from rajni_amd import _native as nat
from rajni_amd import timm_shaped as ts
from rajni_amd.wrapper.model import classify_rope_embed, rope_layout, rope_tables

OK, INVALID, UNSUPPORTED = 0, 1, 2
PTR = 0x10000           # fake addresses, 16-byte aligned, never followed
IMAGES, LOGITS = PTR + 0x100, PTR + 0x200
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rajni_hip_rope.h")).read()


# ---- the record and the ABI ------------------------------------------------------------------------------------------------

def test_record_layout_matches_the_header():
    body = re.search(r"typedef struct \{(.*?)\} rajni_vit_rope;", HEADER, re.S).group(1)
    names = re.findall(r"(?:int|long long|const float\*)\s+(\w+);", body)
    assert names == [n for n, _ in nat.VitRope._fields_] == ["cos", "sin", "head_stride", "block_stride", "rows", "layout"]
    assert C.sizeof(nat.VitRope) == 40
    assert [getattr(nat.VitRope, n).offset for n in names] == [0, 8, 16, 24, 32, 36]
    assert re.search(r"RAJNI_ROPE_INTERLEAVED\s*=\s*0\s*,\s*RAJNI_ROPE_HALF\s*=\s*1\b", HEADER)
    assert (nat.ROPE_INTERLEAVED, nat.ROPE_HALF) == (0, 1) == (nrp.INTERLEAVED, nrp.HALF)
    assert '#include "rajni_hip_norm.h"' in HEADER and "(end of the placement table)" in HEADER
    table = HEADER[HEADER.index("---- placement"):HEADER.index("(end of the placement table)")]
    rows = dict(re.findall(r"^ \*   (rajni_\w+): (.+)$", table, re.M))
    assert rows["rajni_rope_qk"] == "qkv 16, src 4, cos 16, sin 16" and rows["rajni_vit_rope"] == "cos 16, sin 16"
    assert "DOES NOT VALIDATE src" in HEADER


def test_symbols_resolve_and_the_abi_stays_where_it_is():
    lib = nat.lib()
    assert nat.ROPE_SYMBOLS == ("rajni_rope_qk", "rajni_vit_workspace_bytes_rope", "rajni_vit_forward_rope")
    for sym in nat.ROPE_SYMBOLS:
        assert getattr(lib, sym).argtypes is not None
    assert nat.ABI_VERSION == 8 and lib.rajni_abi_version() == 8 and nat.NUM_KCLASS == 17
    assert not set(nat.ROPE_SYMBOLS) & set(nat.EXPORTED_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "rajni_hip.h")).read() + open(os.path.join(ROOT, "include", "rajni_hip_debug.h")).read()
    declared = set(re.findall(r"\b(rajni_\w+)\s*\(", main))
    assert set(nat.EXPORTED_SYMBOLS) <= declared and not set(nat.ROPE_SYMBOLS) & declared
    assert re.search(r"#define RAJNI_ABI_VERSION 8\b", main)
    # every record that existed keeps its size
    sizes = {nat.VitExt: 72, nat.VitPrefix: 16, nat.VitImage: 8, nat.VitQuery: 8, nat.VitNorm: 24, nat.VitLayers: 40}
    assert {k.__name__: C.sizeof(k) for k in sizes} == {k.__name__: v for k, v in sizes.items()}
    assert C.sizeof(nat.VitPlan) == 168 and C.sizeof(nat.Block) == 200 and C.sizeof(nat.VitAttnPool) == 112 and C.sizeof(nat.LinearArgs) == 144


# ---- the forward's refusals, before any launch ---------------------------------------------------------------------------

def _plan(act_fp8=0, C_=128, hidden=512, H=2):
    depth = 4
    blocks = (nat.Block * depth)()
    for i in range(depth):
        for name, _ in nat.Block._fields_[:14]:          # the weights
            setattr(blocks[i], name, PTR)
        if act_fp8:
            blocks[i].qkv_s = blocks[i].proj_s = blocks[i].fc1_s = blocks[i].fc2_s = PTR
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = C_, H, 64, depth, hidden, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-5, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, PTR)
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    p.act_fp8 = act_fp8
    return p, blocks


def _rope(rows=16, D=64, H=2, per_head=False, per_block=False, layout=0):
    r = nat.VitRope()
    r.cos, r.sin, r.rows, r.layout = PTR, PTR + 0x1000, rows, layout
    r.head_stride = rows * D if per_head or per_block else 0
    r.block_stride = H * rows * D if per_block else 0
    return r


def _forward(p, rope, pre=None, img=None):
    lib = nat.lib()
    ref = lambda r: C.byref(r) if r is not None else None
    rc = lib.rajni_vit_forward_rope(C.byref(p), None, ref(pre), None, ref(img), None, None, None, ref(rope), IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error().decode()


def _size(p, rope, pre=None, img=None):
    ref = lambda r: C.byref(r) if r is not None else None
    return nat.lib().rajni_vit_workspace_bytes_rope(C.byref(p), ref(pre), ref(img), None, None, None, ref(rope))


def test_a_valid_plan_stops_at_the_workspace_and_the_map_is_all_the_record_adds():
    # the control: every check passes in each table form and layout, and nothing was launched on the way
    base = nat.lib().rajni_vit_workspace_bytes(C.byref(_plan()[0]))
    for kw in (dict(), dict(per_head=True), dict(per_block=True), dict(layout=1)):
        p, keep = _plan()
        rc, msg = _forward(p, _rope(**kw))
        assert rc == INVALID and "workspace too small" in msg, msg
        assert _size(p, _rope(**kw)) == base + (4 * 17 * 4 + 255) // 256 * 256          # B * n0 * 4 bytes, whole 256-byte units
    p, keep = _plan()
    assert _size(p, None) == _size(p, nat.VitRope()) == base
    # the record composes with a prefix and an image record: rows follow the grid and P
    p, keep = _plan()
    pre = nat.VitPrefix(5, PTR)
    rc, msg = _forward(p, _rope(rows=16), pre=pre)
    assert rc == INVALID and "workspace too small" in msg, msg
    p.img_size = 48
    rc, msg = _forward(p, _rope(rows=18), pre=pre, img=nat.VitImage(48, 96))
    assert rc == INVALID and "workspace too small" in msg, msg


@pytest.mark.parametrize("bad", [2, -1, 7])
def test_an_unknown_layout_is_invalid(bad):
    p, keep = _plan()
    rc, msg = _forward(p, _rope(layout=bad))
    assert rc == INVALID and msg == f"rajni_vit_forward_rope: rope.layout must be RAJNI_ROPE_INTERLEAVED or RAJNI_ROPE_HALF ({bad})", msg
    assert _size(p, _rope(layout=bad)) == 0 and "rope.layout" in nat.lib().rajni_last_error().decode()


def test_refused_records_name_themselves():
    # NULL cos or sin with a non-zero record
    for name in ("cos", "sin"):
        p, keep = _plan()
        r = _rope()
        setattr(r, name, None)
        rc, msg = _forward(p, r)
        assert rc == INVALID and f"null pointer (rope.{name}) with a non-zero rope record" in msg, msg
    # rows against the grid: 16 patches at 64 px, whatever the prefix count; 18 at 48 x 96
    for rows, pre, img, n in ((15, None, None, 16), (17, None, None, 16), (21, nat.VitPrefix(5, PTR), None, 16),
                              (16, None, nat.VitImage(48, 96), 18)):
        p, keep = _plan()
        if img is not None:
            p.img_size = 48
        rc, msg = _forward(p, _rope(rows=rows), pre=pre, img=img)
        assert rc == INVALID and f"rope.rows must equal the patches of the grid, n0 - P = {n} ({rows})" in msg, msg
    # strides: exactly the two values each
    for hs in (64, 16 * 64 + 8, -16 * 64, 2 * 16 * 64):
        p, keep = _plan()
        r = _rope()
        r.head_stride = hs
        rc, msg = _forward(p, r)
        assert rc == INVALID and f"rope.head_stride must be 0 (one table for all heads) or rows * D = 1024 ({hs})" in msg, msg
    for per_head, bs, want in ((False, 2 * 1024, 1024), (True, 1024, 2048), (True, 4096, 2048), (False, -1024, 1024)):
        p, keep = _plan()
        r = _rope(per_head=per_head)
        r.block_stride = bs
        rc, msg = _forward(p, r)
        assert rc == INVALID and f"rope.block_stride must be 0 (one table for all blocks) or (head_stride ? H : 1) * rows * D = {want} ({bs})" in msg, msg
    # act_fp8
    p, keep = _plan(act_fp8=1, C_=512, hidden=2048, H=8)
    rc, msg = _forward(p, _rope(H=8))
    assert rc == UNSUPPORTED and "RoPE" in msg and "plan.act_fp8" in msg, msg
    rc, msg = _forward(p, None)          # (the control: the same plan without the record is served)
    assert rc == INVALID and "workspace too small" in msg, msg
    # placement of the record's own pointers
    for name in ("cos", "sin"):
        p, keep = _plan()
        r = _rope()
        setattr(r, name, PTR + 4)
        rc, msg = _forward(p, r)
        assert rc == INVALID and f"{name} must be 16-byte aligned" in msg, msg
    # check_all order: the layout in front of the pointers, the pointers in front of the rows, the rows in front of the strides,
    # the record in front of the plan's own refusals
    p, keep = _plan()
    r = _rope(layout=5, rows=3)
    r.cos, r.head_stride = None, 7
    p.C = 100
    seen = []
    for fix in (lambda: setattr(r, "layout", 1), lambda: setattr(r, "cos", PTR), lambda: setattr(r, "rows", 16),
                lambda: setattr(r, "head_stride", 0), lambda: setattr(p, "C", 128)):
        seen.append(_forward(p, r)[1])
        fix()
    assert ["rope.layout" in seen[0], "rope.cos" in seen[1], "rope.rows" in seen[2], "rope.head_stride" in seen[3],
            "need C == H*D" in seen[4]] == [True] * 5, seen
    assert "workspace too small" in _forward(p, r)[1]


def test_the_kernel_entry_point_refuses_before_any_launch():
    lib = nat.lib()
    call = lambda **kw: lib.rajni_rope_qk(*[{**dict(qkv=PTR, src=None, cos=PTR, sin=PTR, hs=0, B=2, N=17, P=1, H=2, D=64, layout=0,
                                                    dtype=nat.RAJNI_BF16, stream=None), **kw}[k]
                                            for k in ("qkv", "src", "cos", "sin", "hs", "B", "N", "P", "H", "D", "layout", "dtype", "stream")])
    err = lambda: lib.rajni_last_error().decode()
    for D in (4, 12, 136, 0):
        assert call(D=D) == UNSUPPORTED and "multiple of 8 up to 128" in err()
    assert call(layout=2) == INVALID and "layout" in err()
    assert call(dtype=5) == INVALID and "bad dtype" in err()
    assert call(P=17) == INVALID and call(P=-1) == INVALID and call(P=33, N=40) == INVALID and call(B=0) == INVALID and call(H=0) == INVALID
    assert call(hs=-64) == INVALID and call(hs=6) == INVALID and "head_stride" in err()
    for name in ("qkv", "cos", "sin"):
        assert call(**{name: None}) == INVALID and "null pointer" in err()
        assert call(**{name: PTR + 8}) == INVALID and f"{name} must be 16-byte aligned" in err()
    assert call(src=PTR + 2) == INVALID and "src must be 4-byte aligned" in err()


# ---- the timm-shaped modules against the rule ------------------------------------------------------------------------------

@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("per_head", [False, True])
def test_attention_with_rope_agrees_with_the_rule(per_head, half):
    torch.manual_seed(0)
    B, N, P, H, D = 2, 11, 3, 2, 24
    att = ts.Attention(H * D, H, qk_norm=True, rotate_half=half, num_prefix_tokens=P).eval()
    x = torch.randn(B, N, H * D)
    rng = np.random.default_rng(1)
    emb = rng.uniform(-1, 1, ((H,) if per_head else ()) + (N - P, 2 * D)).astype(np.float32)      # sin || cos, no identity assumed
    with torch.no_grad():
        got = att(x, rope=torch.from_numpy(emb)).numpy()
        qkv = att.qkv(x).reshape(B, N, 3, H, D)
        q, k, v = att.q_norm(qkv[:, :, 0]), att.k_norm(qkv[:, :, 1]), qkv[:, :, 2]
        flat = torch.stack([q, k, v], 2).numpy()
    sin, cos = emb[..., :D], emb[..., D:]
    want, bud = nrp.rope_qkv(flat, cos, sin, P, nrp.HALF if half else nrp.INTERLEAVED, None, "fp32")
    # the module's own rotation to fp32 rounding, element for element
    with torch.no_grad():
        mine = torch.cat([q[:, :P], ts.apply_rot_embed_cat(q[:, P:].transpose(1, 2), torch.from_numpy(emb), half).transpose(1, 2)], 1).numpy()
    assert np.all(np.abs(mine - want[:, :, 0]) <= bud[:, :, 0] + 1e-30) and np.array_equal(mine[:, :P], flat[:, :P, 0])
    # ... and its output is attention over the rule's q and k
    qr, kr = torch.from_numpy(want[:, :, 0]), torch.from_numpy(want[:, :, 1])
    a = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", qr, kr) * D ** -0.5, -1)
    out = torch.einsum("bhqk,bkhd->bqhd", a, v.double()).reshape(B, N, H * D)
    with torch.no_grad():
        ref = (out @ att.proj.weight.double().T + att.proj.bias.double()).numpy()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    assert att.rotate_half is half and att.num_prefix_tokens == P


def test_rotary_embedding_tables():
    for name, shape in (("vit_micro_rope_patch16_64", (16, 128)), ("vit_micro_rope_half_reg4_patch16_64", (16, 128)),
                        ("vit_micro_rope_mixed_gap_patch16_64", (4, 2, 16, 128)), ("vit_micro_rope_d40_patch14_56", (16, 80))):
        m = nrp.build_model(name, wseed=2)
        e = m.rope.get_embed()
        assert tuple(e.shape) == shape and e.dtype == torch.float32
        assert torch.equal(e, m.rope.get_embed()) and torch.equal(e, nrp.build_model(name, wseed=2).rope.get_embed())      # deterministic
        D = m.cfg.head_dim
        s, c = e[..., :D], e[..., D:]
        assert float((s * s + c * c - 1).abs().max()) < 1e-5                   # sin first, cos second, of one angle
        pair = (lambda t: (t[..., :D // 2], t[..., D // 2:])) if m.cfg.rope_half else (lambda t: (t[..., ::2], t[..., 1::2]))
        assert torch.equal(*pair(s)) and torch.equal(*pair(c))                  # both elements of a pair share the angle
        g = m.rope.get_embed(shape=(3, 6))
        assert tuple(g.shape) == shape[:-2] + (18, shape[-1])
        # row-major like the patch embedding: patch (y, x) of the 3 x 6 grid is patch (y, x) of the 4 x 4 grid
        assert torch.equal(g[..., [0, 1, 6, 7, 13], :], e[..., [0, 1, 4, 5, 9], :])
    # axial: row 0 is the identity, and the first half of the angles follows y, the second x
    e = nrp.build_model("vit_micro_rope_patch16_64").rope.get_embed()
    assert torch.equal(e[0, :64], torch.zeros(64)) and torch.equal(e[0, 64:], torch.ones(64))
    assert torch.equal(e[1, :32], torch.zeros(32)) and torch.equal(e[4, 32:64], torch.zeros(32)) and float(e[4, 0]) == pytest.approx(np.sin(1.0))


# ---- the wrapper's recognition -----------------------------------------------------------------------------------------------

class Tables(nn.Module):
    """a rotary module by contract alone: get_embed returns what it was given"""

    def __init__(self, emb):
        super().__init__()
        self.emb = emb

    def get_embed(self, shape=None):
        return self.emb


def test_table_shapes_and_layout_are_classified():
    H, D, depth, n = 2, 64, 4, 16
    assert classify_rope_embed(torch.zeros(n, 2 * D), H, D, depth) == "shared"
    assert classify_rope_embed(torch.zeros(H, n, 2 * D), H, D, depth) == "per_head"
    assert classify_rope_embed(torch.zeros(depth, H, n, 2 * D), H, D, depth) == "per_block"
    for bad, word in ((torch.zeros(n, D), "2 \\* head_dim = 128"), (torch.zeros(n, 2 * D + 2), "2 \\* head_dim"),
                      (torch.zeros(3, n, 2 * D), "per-head table needs 2 heads"), (torch.zeros(5, H, n, 2 * D), "per-block table needs 4 blocks"),
                      (torch.zeros(2 * D), "get_embed"), (torch.zeros(n, 2 * D, dtype=torch.int32), "get_embed"), ("no", "get_embed")):
        with pytest.raises(NotImplementedError, match=word):
            classify_rope_embed(bad, H, D, depth)
    want = {"vit_micro_rope_patch16_64": ("shared", False), "vit_micro_rope_half_reg4_patch16_64": ("shared", True),
            "vit_micro_rope_mixed_gap_patch16_64": ("per_block", False), "vit_micro_rope_d40_patch14_56": ("shared", True)}
    for name, (kind, half) in want.items():
        w = rajni_amd.RAJNIViTWrapper(nrp.build_model(name), nrp.SCHED)
        d = w.check_supported()
        assert (d["rope"], d["rope_half"]) == (kind, half), name
        assert rope_layout(w.blocks) is half          # read through RAJNIAttention on the scheduled blocks too
    # a model without rotary positions says so and keeps its entry point; a per-head stub is recognised by contract
    m = ts.create_model("vit_micro_patch16_64")
    assert rope_tables(m, 2, 64, 4) is None and rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["rope"] is None
    m.rope = Tables(torch.zeros(2, 16, 128))
    assert rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["rope"] == "per_head"
    # a model without an absolute embedding is described like any other
    m = nrp.build_model("vit_micro_rope_half_reg4_patch16_64")
    assert m.pos_embed is None and "pos_embed" not in m.state_dict()
    assert rajni_amd.RAJNIViTWrapper(m, {}).check_supported()["num_prefix"] == 5


def test_wrapper_refusals_name_the_module():
    m = nrp.build_model("vit_micro_rope_patch16_64")
    m.rope = Tables(torch.zeros(16, 64))                   # half the width: a table for part of the head dim
    with pytest.raises(NotImplementedError, match=r"2 \* head_dim = 128; got \(16, 64\)"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    m = nrp.build_model("vit_micro_rope_patch16_64")
    m.rope = nn.Identity()
    with pytest.raises(NotImplementedError, match="has no get_embed"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    m = nrp.build_model("vit_micro_rope_patch16_64")
    m.blocks[2].attn.rotate_half = True
    with pytest.raises(NotImplementedError, match="block 2: attn.rotate_half differs between blocks"):
        rajni_amd.RAJNIViTWrapper(m, nrp.SCHED).check_supported()
    m = nrp.build_model("vit_micro_rope_half_reg4_patch16_64")
    m.blocks[3].attn.num_prefix_tokens = 1
    with pytest.raises(NotImplementedError, match="block 3: attn.num_prefix_tokens = 1 but the model has 5"):
        rajni_amd.RAJNIViTWrapper(m, {}).check_supported()
    # fp8_mfma: at the setter, and where a table attached after the setter is caught
    w = rajni_amd.RAJNIViTWrapper(nrp.build_model("vit_micro_rope_patch16_64"), nrp.SCHED)
    with pytest.raises(NotImplementedError, match="rotary position embeddings"):
        w.set_weight_format("fp8_mfma")
    assert w.set_weight_format("fp8") is w
    m = ts.create_model("vit_micro512_patch16_64")
    w = rajni_amd.RAJNIViTWrapper(m, {}).set_weight_format("fp8_mfma")
    m.rope = Tables(torch.zeros(16, 128))
    with pytest.raises(NotImplementedError, match='"fp8_mfma" on a model with rotary position embeddings'):
        w.check_supported()


# ---- timm_shaped -----------------------------------------------------------------------------------------------------------

def _digest(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()[:16]


def test_configs_and_synthetic_weights():
    assert len(dataclasses.fields(ts.ViTConfig)) == 20          # (what existing tests count)
    fields = [f.name for f in dataclasses.fields(ts.RopeViTConfig)]
    assert fields[-3:] == ["rope", "rope_half", "abs_pos"] and fields[:23] == [f.name for f in dataclasses.fields(ts.NormViTConfig)]
    c = ts.ViTConfig()
    assert (c.rope, c.rope_half, c.abs_pos) == ("none", False, True)
    with pytest.raises(ValueError, match="rope"):
        ts.RopeViTConfig(rope="learned")
    with pytest.raises(ValueError, match="multiple of 4"):
        ts.RopeViTConfig(embed_dim=132, num_heads=6, rope="axial")
    assert list(ts.ROPE_CONFIGS)[:4] == nrp.MICRO
    others = set(ts.CONFIGS) | set(ts.SWIGLU_CONFIGS) | set(ts.NOCLASS_CONFIGS) | set(ts.MAP_CONFIGS) | set(ts.NORM_CONFIGS)
    assert not set(ts.ROPE_CONFIGS) & others and all(ts.config_of(n) is ts.ROPE_CONFIGS[n] for n in ts.ROPE_CONFIGS)
    want = {"vit_micro_rope_patch16_64": ("axial", False, True, 64, 1, "token"),
            "vit_micro_rope_half_reg4_patch16_64": ("axial", True, False, 64, 5, "token"),
            "vit_micro_rope_mixed_gap_patch16_64": ("mixed", False, True, 64, 0, "avg"),
            "vit_micro_rope_d40_patch14_56": ("axial", True, True, 40, 1, "token")}
    for name, v in want.items():
        c = ts.config_of(name)
        assert (c.rope, c.rope_half, c.abs_pos, c.head_dim, c.num_prefix_tokens, c.global_pool) == v, name
    assert ts.config_of("vit_micro_rope_half_reg4_patch16_64").layer_scale and ts.config_of("vit_micro_rope_d40_patch14_56").patch_size == 14
    # adding the options moves no existing config's weights: a config that says what ViTConfig's defaults say draws the stream it
    # always drew, and three existing streams are held to the digests they had before this file existed
    for name in ("vit_micro_patch16_64", "vit_micro_swiglu_split_patch16_64", "vit_micro_reg4_nocls_gap_patch16_64",
                 "vit_micro_aimv2_patch16_64", "vit_micro_map_patch16_64"):
        base = ts.config_of(name)
        kw = {**base.to_dict(), **{k: getattr(base, k) for k in ("norm", "embed_norm", "bias")}}
        twin = ts.RopeViTConfig(**kw)
        a, b = ts.synth_state_dict(base, seed=3, std=0.08, bias_std=0.02), ts.synth_state_dict(twin, seed=3, std=0.08, bias_std=0.02)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
    digests = {"vit_micro_patch16_64": "0b25e3a4f0eed014", "deit3_micro_reg4_patch16_64": "4f600a2150cd962c",
               "vit_micro_aimv2_patch16_64": "7540c14fe4a2d60f", "vit_micro_map_patch16_64": "f1a645e9f6550c3e"}
    for name, d in digests.items():
        assert _digest(ts.synth_state_dict(ts.config_of(name), seed=3, std=0.08, bias_std=0.02)) == d, name
    # the axial model draws exactly the plain model's stream; the mixed model's frequencies come after every other draw; a
    # model without an absolute embedding draws none
    plain = ts.synth_state_dict(ts.config_of("vit_micro_patch16_64"), seed=3)
    axial = ts.synth_state_dict(ts.config_of("vit_micro_rope_patch16_64"), seed=3)
    assert list(plain) == list(axial) and all(np.array_equal(plain[k], axial[k]) for k in plain)
    mixed = ts.synth_state_dict(ts.config_of("vit_micro_rope_mixed_gap_patch16_64"), seed=3)
    gap = ts.synth_state_dict(ts.config_of("vit_micro_nocls_gap_patch16_64"), seed=3)
    assert list(mixed) == list(gap) + ["rope.freqs"] and all(np.array_equal(mixed[k], gap[k]) for k in gap)
    assert mixed["rope.freqs"].shape == (4, 2, 32, 2)
    assert "pos_embed" not in ts.synth_state_dict(ts.config_of("vit_micro_rope_half_reg4_patch16_64"), seed=3)
    m = ts.create_model("vit_micro_patch16_64")
    assert m.rope is None and m.blocks[0].attn.rotate_half is False


@pytest.mark.parametrize("name", nrp.MICRO)
def test_restatement_is_the_stock_forward_on_the_empty_schedule(name):
    cfg, sd, iseed, tables = nrp.fixture(name)
    imgs = nrp.images_of(cfg, 2, iseed)
    with torch.no_grad():
        stock = nrp.build_model(name)(torch.from_numpy(imgs)).numpy()
    want, counts, tr = nrp.vit_forward_restated(sd, imgs, {}, cfg, tables)
    assert not tr and counts == [cfg.num_patches + cfg.num_prefix_tokens] * cfg.depth
    assert np.abs(want - stock).max() <= 1e-4 * np.abs(want).max()


# ---- the fixtures are evidence ---------------------------------------------------------------------------------------------

CASES = [(name, sched, size) for name in nrp.MICRO for sched, size in [("SCHED", None)] + nrp.EXTRA.get(name, [])]


@pytest.mark.parametrize("name,sched,size", CASES, ids=[f"{n}-{s}-{z or 'own'}" for n, s, z in CASES])
def test_every_mutant_clears_four_bars_on_every_fixture(name, sched, size):
    cfg = nrp.fixture(name)[0]
    sep = nrp.mutant_separations(name, sched, size)
    floor = nrp.MUTANT_FACTOR * max(nrp.BAR.values())
    print(f"[rope] {name} {sched} {size}: " + ", ".join(f"{m} {v:.3g}" for m, v in sep.items()) + f" (floor {floor:.3g})")
    assert set(sep) == set(nrp.MUTANTS) == {"no_rope", "stream_positions", "rotate_prefix", "rotate_v", "other_layout", "sign_flipped"}
    for mut, v in sep.items():
        if nrp.vacuous(cfg, mut):          # no prefix rows: the mutant is the forward itself, to the bit
            assert v == 0.0 and cfg.num_prefix_tokens == 0
        else:
            assert v >= floor, f"{name} {sched} {size}: mutant {mut} moves the logits by {v:.3g} of their scale, under {floor:.3g}"
    # the schedule prunes in block 1, so two blocks rotate a pruned stream
    tr = nrp.case(name, sched, size)[3][2]
    assert min(tr) == 1 and tr[1]["keep_idx"].shape[1] < nrp.case(name, sched, size)[3][1][0]


@pytest.mark.parametrize("name,sched,size", CASES, ids=[f"{n}-{s}-{z or 'own'}" for n, s, z in CASES])
def test_fixture_seeds_leave_no_near_tie(name, sched, size):
    assert nrp.boundary_gap_ratios(name, sched, size) >= nrp.GAP_FACTOR


@pytest.mark.parametrize("name", nrp.MICRO)
def test_committed_seeds_have_the_property(name):
    # (search_seeds walks the seeds from 1 up with this test and stops at the committed one; the walk itself takes minutes and
    # is run here only where it ends at once)
    wseed, iseed = nrp.SEEDS[name]
    assert iseed == wseed + 4 and nrp.holds(name, wseed)
    assert max(nrp.format_cost(name, wseed, B) for B in (1, nrp.BATCH)) <= nrp.FORMAT_HEADROOM * nrp.BAR["bf16"]
    if wseed == 1:
        assert nrp.search_seeds(name) == (1, 5)
