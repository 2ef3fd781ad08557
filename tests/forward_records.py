"""The optional records of the whole forward (rajni_vit_ext, _prefix, _layers, _image, _query, _attn_pool), as a deterministic
generator of cases.  A plain module, not a test: tests/test_forward_records_cpu.py states three properties over its cases, and
tools/forward_records_ab.py prints one line per case for a line-by-line comparison of two builds of the library.

Every plan here is test_forward_refusals_cpu.py's: a 64-pixel image, patch 16, C 128 = 2 x 64, depth 4, hidden 512, 16 classes,
fake 16-byte-aligned addresses nobody follows, and workspace = NULL - so whichever way a check goes nothing is launched, and a
call that passes every other refusal ends at "workspace too small (0 < N)".  No GPU.

An axis is a list of `Value`s; `valid` says whether the value is legal on its own terms (beside some choice of the others),
and an invalid value carries `needles`: a refusal of it beside otherwise-default records names one of them.  `legal` says
whether a combination of valid values is one the forward takes."""
from __future__ import annotations

import ctypes as C
import itertools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

from rajni_amd import _native as nat

FAKE = 0x10000          # 16-byte aligned, never dereferenced
IMAGES, LOGITS = FAKE + 0x100, FAKE + 0x200
DEPTH = 4


class Value(NamedTuple):
    label: str
    valid: bool
    obj: object               # the ctypes record (None: the NULL record)
    ref: object               # C.byref(obj), made once, or None
    needles: Tuple[str, ...]  # an invalid value: what its refusal names (its entry point, or its field)
    alive: object             # whatever `obj` points to on the host


def _value(label, valid, obj, needles=(), alive=None) -> Value:
    return Value(label, valid, obj, None if obj is None else C.byref(obj), tuple(needles), alive)


# ---- the plan -------------------------------------------------------------------------------------------------------------
def _plan(keeps=(0, 0, 0, 0), buffers=(), **fields):
    blocks = (nat.Block * DEPTH)()
    for i, k in enumerate(keeps):
        for name, _ in nat.Block._fields_[:14]:          # the weights
            setattr(blocks[i], name, FAKE)
        blocks[i].keep = k
        if i in buffers:
            blocks[i].keep_idx = blocks[i].next_scores = FAKE
    p = nat.VitPlan()
    p.dtype, p.B, p.in_chans, p.img_size, p.patch_size = nat.RAJNI_BF16, 4, 3, 64, 16
    p.C, p.H, p.D, p.depth, p.hidden, p.num_classes = 128, 2, 64, DEPTH, 512, 16
    p.ln_eps, p.attn_scale, p.pos_has_cls = 1e-6, 0.125, 1
    for name in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"):
        setattr(p, name, FAKE)
    p.blocks = blocks
    p.workspace, p.workspace_bytes = None, 0
    for name, v in fields.items():
        setattr(p, name, v)
    return p, blocks


def _plans() -> List[Value]:
    who = "rajni_vit_forward"
    out = []

    def add(label, valid, made, needles=()):
        out.append(_value(label, valid, made[0], needles, made[1]))
    add("plain", True, _plan())
    add("headless", True, _plan(head_w=None, head_b=None, num_classes=0))
    add("cls_only_last_block", True, _plan(cls_only_last_block=1))
    add("act_fp8", False, _plan(act_fp8=1), (who, "act_fp8"))          # C = 128: act_fp8 needs C >= 512
    add("fp16", True, _plan(dtype=nat.RAJNI_F16))
    add("fp32", True, _plan(dtype=nat.RAJNI_F32))
    add("logits_ld12", False, _plan(logits_ld=12), (who, "logits row stride"))
    add("keeps_0_8_6_0", True, _plan(keeps=(0, 8, 6, 0), buffers=(1, 2)))
    add("keeps_0_17_0_0", False, _plan(keeps=(0, 17, 0, 0), buffers=(1,)), (who, "keep=17"))
    missing = _plan(keeps=(0, 8, 0, 0), buffers=(1,))
    missing[1][1].next_scores = None
    add("no_next_scores", False, missing, (who, "next_scores"))
    add("no_cls_token", False, _plan(cls_token=None), (who, "null weight pointer"))      # (legal without a class row only)
    return out


# ---- the records ----------------------------------------------------------------------------------------------------------
def _exts() -> List[Value]:
    who = "rajni_vit_forward_ext"

    def ext(**fields):
        e = nat.VitExt()
        for name, v in fields.items():
            setattr(e, name, v)
        return e
    out = [_value("NULL", True, None), _value("zero", True, ext())]
    for pool in range(8):
        out.append(_value(f"pool{pool}", pool not in (4, 7), ext(pool=pool), (who, "pool")))
    out.append(_value("norm_absent", True, ext(norm_absent=1)))
    out.append(_value("fc_norm", True, ext(fc_norm_w=FAKE, fc_norm_b=FAKE, fc_norm_eps=1e-6)))
    for act in range(4):
        out.append(_value(f"mlp_act{act}", act != 2, ext(mlp_act=act), (who, "mlp_act")))
    qk = (nat.QkAffine * DEPTH)()
    for i in range(DEPTH):
        for name, _ in nat.QkAffine._fields_:
            setattr(qk[i], name, FAKE)
    qk[2].k_norm_w = None
    out.append(_value("qk_norm_one_missing", False, ext(qk_norm=qk, qk_eps=1e-6), (who, "q/k-norm"), qk))
    return out


def _prefixes() -> List[Value]:
    who = "rajni_vit_forward_ext_prefix"
    return [
        _value("NULL", True, None),
        _value("P0", True, nat.VitPrefix(0)),
        _value("P1", True, nat.VitPrefix(1)),
        _value("P5_reg", True, nat.VitPrefix(5, FAKE)),
        _value("P2_reg_hr2", True, nat.VitPrefix(2, FAKE, 2)),
        _value("P33_reg", False, nat.VitPrefix(33, FAKE), (who, "num_prefix")),
        _value("P3_noreg", False, nat.VitPrefix(3), (who, "reg_token")),
        _value("P1_reg", False, nat.VitPrefix(1, FAKE), (who, "reg_token")),
        _value("hr3", False, nat.VitPrefix(0, None, 3), (who, "head_rows")),
    ]


def _layers() -> List[Value]:
    who = "rajni_vit_forward_layers"

    def lay(blocks, norm=0, fill=0, out=FAKE, slab_stride=0, n=None):
        arr = (C.c_int * max(len(blocks), 1))(*blocks)
        y = nat.VitLayers()
        y.n, y.blocks, y.norm, y.fill, y.out, y.slab_stride = (len(blocks) if n is None else n), arr, norm, fill, out, slab_stride
        return y, arr
    out = [_value("NULL", True, None)]
    for norm, fill in itertools.product((0, 1), repeat=2):
        y, arr = lay([1, 3], norm, fill)
        out.append(_value(f"b13_norm{norm}_fill{fill}", True, y, (), arr))
    for label, valid, (y, arr) in [
        ("n0", False, lay([1, 3], n=0)),
        ("descending", False, lay([3, 1])),
        ("norm2", False, lay([1, 3], norm=2)),
        ("last_block", True, lay([3])),
        ("out_null", False, lay([1, 3], out=None)),
        ("short_slab_stride", False, lay([1, 3], slab_stride=8)),
    ]:
        out.append(_value(label, valid, y, (who, "layers."), arr))
    return out


def _images() -> List[Value]:
    who = "rajni_vit_forward_image"
    out = [_value("NULL", True, None)]
    for h, w, valid in ((64, 64, True), (64, 96, True), (64, 70, False), (48, 64, False)):     # (plan.img_size is 64)
        out.append(_value(f"{h}x{w}", valid, nat.VitImage(h, w), (who, "image.")))
    return out


def _queries() -> List[Value]:
    who = "rajni_vit_forward_query"
    out = [_value("NULL", True, None)]
    for ct, q, valid in ((1, 0, True), (1, 1, True), (0, 1, True), (0, 0, False), (2, 0, False), (1, 2, False)):
        out.append(_value(f"q{ct}{q}", valid, nat.VitQuery(ct, q), (who, "query.")))
    return out


def _pools() -> List[Value]:
    who = "rajni_vit_forward_pool"

    def pool(**fields):
        a = nat.VitAttnPool()
        for name in ("q", "kv_w", "kv_b", "proj_w", "proj_b", "norm_w", "norm_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b"):
            setattr(a, name, FAKE)
        a.norm_eps, a.hidden, a.heads, a.act = 1e-6, 512, 2, nat.MLP_GELU
        for name, v in fields.items():
            setattr(a, name, v)
        return a
    return [
        _value("NULL", True, None),
        _value("good", True, pool()),
        _value("hidden100", False, pool(hidden=100), (who, "pool.hidden")),
        _value("heads3", False, pool(heads=3), (who, "pool.heads")),
        _value("q_null", False, pool(q=None), (who, "pool.q")),
        _value("act2", False, pool(act=2), (who, "pool.act")),
    ]


RECORDS = ("ext", "prefix", "layers", "image", "query", "pool")     # in the order the entry points take them
# level k takes the plan and the first k records
ENTRY_POINTS = ("rajni_vit_forward", "rajni_vit_forward_ext", "rajni_vit_forward_ext_prefix", "rajni_vit_forward_layers",
                "rajni_vit_forward_image", "rajni_vit_forward_query", "rajni_vit_forward_pool")
# the size functions take the plan and (prefix, image, query, pool), the first k of them
SIZE_RECORDS = ("prefix", "image", "query", "pool")
SIZE_FUNCTIONS = ("rajni_vit_workspace_bytes", "rajni_vit_workspace_bytes_prefix", "rajni_vit_workspace_bytes_image",
                  "rajni_vit_workspace_bytes_query", "rajni_vit_workspace_bytes_pool")

_AXES: Optional[Dict[str, List[Value]]] = None


def axes() -> Dict[str, List[Value]]:
    """axis name -> its values, built once (the records are never written to, so every case shares them)"""
    global _AXES
    if _AXES is None:
        _AXES = dict(plan=_plans(), ext=_exts(), prefix=_prefixes(), layers=_layers(), image=_images(), query=_queries(),
                     pool=_pools())
    return _AXES


def cases(level: int, only_valid: bool = False):
    """the full crossing of the plan flavours and the records entry point `level` takes: tuples (plan, record, ...)"""
    ax = axes()
    lists = [ax["plan"]] + [ax[name] for name in RECORDS[:level]]
    if only_valid:
        lists = [[v for v in vals if v.valid] for vals in lists]
    return itertools.product(*lists)


def size_cases(level: int):
    ax = axes()
    return itertools.product(ax["plan"], *[ax[name] for name in SIZE_RECORDS[:level]])


def forward(lib, level: int, case: Sequence[Value], extra_null: int = 0):
    """entry point `level + extra_null` on the case's records, NULL for the records beyond them: (rc, last_error)"""
    fn = getattr(lib, ENTRY_POINTS[level + extra_null])
    rc = fn(*[v.ref for v in case], *([None] * extra_null), IMAGES, LOGITS, None)
    return rc, lib.rajni_last_error()


def size(lib, level: int, case: Sequence[Value], extra_null: int = 0) -> int:
    """size function `level + extra_null` on (plan, prefix, image, query, pool)[: level + 1]"""
    return getattr(lib, SIZE_FUNCTIONS[level + extra_null])(*[v.ref for v in case], *([None] * extra_null))


def legal(plan: Value, ext: Value, prefix: Value, layers: Value, image: Value, query: Value, pool: Value) -> bool:
    """whether a combination of VALID values is one the forward takes (include/rajni_hip*.h).  Written from the headers' rules,
    one per line; the test that uses it asks the library to agree on every combination."""
    e, p = ext.obj, plan.obj
    ext_pool = e.pool if e is not None else nat.POOL_TOKEN
    tokens_out = ext_pool in (nat.POOL_NONE, nat.POOL_DENSE, nat.POOL_DENSE_LAST)
    plain_token_head = e is None or (ext_pool == nat.POOL_TOKEN and not e.fc_norm_w and not e.norm_absent)
    headless = p.num_classes == 0
    cls_only = bool(p.cls_only_last_block)
    nocls = query.obj is not None and query.obj.class_token == 0
    hr2 = prefix.obj is not None and prefix.obj.head_rows == 2
    last_captured = layers.obj is not None and layers.obj.blocks[layers.obj.n - 1] == DEPTH - 1
    if tokens_out and (not headless or cls_only):                 # the token outputs: a headless plan, every row formed
        return False
    if ext_pool == nat.POOL_AVG and cls_only:                       # 'avg' reads every row
        return False
    if (ext_pool == nat.POOL_MAP) != (pool.obj is not None):        # the attention pool: the value and the record, together
        return False
    if pool.obj is not None and (cls_only or hr2):
        return False
    if hr2 and (nocls or headless or cls_only or not plain_token_head):   # the distilled head: two rows into a linear layer
        return False
    if nocls:                                                       # no class row: nothing reads a single row
        if ext_pool == nat.POOL_TOKEN or cls_only:
            return False
        if prefix.obj is not None and (prefix.obj.num_prefix > 0) != bool(prefix.obj.reg_token):
            return False                                            # the record counts the registers alone
    if layers.obj is not None:
        if layers.obj.norm == 1 and e is not None and e.norm_absent:
            return False
        if cls_only and last_captured:
            return False
    return True
