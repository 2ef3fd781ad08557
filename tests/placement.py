"""The placement contract of include/rajni_hip.h ("placement"), restated for the tests, and the helper that puts every
operand of a kernel launch at a chosen legal placement.  A plain module: tests/test_placement_cpu.py holds the table to the
header's (and every entry point to the table, with fake addresses); tests/test_gpu_placement.py launches every kernel twice,
once with every buffer dense on a 256-byte boundary and once with every pointer at a 256-byte boundary PLUS its minimum
and every row stride at the least legal non-dense value, and asks for the same bits.

No kernel or tiling choice looks at an address or at a stride's residue (csrc: `uintptr_t` appears in refusals only, and the
planner sees shapes), so equality needs no tolerance and fails on one wrong element.
"""
from __future__ import annotations

import os
import re
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from guarded import ALIGN, Guarded

ELEM = "elem"       # one element of the call's dtype: 2 bytes for bf16 / fp16, 4 for fp32 (score arrays)
Align = Union[int, str]

_SCORES = {"scores": ELEM, "keep_idx": 4, "next_scores": ELEM}
_SCORE_SELECT = {"qkv": 16, "scores_out": ELEM, "keep_idx": 4, "next_scores": ELEM}
_POOL = {"x": 16, "norm_w": 16, "norm_b": 16, "fc_w": 16, "fc_b": 16, "out": 16}
_VEC16 = lambda *names: {n: 16 for n in names}

# entry point (or plan struct) -> pointer -> minimum alignment in bytes, in the header's order
CONTRACT: Dict[str, Dict[str, Align]] = {
    "rajni_importance": {"qkv": 16, "scores_out": ELEM},
    "rajni_select_topk": dict(_SCORES),
    "rajni_score_select": dict(_SCORE_SELECT),
    "rajni_select_topk_prefix": dict(_SCORES),
    "rajni_score_select_prefix": dict(_SCORE_SELECT),
    "rajni_score_select_ws": dict(_SCORE_SELECT, workspace=256),
    "rajni_gather_rows": {"src": 16, "idx": 4, "dst": 16},
    "rajni_attention": {"qkv": 16, "keep_idx": 4, "out": 16},
    "rajni_attention_fp8": {"qkv": 16, "keep_idx": 4, "out_q": 16, "row_scale": 4},
    "rajni_layernorm": _VEC16("x", "w", "b", "y"),
    "rajni_layernorm_fp8": dict(_VEC16("x", "w", "b", "y_q"), y_scale=4, hid_scale=4),
    "rajni_linear": dict(_VEC16("x", "w", "y", "resid", "bias", "gamma", "w_scale"), x_scale=4, y_scale=4, r_idx=4),
    "rajni_patch_embed": _VEC16("images", "w", "bias", "cls", "pos", "x", "workspace"),
    "rajni_patch_embed_prefix": _VEC16("images", "w", "bias", "cls", "reg", "pos", "x", "workspace"),
    "rajni_qk_norm": _VEC16("qkv", "q_w", "q_b", "k_w", "k_b"),
    "rajni_layernorm_stream": _VEC16("x", "w", "b"),
    "rajni_pool_norm": dict(_POOL),
    "rajni_pool_norm_prefix": dict(_POOL),
    "rajni_vit_forward": _VEC16("images", "logits"),
    "rajni_vit_plan": dict(_VEC16("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b", "head_w", "head_b"),
                           workspace=256),
    "rajni_block": dict(_VEC16("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "norm2_w", "norm2_b",
                               "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2"),
                        keep_idx=4, scores=ELEM, next_scores=ELEM, forced_keep_idx=4, qkv_s=16, proj_s=16, fc1_s=16, fc2_s=16),
    "rajni_qk_affine": _VEC16("q_norm_w", "q_norm_b", "k_norm_w", "k_norm_b"),
    "rajni_vit_ext": _VEC16("norm_pre_w", "norm_pre_b", "fc_norm_w", "fc_norm_b"),
    "rajni_vit_prefix": {"reg_token": 16},
}

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rajni_hip.h")


def parse_header(path: str = HEADER) -> Dict[str, Dict[str, Align]]:
    """the table of the header's placement paragraph: `rajni_x: name bytes, name bytes, ...` lines up to its end mark"""
    text = open(path).read()
    start = text.index("---- placement: minimum alignment of every pointer ----")
    body = text[start:text.index("(end of the placement table)", start)]
    table: Dict[str, Dict[str, Align]] = {}
    for m in re.finditer(r"^ \*   (rajni_\w+): (.+)$", body, re.M):
        entry: Dict[str, Align] = {}
        for item in m.group(2).split(","):
            name, value = item.split()
            entry[name] = ELEM if value == ELEM else int(value)
        assert m.group(1) not in table, m.group(1)
        table[m.group(1)] = entry
    return table


def min_align(entry: str, name: str, elem_bytes: int = 2) -> int:
    a = CONTRACT[entry][name]
    return elem_bytes if a == ELEM else int(a)


def bits(t: torch.Tensor) -> torch.Tensor:
    """the raw bits of a tensor's elements, dense (torch.equal on floats would call NaN != NaN and -0 == +0)"""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Launch:
    """The buffers of ONE launch of a case.  `shifted=False`: every buffer dense on a 256-byte boundary.  `shifted=True`: every
    pointer at a 256-byte boundary plus the minimum CONTRACT gives it, every row stride `cols + ld_extra` where the caller
    names one.  All buffers are Guarded (poisoned guards, gaps and tails); `check()` holds every one of them to its guards and
    gaps, and every output to "each element written"."""

    def __init__(self, entry: str, shifted: bool, device="cuda", elem_bytes: int = 2):
        self.entry, self.shifted, self.device, self.elem_bytes = entry, shifted, device, elem_bytes
        self.bufs: List[Tuple[str, Guarded, bool]] = []

    def _make(self, name, shape, dtype, ld_extra, out, entry=None, key=None, stride=None, **kw) -> Guarded:
        """`name` labels the buffer; CONTRACT[entry or the launch's][key or name] is its minimum.  `stride`: a row stride both
        launches use (a CLS-row stride, logits_ld); `ld_extra`: elements added to the dense stride in the shifted launch"""
        a = min_align(entry or self.entry, key or name, self.elem_bytes)
        cols = shape[-1] if len(shape) else 1
        if stride is None:
            stride = cols + ld_extra if (self.shifted and ld_extra) else None
        if self.shifted and a < ALIGN:
            g = Guarded(shape, dtype, self.device, row_stride=stride, align=a, misalign=a, **kw)
            assert g.ptr() % ALIGN == a, (name, g.ptr() % ALIGN)
        else:
            g = Guarded(shape, dtype, self.device, row_stride=stride, **kw)
        self.bufs.append((name, g, out))
        return g

    def inp(self, name: str, value: Optional[torch.Tensor], ld_extra: int = 0, **kw) -> Optional[Guarded]:
        """`value` in a guarded view at this launch's placement (None stays None: an optional pointer)"""
        if value is None:
            return None
        return self._make(name, tuple(value.shape), value.dtype, ld_extra, False, **kw).fill_(value)

    def idx(self, name: str, value: torch.Tensor, fill: int, **kw) -> Guarded:
        """int32 index array whose arena (tail included) holds `fill`: a valid index, so an over-read stays in bounds"""
        return self._make(name, tuple(value.shape), torch.int32, 0, False, fill_int32=fill, **kw).fill_(value.to(torch.int32))

    def out(self, name: str, shape: Sequence[int], dtype: torch.dtype, ld_extra: int = 0, **kw) -> Guarded:
        return self._make(name, tuple(shape), dtype, ld_extra, True, **kw)

    def mark_output(self, g: Guarded) -> None:
        """an input the launch also writes (in place): held to "each element written" too"""
        self.bufs = [(n, b, True if b is g else o) for n, b, o in self.bufs]

    def check(self, what: str) -> None:
        for name, g, out in self.bufs:
            g.check(f"{what} [{'shifted' if self.shifted else 'aligned'}]: {name}", written=out)


def ptr(g: Optional[Guarded]) -> Optional[int]:
    return None if g is None else g.ptr()


def assert_same_bits(aligned: Guarded, shifted: Guarded, what: str) -> None:
    a, b = bits(aligned.t), bits(shifted.t)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} elements differ between the aligned and the shifted "
                             f"launch, first at {tuple(int(i) for i in bad[0])}")
