"""Yardstick for `forward_intermediates` / rajni_vit_forward_layers, torch on the CPU, shared by tests/test_layers_cpu.py and
tests/test_gpu_layers.py.  No graph code of its own: everything is tests/numerics_last.features_last_restated (and through it
tests/numerics_features.features_restated), called once per captured block.

For the capture list c_0 < c_1 < ... slab l is [B, P + n, C], the unpruned sequence:
  a token alive behind block c_l        f(x_after_{c_l}) at its source position;
  a token scheduled block i <= c_l drops  zeros (fill="zero"), or f(x_entry_i), the state it had when it left (fill="last").
f is the model's final LayerNorm (norm=True) or the identity on the stream (norm=False).

Slab l is the `dense` / `dense_last` of the SAME graph cut off behind block c_l: `depth = c_l + 1`, the schedule restricted to
the blocks <= c_l, the full run's selections forced - a block that is both scheduled and captured drops first.  norm=False is
that graph on a state dict without `norm.*`: features_restated applies the final norm only where the weights exist."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

import numerics_features as nf
import numerics_last as nl
from oracle import rajni_oracle as orc


def layers_restated(sd, images, schedule, cfg, blocks, norm, fill, forced_keep=None, dtype=torch.float64):
    """dict(slabs [L, B, P + n, C], exit_block [B, P + n] int32 (`depth` for the survivors), source_idx, counts, trace, final):
    `final` is the full graph's `dense` / `dense_last` WITH the final norm, what forward_intermediates returns beside the list"""
    assert fill in ("zero", "last") and list(blocks) == sorted(set(blocks)) and all(0 <= c < cfg.depth for c in blocks)
    schedule = orc.normalise_schedule(schedule)
    full = nl.features_last_restated(sd, images, schedule, cfg, forced_keep=forced_keep, dtype=dtype)
    sel = {i: t["keep_idx"] for i, t in full["trace"].items()}
    sd_f = sd if norm else {k: v for k, v in sd.items() if not k.startswith("norm.")}
    what = "dense_last" if fill == "last" else "dense"
    slabs = []
    for c in blocks:
        cut = nl.features_last_restated(sd_f, images, {k: v for k, v in schedule.items() if k <= c}, dataclasses.replace(cfg, depth=c + 1),
                                        forced_keep={k: v for k, v in sel.items() if k <= c}, dtype=dtype)
        slabs.append(cut[what])
    return dict(slabs=np.stack(slabs), exit_block=full["exit_block"], source_idx=full["source_idx"], counts=full["counts"],
                trace=full["trace"], final=full[what])


def layernorm64(x, sd, eps):
    """the final LayerNorm of numpy rows in fp64"""
    x = np.asarray(x, np.float64)
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(sd["norm.weight"], np.float64) + np.asarray(sd["norm.bias"], np.float64)
