"""Yardstick for `forward_features(x, dense=True, fill="last")` (RAJNI_POOL_DENSE_LAST), torch on the CPU, shared by
tests/test_features_last_cpu.py and tests/test_gpu_features_last.py.  No graph code of its own: everything is
tests/numerics_features.features_restated, called once per scheduled block.

  dense_last  [B, P + n, C]: a token that survives the last block has norm(x_final) at its source position, the row `dense`
              holds there; a token that scheduled block i drops (it entered the block and is not in the block's keep_idx) has
              norm(x_entry_i), x_entry_i the residual stream at the entry of block i (behind norm_pre; the embedded stream for
              i = 0) and norm the model's final LayerNorm.  No row is zero.
  exit_block  [B, P + n] int32: the scheduled block that dropped the token of each position, `depth` for the survivors.

norm(x_entry_i) at original positions is the `dense` of the SAME graph cut off in front of block i: `depth=i`, the schedule
restricted to the blocks < i, the same selections forced.  (`depth=0` runs no block: the embedded stream through the norm.)"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

import numerics_features as nf
from oracle import rajni_oracle as orc


def dropped_positions(selections, B, n0):
    """{block: keep_idx [B, P + keep]} -> ({block: [per image: the ascending source positions the block drops]}, exit_block
    [B, n0] int32 with `-1` at the positions no block drops)"""
    pos = np.broadcast_to(np.arange(n0, dtype=np.int64), (B, n0)).copy()
    exit_block = np.full((B, n0), -1, dtype=np.int32)
    dropped = {}
    for i in sorted(selections):
        idx = np.asarray(selections[i], np.int64)
        kept = np.take_along_axis(pos, idx, axis=1)
        dropped[i] = [np.setdiff1d(pos[b], kept[b]) for b in range(B)]
        for b in range(B):
            assert len(dropped[i][b]) == pos.shape[1] - idx.shape[1], "a selection names a token twice"
            exit_block[b, dropped[i][b]] = i
        pos = kept
    return dropped, exit_block


def features_last_restated(sd, images, schedule, cfg, forced_keep=None, dtype=torch.float64):
    """features_restated's dict plus `dense_last` [B, P + n, C], `exit_block` [B, P + n] int32 and `entry` {block: norm(x_entry)
    at original positions, [B, P + n, C]} for every scheduled block"""
    schedule = orc.normalise_schedule(schedule)
    full = nf.features_restated(sd, images, schedule, cfg, forced_keep=forced_keep, dtype=dtype)
    sel = {i: t["keep_idx"] for i, t in full["trace"].items()}
    B, n0, _ = full["dense"].shape
    dropped, exit_block = dropped_positions(sel, B, n0)
    exit_block[exit_block < 0] = cfg.depth
    out, entry = full["dense"].copy(), {}
    for i in sorted(sel):
        head = nf.features_restated(sd, images, {k: v for k, v in schedule.items() if k < i}, dataclasses.replace(cfg, depth=i),
                                    forced_keep={k: v for k, v in sel.items() if k < i}, dtype=dtype)
        entry[i] = head["dense"]
        for b in range(B):
            out[b, dropped[i][b]] = entry[i][b, dropped[i][b]]
    for b in range(B):       # the survivors and the dropped rows partition the sequence
        assert np.array_equal(np.sort(np.concatenate([full["source_idx"][b]] + [dropped[i][b] for i in dropped])), np.arange(n0))
    return dict(full, dense_last=out, exit_block=exit_block, entry=entry)
