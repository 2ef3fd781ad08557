#!/usr/bin/env python
"""What one forward of an RMSNorm trunk costs on the device (include/rajni_hip_norm.h): the aimv2_large_patch14_224 dimensions
(1024 wide, 24 blocks, 8 heads of 128, split SwiGLU of width 2816, patch 14, no class token, RMSNorm with an embedding norm)
against the same trunk with LayerNorm substituted for every RMSNorm, bf16, keep ratios .7 / .5 / .3 at blocks 6 / 12 / 18.

Modes alternate A B B A inside one process (so a drifting clock falls on both alike); every figure is the MEDIAN over the
rounds of a device-event time around 10 back-to-back forwards after 3 warm-up calls.  Neither measurement has a pass mark.

    python tools/rmsnorm_cost.py [--out FILE (appended to)] [--rounds 6] [--batch 64]
"""
import argparse
import dataclasses
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))

import rajni_amd  # noqa: E402
from rajni_amd import _native as nat  # noqa: E402
from rajni_amd import timm_shaped as ts  # noqa: E402

SCHEDULE = {6: {"keep_ratio": 0.7, "update": True}, 12: {"keep_ratio": 0.5, "update": True}, 18: {"keep_ratio": 0.3, "update": True}}


def timed(call, calls=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls      # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    nat.check(nat.lib().rajni_device_check(), "device check")
    cfg = ts.config_of("aimv2_large_patch14_224")
    x = torch.randn((args.batch, 3, cfg.img_size, cfg.img_size), generator=torch.Generator(device="cuda").manual_seed(0),
                    device="cuda").to(torch.bfloat16)
    models = {}
    for label, c in (("RMSNorm", cfg), ("LayerNorm substituted", dataclasses.replace(cfg, norm="layernorm"))):
        w = rajni_amd.RAJNIViTWrapper(ts.create_model(c, seed=0).to(torch.bfloat16), SCHEDULE).to("cuda").eval()
        models[label] = w
        for _ in range(3):
            w(x)
    torch.cuda.synchronize()
    times = {m: [] for m in models}
    for _ in range(args.rounds):
        for m in list(models) + list(reversed(list(models))):
            times[m].append(timed(lambda: models[m](x)))
    lines = [f"# tools/rmsnorm_cost.py: aimv2_large_patch14_224 dimensions, bf16, batch {args.batch}, keep .7/.5/.3 at blocks 6/12/18; "
             f"medians over {args.rounds} A B B A rounds of 10 forwards, [min, max] beside"]
    for m, v in times.items():
        med = statistics.median(v)
        lines.append(f"forward {m:22s}: {med:7.3f} ms [{min(v):.3f}, {max(v):.3f}]  {args.batch / med * 1000:8.0f} img/s "
                     f"(token counts {models[m].get_last_stats()['token_counts']})")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
