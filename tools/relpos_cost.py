#!/usr/bin/env python
"""What a relative position bias costs in the attention launch (include/rajni_hip_relpos.h): ViT-B/16 dimensions (H = 12, head
dim 64), bf16, batch 256, at 197 tokens (14 x 14 + class) unpruned and at the README schedule's pruned counts with a position map.

Microseconds per launch (device events around 50 back-to-back launches after 5 warm-up launches, the median of 5 such windows,
[min, max] behind it) of
  rajni_attention          the persistent kernel (what a model without a bias runs), and its one-shot form
                           (rajni_debug_force_attention(2): the form the bias kernel is built on)
  rajni_attention_relpos   the one-shot kernel with the bias: per-token codes in LDS, the table read through the cache
A record, not a pass mark.

    python tools/relpos_cost.py [--out FILE (appended to)] [--batch 256]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))

from rajni_amd import _native as nat  # noqa: E402


def window_us(call, launches=50, warm=5, windows=5):
    for _ in range(warm):
        call()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / launches * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    B, H, D, gh, gw, P = args.batch, 12, 64, 14, 14, 1
    C, n0 = H * D, gh * gw + P
    lib, s = nat.lib(), nat.stream_ptr(torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(0)
    T = (2 * gh - 1) * (2 * gw - 1)
    table = torch.randn((H, T), generator=g, device="cuda")
    pq, pk, pqk = (torch.randn(H, generator=g, device="cuda") for _ in range(3))
    qkv = torch.randn((B, n0, 3 * C), generator=g, device="cuda").to(torch.bfloat16)
    lines = [f"{'tokens':>6s} | {'persistent us':>13s} {'[min, max]':>16s} | {'one-shot us':>11s} {'[min, max]':>16s} | "
             f"{'with bias us':>12s} {'[min, max]':>16s} | bias / persistent  bias / one-shot"]
    for N in (197, 173, 152, 121, 87):
        idx = pos = None
        if N < n0:      # a sub-selection of the grid in ascending order per image, as the forward's selection and map are
            idx = torch.cat([torch.arange(P, device="cuda").expand(B, P),
                             P + torch.rand((B, n0 - P), generator=g, device="cuda").argsort(1)[:, :N - P].sort(1).values], 1)
            idx = pos = idx.to(torch.int32).contiguous()
        out = torch.empty((B, N, C), dtype=torch.bfloat16, device="cuda")
        ip = idx.data_ptr() if idx is not None else None
        plain = lambda: nat.check(lib.rajni_attention(qkv.data_ptr(), ip, out.data_ptr(), B, n0, N, H, D, 0.125, nat.RAJNI_BF16, s),
                                  "rajni_attention")
        bias = lambda: nat.check(lib.rajni_attention_relpos(qkv.data_ptr(), ip, out.data_ptr(), B, n0, N, H, D, 0.125, nat.RAJNI_BF16,
                                                            table.data_ptr(), pq.data_ptr(), pk.data_ptr(), pqk.data_ptr(), gh, gw, P,
                                                            ip, s), "rajni_attention_relpos")
        a = window_us(plain)
        lib.rajni_debug_force_attention(2)
        try:
            o = window_us(plain)
        finally:
            lib.rajni_debug_force_attention(0)
        r = window_us(bias)
        fmt = lambda t: f"{t[0]:9.1f} [{t[1]:6.1f}, {t[2]:6.1f}]"
        lines.append(f"{N:6d} | {fmt(a):>30s} | {fmt(o):>28s} | {fmt(r):>29s} | {r[0] / a[0]:17.2f}  {r[0] / o[0]:15.2f}")
    text = "\n".join([f"# tools/relpos_cost.py: attention launch, H = {H}, D = {D}, bf16, batch {B}, grid {gh} x {gw} + class; "
                      f"{torch.cuda.get_device_name(0)}"] + lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
