#!/usr/bin/env python
"""Time the tiled importance + top-k path (score_tile_kernel + score_finish_kernel) on the device.

  tiled path alone             (64, 1374, 6, 64)  (16, 1025, 16, 64)  (4, 1374, 12, 64)         - shapes one workgroup cannot hold
  tiled (forced) vs one        (256, 197, 12, 64)  (64, 577, 16, 64)                            - shapes both paths take
  workgroup per image

Every figure is a device-event time around CALLS back-to-back enqueues of rajni_score_select_ws on preallocated buffers
(bf16, keep = 70 % of the patch tokens), after WARM warm-up calls, repeated REPS times; compared paths alternate A B A B ...
inside one process.  Bytes/s are the ALGORITHMIC bytes over that time: the K and V thirds of qkv and the CLS query row read once,
the scratch written once and read once (tiled path only), the scores and the selection written once.

    python tools/score_tiled_bench.py [--out profiles/score_tiled_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rajni-vit_amd"))

from rajni_amd import _native as nat  # noqa: E402

TILED_ONLY = [(64, 1374, 6, 64), (16, 1025, 16, 64), (4, 1374, 12, 64)]
BOTH = [(256, 197, 12, 64), (64, 577, 16, 64)]
WARM, CALLS, REPS = 10, 50, 7


class Case:
    def __init__(self, B, N, H, D, tiled):
        self.shape, self.tiled = (B, N, H, D), tiled
        lib = nat.lib()
        lib.rajni_debug_force_score_tiled(int(tiled))
        try:
            self.ws_bytes = lib.rajni_score_select_workspace_bytes(B, N, H, D, nat.RAJNI_BF16)
        finally:
            lib.rajni_debug_force_score_tiled(0)
        assert bool(self.ws_bytes) == bool(tiled), (self.shape, tiled, self.ws_bytes)
        g = torch.Generator(device="cuda").manual_seed(N * H + D)
        self.qkv = torch.randn((B, N, 3 * H * D), generator=g, device="cuda").to(torch.bfloat16)
        self.keep = max(1, int(0.7 * (N - 1)))
        self.scores = torch.empty((B, N), dtype=torch.bfloat16, device="cuda")
        self.idx = torch.empty((B, self.keep + 1), dtype=torch.int32, device="cuda")
        self.nxt = torch.empty((B, self.keep + 1), dtype=torch.bfloat16, device="cuda")
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda") if self.ws_bytes else None
        io = (2 * N * H * D + H * D) * 2 * B + 2 * N * B + (4 + 2) * (self.keep + 1) * B
        self.bytes = io + 2 * self.ws_bytes

    def call(self):
        B, N, H, D = self.shape
        lib = nat.lib()
        lib.rajni_debug_force_score_tiled(int(self.tiled))
        try:
            nat.check(lib.rajni_score_select_ws(self.qkv.data_ptr(), B, N, H, D, 1e-6, 1, self.keep, self.scores.data_ptr(),
                                                self.idx.data_ptr(), self.nxt.data_ptr(), nat.RAJNI_BF16, nat.ptr(self.ws),
                                                self.ws_bytes, nat.stream_ptr()), "rajni_score_select_ws")
        finally:
            lib.rajni_debug_force_score_tiled(0)

    def time_us(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            self.call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / CALLS


def measure(cases):
    for c in cases:
        for _ in range(WARM):
            c.call()
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(REPS):
        for i, c in enumerate(cases):        # alternating: A B A B ...
            times[i].append(c.time_us())
    return times


def line(c, t):
    med, lo, hi = statistics.median(t), min(t), max(t)
    name = "tiled (tile + finish kernel)" if c.tiled else "one workgroup per image     "
    return (f"{str(c.shape):22s} {name}  med {med:8.1f} us  min {lo:8.1f}  max {hi:8.1f}  | algorithmic {c.bytes / 1e6:8.2f} MB "
            f"(scratch {c.ws_bytes / 1e6:7.2f} MB) -> {c.bytes / med / 1e6:7.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_tiled_bench: needs the GPU (no CPU fallback; a CPU timing would say nothing)")
    nat.check(nat.lib().rajni_device_check(), "device check")
    out = [f"# tools/score_tiled_bench.py on {torch.cuda.get_device_name(0)}: bf16, keep 70 %, {REPS} x {CALLS} back-to-back calls per figure "
           f"(device events), {WARM} warm-up calls; us per call (both launches of the tiled path)"]
    out.append("# shapes one workgroup's LDS cannot hold (refused before): the tiled path")
    for shape in TILED_ONLY:
        c = Case(*shape, tiled=True)
        out.append(line(c, measure([c])[0]))
    out.append("# shapes both paths take: the hook forces the tiled kernels; alternating A B A B in one process (dispatch itself never picks tiled here)")
    for shape in BOTH:
        a, b = Case(*shape, tiled=False), Case(*shape, tiled=True)
        ta, tb = measure([a, b])
        assert torch.isfinite(a.scores.float()).all() and torch.isfinite(b.scores.float()).all()
        out += [line(a, ta), line(b, tb)]
    text = "\n".join(out)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
