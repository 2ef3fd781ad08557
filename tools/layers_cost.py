"""What intermediate-layer features cost: ViT-B/16 @224, bf16, batch 256, the README schedule, one process, host clock around
sync -> call -> sync (as evaluate_model times a forward), the median over the timed calls of every mode:
  D  forward_features(x, dense=True)                                              the same tree's one-output baseline
  Z  forward_intermediates(x, [2, 5, 8, 11], norm=True, output_fmt="NLC")          four slabs and `final`, ONE forward
  L  the same with fill="last"
  T  four wrappers whose base models are deep copies cut to blocks[:3], [:6], [:9], [:12], scheduled in the blocks they
     still have, forward_features(x, dense=True) on each: what the four tensors took before forward_intermediates existed
Every mode is warmed up first (every shape the timed windows use); the rounds alternate D Z L T T L Z D.  "NLC" keeps the
timed call free of the NCHW permute, which is a torch copy of the four slabs' patch rows.
usage: python tools/layers_cost.py [batch=256] [rounds=6] [calls per mode and round=10]"""
import copy, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rajni-vit_amd"))
import torch, rajni_amd
from rajni_amd import timm_shaped as ts

SCHED = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
         7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}
CAPS = [2, 5, 8, 11]


def main(B, rounds, inner):
    cfg = ts.config_of("vit_base_patch16_224")
    base = ts.create_model(cfg, seed=0)
    wrap = lambda m, s: rajni_amd.RAJNIViTWrapper(m, s).to("cuda").to(torch.bfloat16).eval()
    w = wrap(copy.deepcopy(base), SCHED)
    twins = []
    for c in CAPS:
        m = copy.deepcopy(base)
        m.blocks = m.blocks[:c + 1]
        twins.append(wrap(m, {k: v for k, v in SCHED.items() if k <= c}))
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").to(torch.bfloat16)
    run = {"D": lambda: w.forward_features(x, dense=True),
           "Z": lambda: w.forward_intermediates(x, CAPS, norm=True, output_fmt="NLC"),
           "L": lambda: w.forward_intermediates(x, CAPS, norm=True, output_fmt="NLC", fill="last"),
           "T": lambda: [t.forward_features(x, dense=True) for t in twins]}
    for f in run.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # the four slabs are the four twins' tensors (free-running selections agree: the same kernels on the same rows)
    final, inter = w.forward_intermediates(x, CAPS, norm=True, output_fmt="NLC", return_prefix_tokens=True)
    same = all(torch.equal(torch.cat([p, s], 1).view(torch.int16), t.forward_features(x, dense=True).view(torch.int16))
               for (s, p), t in zip(inter, twins))
    ms = {m: [] for m in run}
    for r in range(rounds):
        for m in ("DZLT" if r % 2 == 0 else "TLZD"):
            for _ in range(inner):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run[m]()
                torch.cuda.synchronize()
                ms[m].append((time.perf_counter() - t0) * 1e3)
    med = lambda v: sorted(v)[len(v) // 2]
    n0 = final.shape[1]
    print(f"vit_base_patch16_224 bf16 batch {B}, README schedule, fp32 stream; token counts {w.get_last_stats()['token_counts']}; "
          f"captures {CAPS}; slab [B, {n0}, {cfg.embed_dim}] = {B * n0 * cfg.embed_dim * 2 / 1e6:.1f} MB; {rounds} rounds x {inner} calls "
          f"per mode, alternating; slabs == the cut twins' tensors bit for bit: {same}")
    for m, what in (("D", "forward_features(dense=True)"), ("Z", "forward_intermediates, four slabs"),
                    ("L", 'forward_intermediates, fill="last"'), ("T", "four cut twins, four forwards")):
        v = ms[m]
        print(f"{m} {what:36s}: {med(v):8.3f} ms per call (min {min(v):.3f}, max {max(v):.3f}, {len(v)} calls)")
    d, z, l, t = (med(ms[m]) for m in "DZLT")
    print(f"Z - D = {(z - d) * 1e3:+8.1f} us = {(z - d) / len(CAPS) * 1e3:.1f} us per slab; Z / D = {z / d:.4f}")
    print(f"L - D = {(l - d) * 1e3:+8.1f} us; L / D = {l / d:.4f}; L - Z = {(l - z) * 1e3:+.1f} us")
    print(f"T / Z = {t / z:.3f}; T / L = {t / l:.3f}")


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(a[0] if a else 256, a[1] if len(a) > 1 else 6, a[2] if len(a) > 2 else 10)
