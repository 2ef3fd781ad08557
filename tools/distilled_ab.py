"""The two-row last block of a distilled model against the all-rows form, one process: ms per forward of
deit_base_distilled_patch16_224 (bf16, README schedule) with the default forward (last block on rows 0 and 1 of each image) and under
rajni_debug_set_last_block_all_rows(1), alternated A B B A ..., and the logits of the two compared byte for byte.
usage: python tools/distilled_ab.py [batch=256] [model]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rajni-vit_amd"))
import torch, rajni_amd
from rajni_amd import _native as nat, timm_shaped as ts
sched = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True}, 7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
name = sys.argv[2] if len(sys.argv) > 2 else "deit_base_distilled_patch16_224"
cfg = ts.CONFIGS[name]
m = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=0).to(torch.bfloat16).cuda(), sched).eval()
x = torch.randn(B, 3, cfg.img_size, cfg.img_size, device="cuda").to(torch.bfloat16)
lib = nat.lib()


def run(all_rows, reps=8, inner=10):
    lib.rajni_debug_set_last_block_all_rows(all_rows)
    for _ in range(5): m(x)
    out = m(x).clone()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(inner): m(x)
        torch.cuda.synchronize(); t.append((time.perf_counter() - t0) / inner * 1e3)
    lib.rajni_debug_set_last_block_all_rows(0)
    return out, min(t), sorted(t)[len(t) // 2]


print(f"{name} bf16 B={B} README schedule, token counts {m(x) is not None and m.get_last_stats()['token_counts']}")
res = {0: [], 1: []}
outs = {}
for tag, mode in (("A1", 0), ("B1", 1), ("B2", 1), ("A2", 0), ("A3", 0), ("B3", 1), ("B4", 1), ("A4", 0)):
    out, best, med = run(mode)
    outs.setdefault(mode, out)
    assert torch.equal(out.view(torch.uint8), outs[mode].view(torch.uint8))
    res[mode].append(med)
    print(f"{tag}  {'all rows ' if mode else 'two rows '}  min {best:.3f} ms  median {med:.3f} ms")
same = torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8))
mean = lambda v: sum(v) / len(v)
a, b = mean(res[0]), mean(res[1])
print(f"medians: two rows {a:.3f} ms (spread {max(res[0]) - min(res[0]):.3f}), all rows {b:.3f} ms (spread {max(res[1]) - min(res[1]):.3f}): "
      f"two rows {100 * (a - b) / b:+.2f} %;  logits byte-equal: {same}")
