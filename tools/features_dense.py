"""Per-launch time of the final norm in its three forms, from the rajni_profile_* hooks (HIP events around each launch of the
LayerNorm class), one process: ViT-B/16 @224, bf16, batch 256, the README schedule - 25 LayerNorm launches per forward, of which
only the last differs between the modes when the logits forward runs its last block on all rows (the debug hook), so the
class total's difference between two modes is the difference between their final launches:
  L  logits forward, last block on all rows: the final norm on the B class rows
  T  forward_features(x):                   layernorm_kernel on all B * Nf rows               (RAJNI_POOL_NONE)
  D  forward_features(x, dense=True):       layernorm_dense_kernel on B * (P + n) output rows (RAJNI_POOL_DENSE), and its
                                            source_idx_kernel in the class "other"
Modes alternate L T D D T L ...; the figure per mode is the median over the rounds of the class total per forward.
usage: python tools/features_dense.py [batch=256] [rounds=6] [forwards per round=10]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rajni-vit_amd"))
import torch, rajni_amd
from rajni_amd import _native as nat, timm_shaped as ts

SCHED = {3: {"keep_ratio": 0.88, "update": True}, 4: {"keep_ratio": 0.88, "update": True},
         7: {"keep_ratio": 0.80, "update": True}, 8: {"keep_ratio": 0.72, "update": True}}
KC_LAYERNORM, KC_OTHER = 5, 11


def main(B, rounds, inner):
    cfg = ts.config_of("vit_base_patch16_224")
    w = rajni_amd.RAJNIViTWrapper(ts.create_model(cfg, seed=0), SCHED).to("cuda").to(torch.bfloat16).eval()
    x = torch.randn(B, 3, 224, 224, generator=torch.Generator(device="cuda").manual_seed(1), device="cuda").to(torch.bfloat16)
    run = {"L": lambda: w(x), "T": lambda: w.forward_features(x), "D": lambda: w.forward_features(x, dense=True)}
    nat.lib().rajni_debug_set_last_block_all_rows(1)
    try:
        for f in run.values():          # every shape the timed windows use
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        tokens = w.forward_features(x)
        dense = w.forward_features(x, dense=True)
        src = w.get_last_stats()["source_idx"].long()
        same = torch.equal(torch.gather(dense, 1, src[:, :, None].expand(-1, -1, cfg.embed_dim)).view(torch.int16), tokens.view(torch.int16))
        nf, n0 = tokens.shape[1], dense.shape[1]
        res = {m: {"ln": [], "other": [], "n": 0} for m in run}
        for r in range(rounds):
            for m in ("LTD" if r % 2 == 0 else "DTL"):
                nat.profile_reset()
                nat.profile_enable((1 << KC_LAYERNORM) | (1 << KC_OTHER))
                for _ in range(inner):
                    run[m]()
                torch.cuda.synchronize()
                nat.profile_enable(0)
                p = nat.profile_collect()
                ln = p.get("layernorm_kernel", {"ms": 0.0, "launches": 0})
                res[m]["ln"].append(ln["ms"] / inner * 1e3)
                res[m]["n"] = ln["launches"] // inner
                res[m]["other"].append(sum(v["ms"] for k, v in p.items() if v["kclass"] == KC_OTHER) / inner * 1e3)
        nat.profile_reset()
    finally:
        nat.lib().rajni_debug_set_last_block_all_rows(0)
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"vit_base_patch16_224 bf16 batch {B}, README schedule, fp32 stream; token counts {w.get_last_stats()['token_counts']}; "
          f"Nf {nf}, P + n {n0}; {rounds} rounds x {inner} forwards per mode, alternating; dense rows at source_idx == tokens bit for bit: {same}")
    for m, what in (("L", "logits, last block on all rows"), ("T", "forward_features"), ("D", "forward_features(dense=True)")):
        v = res[m]
        print(f"{m} {what:32s}: LayerNorm class {med(v['ln']):8.1f} us per forward over {v['n']} launches "
              f"(min {min(v['ln']):.1f}, max {max(v['ln']):.1f}); class other {med(v['other']):6.1f} us")
    l, t, d = (med(res[m]["ln"]) for m in "LTD")
    gb = lambda rows_in, rows_out: (rows_in * 768 * 4 + rows_out * 768 * 2) / 1e3     # KB moved: fp32 rows in, bf16 rows out
    print(f"final norm, all {B * nf} rows (layernorm_kernel):          T - L = {t - l:7.1f} us more than the {B}-row launch; "
          f"{gb(B * nf, B * nf) / max(t - l, 1e-9) / 1e3:.2f} TB/s if the small launch were free")
    print(f"final norm, dense, {B * n0} output rows (layernorm_dense_kernel): D - L = {d - l:7.1f} us more than the {B}-row launch; "
          f"{gb(B * nf, B * n0) / max(d - l, 1e-9) / 1e3:.2f} TB/s likewise; D - T = {d - t:+.1f} us; "
          f"source_idx_kernel {med(res['D']['other']):.1f} us")


if __name__ == "__main__":
    a = [int(v) for v in sys.argv[1:]]
    main(a[0] if a else 256, a[1] if len(a) > 1 else 6, a[2] if len(a) > 2 else 10)
