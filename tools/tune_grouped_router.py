"""Development tool: the group-limited router (hpc.grouped_topk_router) at the DeepSeek-V3 shape - 256 experts, 8 groups
keep 4, top 8, sigmoid + correction bias, scale 2.5 - timed in one run, alternating, against
  (b) hpc.topk_router at the same m (the yardstick: the same bytes and the same top-k rounds), timed twice for the spread,
  (c) the eager torch composition a user has without the op (sigmoid, add, view, topk, sum, topk, scatter, masked_fill,
      topk, gather, div, mul).
Every call is timed the way bench.py times its router row: a hipGraph of 20 back-to-back calls, median of 30 replays.
usage: python tools/tune_grouped_router.py [--out FILE]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT))
import torch, bench, hpc  # noqa: E402,E401

E, G, KG, K, SCALE = 256, 8, 4, 8, 2.5


def eager(lg, bias):
    s = torch.sigmoid(lg)
    c = s + bias
    m = c.shape[0]
    gscore = c.view(m, G, E // G).topk(2, dim=-1).values.sum(-1)
    gidx = gscore.topk(KG, dim=-1, sorted=False).indices
    keep = torch.zeros_like(gscore).scatter_(1, gidx, 1.0)
    mask = keep[:, :, None].expand(m, G, E // G).reshape(m, E)
    ids = c.masked_fill(mask == 0, float("-inf")).topk(K, dim=-1).indices
    w = s.gather(1, ids)
    return ids.int(), w / (w.sum(-1, keepdim=True) + 1e-20) * SCALE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = ["# hpc.grouped_topk_router, %d experts, %d groups keep %d, top %d, sigmoid + bias, scale %.1f; us per call, hipGraph of 20 "
             "calls, median of 30 replays" % (E, G, KG, K, SCALE),
             "# m  (a) grouped_topk_router  (b) topk_router  (b) again  (c) eager torch  (a)/(b)  eager ids == (a) ids"]
    for m in (1, 64, 256, 4096):
        lg = torch.randn(m, E, device=dev)
        bias = 0.1 * torch.randn(E, device=dev)
        fa = lambda: hpc.grouped_topk_router(lg, K, G, KG, bias, "sigmoid", True, SCALE)  # noqa: E731
        fb = lambda: hpc.topk_router(lg, K, True)  # noqa: E731
        fc = lambda: eager(lg, bias)  # noqa: E731
        t = {}
        for name, fn in (("a", fa), ("b", fb), ("c", fc), ("b2", fb), ("a2", fa), ("c2", fc)):
            t[name] = bench.timed(fn, graph=True, reps=20)
        same = float((fa()[0].sort(-1).values == fc()[0].sort(-1).values).all(-1).float().mean())
        ta, tb, tc = min(t["a"], t["a2"]), t["b"], min(t["c"], t["c2"])
        lines.append(f"{m:5d}  {t['a']:6.2f} {t['a2']:6.2f}   {t['b']:6.2f}   {t['b2']:6.2f}   {t['c']:7.2f} {t['c2']:7.2f}   "
                     f"{ta / min(tb, t['b2']):5.2f}   {same:.4f}")
        print(lines[-1], flush=True)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
