"""Development tool: the 128-block activation quantisers in front of the blockwise fused MoE, timed in one run, alternating:
  (q)  hpc.blockwise_fp8_quant on bf16 rows,
  (n)  hpc.fused_rmsnorm_blockwise_quant plain, (nr) with residual, (nry) with residual and the normed bf16 output,
  (y)  hpc.fused_rmsnorm_with_scale at the same shape - the yardstick: it moves the bytes of (n) and shares its row layout -
       timed twice for the spread,
  (eq) / (en) the eager torch compositions the ops replace: the quantisation alone, and residual add + RMSNorm + quantisation.
Every call is timed the way bench.py times its router row: a hipGraph of 20 back-to-back calls, median of 30 replays.  The
20 calls go round a ring of input / output sets that together exceed the 256 MiB Infinity Cache (at least 2 sets), so the
large shapes are read from HBM, not from the previous call's lines.  Beside each time: the form's algorithmic bytes over
8 TB/s.
usage: python tools/tune_blockwise_quant.py [--out FILE]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT))
import torch, bench, hpc  # noqa: E402,E401

F8, BF16, EPS, REPS, PEAK = torch.float8_e4m3fn, torch.bfloat16, 1e-6, 20, 8e12


def eager_quant(x):
    t, h = x.shape
    b = x.float().view(t, h // 128, 128)
    s = b.abs().amax(-1) / 448.0
    inv = 1.0 / (s + 1e-8)
    return (b * inv.unsqueeze(-1)).to(F8).view(t, h), s


def eager_norm(a, w, r):
    h32 = r.float().add_(a.float())
    r.copy_(h32)
    h32 = r.float()
    y = (h32 * torch.rsqrt(h32.pow(2).mean(-1, keepdim=True) + EPS) * w.float()).to(BF16)
    return eager_quant(y) + (y,)


def ring(fn, sets):
    """one callable that walks the ring: call i of the captured 20 uses set i % len(sets)"""
    state = {"i": 0}

    def call():
        s = sets[state["i"] % len(sets)]
        state["i"] += 1
        return fn(s)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    one = torch.ones(1, device=dev)
    lines = ["# 128-block e4m3 quantisers; us per call, hipGraph of %d calls round a ring of buffer sets, median of 30 replays; "
             "[bound] = algorithmic bytes / 8 TB/s" % REPS,
             "# T H sets | (q) quant [bound] | (n) norm+quant [bound] | (nr) +residual [bound] | (nry) +normed out [bound] | "
             "(y) fused_rmsnorm_with_scale, again | (eq) eager quant | (en) eager add+norm+quant | (n)/(y) (q)/(eq) (nry)/(en)"]
    for h in (4096, 7168):
        w = (torch.rand(h, device=dev) + 0.5).to(BF16)
        for t in (1, 16, 64, 256, 4096):
            per_set = t * h * 9 + t * (h // 128) * 4  # a, residual, normed: 2 B each; q: 1 B; scales
            nset = max(2, min(REPS, -(-(512 << 20) // per_set)))
            sets = [dict(a=torch.randn(t, h, device=dev).to(BF16), r=torch.randn(t, h, device=dev).to(BF16),
                         q=torch.empty(t, h, dtype=F8, device=dev), s=torch.empty(t, h // 128, device=dev),
                         y=torch.empty(t, h, dtype=BF16, device=dev)) for _ in range(nset)]
            forms = {
                "q": lambda s: hpc.blockwise_fp8_quant(s["a"], s["q"], s["s"]),
                "n": lambda s: hpc.fused_rmsnorm_blockwise_quant(s["a"], w, EPS, None, False, s["q"], s["s"]),
                "nr": lambda s: hpc.fused_rmsnorm_blockwise_quant(s["a"], w, EPS, s["r"], False, s["q"], s["s"]),
                "nry": lambda s: hpc.fused_rmsnorm_blockwise_quant(s["a"], w, EPS, s["r"], True, s["q"], s["s"], s["y"]),
                "y": lambda s: hpc.fused_rmsnorm_with_scale(s["a"], w, EPS, one),
                "eq": lambda s: eager_quant(s["a"]),
                "en": lambda s: eager_norm(s["a"], w, s["r"]),
            }
            us = {}
            for name in ("q", "n", "nr", "nry", "y", "eq", "en", "y2", "nry2", "nr2", "n2", "q2"):
                us[name] = bench.timed(ring(forms[name.rstrip("2")], sets), graph=True, reps=REPS)
            sc = t * (h // 128) * 4
            bound = {"q": t * h * 3 + sc, "n": t * h * 3 + sc + 2 * h, "nr": t * h * 7 + sc + 2 * h, "nry": t * h * 9 + sc + 2 * h}
            best = {k: min(us[k], us[k + "2"]) for k in ("q", "n", "nr", "nry", "y")}
            lines.append(
                f"{t:5d} {h:5d} {nset:2d} | " +
                " | ".join(f"{us[k]:7.2f} {us[k + '2']:7.2f} [{bound[k] / PEAK * 1e6:6.2f}]" for k in ("q", "n", "nr", "nry")) +
                f" | {us['y']:7.2f} {us['y2']:7.2f} | {us['eq']:8.2f} | {us['en']:8.2f} | "
                f"{best['n'] / best['y']:5.2f} {best['q'] / us['eq']:6.3f} {best['nry'] / us['en']:6.3f}")
            print(lines[-1], flush=True)
            del sets
            torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
