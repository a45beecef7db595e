"""Development tool: draft-token verification (hpc.speculative_verify) at V = 120832 for (B, K) in (1, 3), (8, 3), (64, 3),
(64, 1), float32 and bfloat16 logits, self-drawn noise, timed in one run, alternating, against
  (f) hpc.fused_sampler's temperature path on the same B (K + 1) rows - the yardstick: the same bytes read once, the same
      Philox draw and Gumbel score per element; the new op adds an exp per element - timed twice for the spread,
  (e) the eager torch composition the op replaces: softmax(logits / T), gather, compare, cumprod, masked second sampling
      (the exponential race on the probabilities with the draft zeroed), index writes.
Every call is timed the way bench.py times its sampler row: a hipGraph of REPS back-to-back calls, median of 30 replays,
device events.  The calls of a graph go round a ring of logits buffers that together exceed the 256 MiB Infinity Cache where
REPS buffers can (B = 64; the small batches stay cache resident, as they are behind an LM head that has just written them).
Beside each time: the logits bytes over 8 TB/s.
usage: python tools/tune_spec_verify.py [--out FILE]
       rocprofv3 --kernel-trace --stats ... -- python tools/tune_spec_verify.py --plain   (B = 64, K = 3: 20 plain launches of
       (v) and (f) per dtype, for the per-kernel times: segment pass against segment pass, final against final)"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT))
import torch, bench, hpc  # noqa: E402,E401

V, REPS, PEAK, T = 120832, 6, 8e12, 0.8


def eager(lg, draft, B, K):
    probs = torch.softmax(lg.float() / T, -1).view(B, K + 1, V)
    p = probs[:, :K].gather(2, draft.unsqueeze(-1)).squeeze(-1)
    acc = (torch.rand(B, K, device=lg.device) < p).long().cumprod(1).sum(1)
    q = probs.clone()
    q[:, :K].scatter_(2, draft.unsqueeze(-1), 0.0)
    tok = (q / torch.empty_like(q).exponential_()).argmax(-1)
    pos = torch.arange(K + 1, device=lg.device).expand(B, K + 1)
    padded = torch.nn.functional.pad(draft, (0, 1), value=-1)
    out = torch.where(pos < acc[:, None], padded, torch.where(pos == acc[:, None], tok, torch.full_like(tok, -1)))
    return out.int(), acc.int()


def ring(fn, sets):
    """one callable that walks the ring: call i of a captured graph uses set i % len(sets)"""
    state = {"i": 0}

    def call():
        s = sets[state["i"] % len(sets)]
        state["i"] += 1
        return fn(s)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--plain", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if a.plain:
        B, K = 64, 3
        draft = torch.randint(0, V, (B, K), device=dev)
        for dtype in (torch.float32, torch.bfloat16):
            lg = (2 * torch.randn(B * (K + 1), V, device=dev)).to(dtype)
            for _ in range(20):
                hpc.speculative_verify(lg, draft, temperature=T, seed=42)
                hpc.fused_sampler(lg, temperature=T, seed=42)
            torch.cuda.synchronize()
        return
    lines = ["# hpc.speculative_verify, V = %d, T = %.1f, self-drawn noise; us per call, hipGraph of %d calls round a ring of logits "
             "buffers, median of 30 replays; [bound] = logits bytes / 8 TB/s" % (V, T, REPS),
             "# dtype B K rows sets | (v) speculative_verify, again [bound] | (f) fused_sampler temperature path, again | "
             "(e) eager torch, again | (v)/(f)  (f) spread  (v)/(e)"]
    for dtype in (torch.float32, torch.bfloat16):
        for B, K in ((1, 3), (8, 3), (64, 3), (64, 1)):
            rows = B * (K + 1)
            nbytes = rows * V * (4 if dtype == torch.float32 else 2)
            nset = max(2, min(REPS, -(-(512 << 20) // nbytes)))
            sets = [dict(lg=(2 * torch.randn(rows, V, device=dev)).to(dtype)) for _ in range(nset)]
            draft = torch.randint(0, V, (B, K), device=dev)
            out = torch.empty(B, K + 1, dtype=torch.int32, device=dev)
            acc = torch.empty(B, dtype=torch.int32, device=dev)
            forms = {
                "v": lambda s: hpc.speculative_verify(s["lg"], draft, temperature=T, seed=42, output_token_ids=out, num_accepted=acc),
                "f": lambda s: hpc.fused_sampler(s["lg"], temperature=T, seed=42),
                "e": lambda s: eager(s["lg"], draft, B, K),
            }
            us = {}
            for name in ("v", "f", "e", "f2", "v2", "e2"):
                us[name] = bench.timed(ring(forms[name.rstrip("2")], sets), graph=True, reps=REPS)
            bv, bf, be = min(us["v"], us["v2"]), min(us["f"], us["f2"]), min(us["e"], us["e2"])
            lines.append(f"{str(dtype)[6:]:8s} {B:3d} {K:2d} {rows:4d} {nset:2d} | {us['v']:8.2f} {us['v2']:8.2f} [{nbytes / PEAK * 1e6:6.2f}] | "
                         f"{us['f']:8.2f} {us['f2']:8.2f} | {us['e']:9.2f} {us['e2']:9.2f} | {bv / bf:5.2f}  "
                         f"{max(us['f'], us['f2']) / bf:5.2f}  {bv / be:6.3f}")
            print(lines[-1], flush=True)
            del sets
            torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
