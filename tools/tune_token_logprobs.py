"""Development tool: hpc.token_logprobs at V = 120832 for 1, 8, 64 and 256 rows (float32 and bfloat16 logits, num_top 0, 5
and 20) and for a prompt chunk of 4096 rows (bfloat16, num_top 0 and 5), timed in one run, alternating, against
  (e) the eager torch chain the op replaces: float log_softmax of logits / T, gather, compare-and-count for the rank, topk,
  (v) hpc.speculative_verify on the same rows (B = rows / 4, K = 3; one row: K = 0) - the reference point for one pass
      over those logits.
Every form is timed the way bench.py times its sampler row - device events round replays of a hipGraph, median of 30 - and
twice over: a graph of ONE call (what a step that ends in the op sees, replay overhead included) and a graph of REPS = 16
back-to-back calls (the op itself).  Each timing is taken twice, the forms alternating, and both are printed.  The calls of
a graph go round a ring of logits buffers that together exceed the 256 MiB Infinity Cache where 16 buffers can; the small
batches stay cache resident, as they are behind an LM head that has just written them.  Beside the op's time: the logits
bytes over 8 TB/s, and for the 4096-row chunk the share of that bound the op reaches.
usage: python tools/tune_token_logprobs.py [--out FILE]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT))
import torch, bench, hpc  # noqa: E402,E401

V, REPS, PEAK, T = 120832, 16, 8e12, 0.8
CASES = [(rows, dtype, k) for dtype in (torch.float32, torch.bfloat16) for rows in (1, 8, 64, 256) for k in (0, 5, 20)]
CASES += [(4096, torch.bfloat16, 0), (4096, torch.bfloat16, 5)]


def eager(lg, tok, k):
    lp = torch.log_softmax(lg.float() / T, -1)
    t = tok.view(-1, 1)
    tlp = lp.gather(1, t).squeeze(1)
    rank = (lg > lg.gather(1, t)).sum(-1) + 1
    top = torch.topk(lp, k, dim=-1) if k else None
    return tlp, rank, top


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
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = ["# hpc.token_logprobs, V = %d, T = %.1f; us per call, hipGraph replays, median of 30; x1 = one call per graph, x%d = %d "
             "calls per graph round a ring of logits buffers; every timing twice; [bound] = logits bytes / 8 TB/s" % (V, T, REPS, REPS),
             "# dtype rows num_top sets | (l) token_logprobs x1, again; x%d, again [bound] | (e) eager torch x1, again; x%d, again | "
             "(v) speculative_verify x%d, again | (l)/(e) x1  x%d | (l)/(v) x%d | share of bound" % ((REPS,) * 5)]
    for rows, dtype, k in CASES:
        nbytes = rows * V * (4 if dtype == torch.float32 else 2)
        nset = max(2, min(REPS, -(-(512 << 20) // nbytes)))
        sets = [dict(lg=(2 * torch.randn(rows, V, device=dev)).to(dtype)) for _ in range(nset)]
        tok = torch.randint(0, V, (rows,), device=dev)
        B, K = (rows // 4, 3) if rows % 4 == 0 else (rows, 0)
        draft = torch.randint(0, V, (B, K), device=dev)
        outs = [torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                torch.empty(rows, k, dtype=torch.int32, device=dev), torch.empty(rows, k, device=dev)]
        vout, vacc = torch.empty(B, K + 1, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        forms = {
            "l": lambda s: hpc.token_logprobs(s["lg"], tok, T, k, *outs),
            "e": lambda s: eager(s["lg"], tok, k),
            "v": lambda s: hpc.speculative_verify(s["lg"], draft, temperature=T, seed=42, output_token_ids=vout, num_accepted=vacc),
        }
        us = {}
        for name in ("l1", "e1", "l16", "e16", "v16", "l1b", "e1b", "l16b", "e16b", "v16b"):
            form, reps = name[0], (REPS if "16" in name else 1)
            us[name] = bench.timed(ring(forms[form], sets), graph=True, reps=reps)
        best = {n: min(us[n], us[n + "b"]) for n in ("l1", "e1", "l16", "e16", "v16")}
        bound = nbytes / PEAK * 1e6
        lines.append(f"{str(dtype)[6:]:8s} {rows:4d} {k:2d} {nset:2d} | {us['l1']:8.2f} {us['l1b']:8.2f}; {us['l16']:8.2f} {us['l16b']:8.2f} "
                     f"[{bound:6.2f}] | {us['e1']:9.2f} {us['e1b']:9.2f}; {us['e16']:9.2f} {us['e16b']:9.2f} | "
                     f"{us['v16']:8.2f} {us['v16b']:8.2f} | {best['l1'] / best['e1']:6.3f} {best['l16'] / best['e16']:6.3f} | "
                     f"{best['l16'] / best['v16']:5.2f} | {bound / best['l16']:5.3f}")
        print(lines[-1], flush=True)
        del sets
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
