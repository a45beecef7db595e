"""Development tool: DSA prefill timed per shape, every figure of a shape in the same run:
  logits / topk / fused   hpc.mla_indexer_logits_prefill_fp8 into a given output, hpc.mla_indexer_topk_prefill over it, and
                          hpc.mla_indexer_topk_prefill_fp8 (row slabs through the cached scratch);
  per-row                 the same three through the DECODE ops on the expanded form - every row of the chunk its own one-row
                          request with a copy of its request's page-table row, B = T - which is what a caller had to do before
                          the prefill ops existed.  Its lists must equal the prefill ops' before any time is taken;
  eager                   the eager-torch indexer per request and slab of 512 rows (a gather of the request's keys, a bf16
                          einsum, ReLU, the weighted head sum, a causal mask, torch.topk, a sort);
  attn                    hpc.attention_prefill_mla_sparse_bf16 / _fp8 at 128 heads on the fused op's lists, the decode op on
                          the expanded form (the same kernel: the figure shows what the row rule costs) and eager torch
                          (tests/mla_sparse_ref.py::sparse_eager over slabs of 256 rows).
Times are device-event times of a replayed hipGraph holding one call, median of the replays after warm-up (bench.timed); eager
torch is timed without a graph.  Every shape runs in a child process of its own under its own time limit; the first shape that
fails ends the run.
usage: python tools/tune_mla_indexer_prefill.py [--out FILE] [--shapes 0,1,...] [--no-eager] [--limit SECONDS]"""
import argparse
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
P, HI, TOPK, H = 64, 64, 2048, 128
# (name, requests, new rows per request (None: 16 .. 512), cached context per request (None: bench.py's 128 .. 32k mix))
SHAPES = [("1x4096 fresh", 1, 4096, 0), ("4x4096 fresh", 4, 4096, 0), ("4096 over 28k", 1, 4096, 28672), ("64 ragged", 64, None, None)]


def child(idx, no_eager):
    sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    import torch, bench, hpc  # noqa: E401
    import mla_indexer_ref as ir
    import mla_sparse_ref as sr

    name, B, new, ctx = SHAPES[idx]
    dev = torch.device("cuda", 0)
    torch.manual_seed(idx)
    g = torch.Generator().manual_seed(idx)
    new_t = torch.full((B,), new, dtype=torch.int32) if new else torch.randint(16, 513, (B,), generator=g, dtype=torch.int32)
    ctx_t = torch.full((B,), ctx, dtype=torch.int32) if ctx is not None else bench.c3_lens()[:B]
    lens = new_t + ctx_t
    qi = torch.tensor([0] + new_t.cumsum(0).tolist(), dtype=torch.int32)
    T = int(qi[-1])
    nb = (lens + P - 1) // P
    total, max_blocks = int(nb.sum()), int(nb.max())
    pool, cols = total + 8, int(nb.max()) * P

    def codes(*shape):
        raw = torch.randint(0, 256, shape, dtype=torch.int32, device=dev)
        raw[(raw & 0x7F) == 0x7F] = 0x38  # no NaN code
        return raw.to(torch.uint8)

    k_cache = torch.empty(pool, P * ir.TOKEN_BYTES, dtype=torch.uint8, device=dev)
    k_cache[:, : P * ir.DIM] = codes(pool, P * ir.DIM)
    k_cache[:, P * ir.DIM:].view(torch.float32).copy_(torch.exp2(-6 + 4 * torch.rand(pool, P, device=dev)))
    q = codes(T, HI, ir.DIM).view(ir.F8)
    w = torch.randn(T, HI, device=dev)
    perm = torch.randperm(pool)[:total].to(torch.int32)
    bid = torch.zeros(B, max_blocks, dtype=torch.int32)
    off = 0
    for i, n in enumerate(nb.tolist()):
        bid[i, :n] = perm[off: off + n]
        off += n
    # the expanded form: what the per-row route is given
    req = torch.repeat_interleave(torch.arange(B), new_t.long())
    pos = torch.cat([torch.arange(int(c), int(c) + int(n)) for c, n in zip(ctx_t, new_t)])
    x_bid, x_lens = bid[req].contiguous().to(dev), (pos + 1).to(torch.int32).to(dev)
    bid_d, lens_d, qi_d = bid.to(dev), lens.to(dev), qi.to(dev)
    pairs = int((pos + 1).sum())

    logits = torch.empty(T, cols, dtype=torch.float32, device=dev)
    ids, ids2, ids3 = (torch.empty(T, TOPK, dtype=torch.int32, device=dev) for _ in range(3))
    iters = 20 if pairs < 5e7 else 8

    def t(fn, graph=True, n=iters):
        return bench.timed(fn, iters=n, warm=2, graph=graph)

    new_ops = dict(
        logits=lambda: hpc.mla_indexer_logits_prefill_fp8(q, w, k_cache, bid_d, lens_d, qi_d, output=logits),
        topk=lambda: hpc.mla_indexer_topk_prefill(logits, lens_d, qi_d, TOPK, output=ids),
        fused=lambda: hpc.mla_indexer_topk_prefill_fp8(q, w, k_cache, bid_d, lens_d, qi_d, TOPK, output=ids2))
    row_ops = dict(
        logits=lambda: hpc.mla_indexer_logits_fp8(q, w, k_cache, x_bid, x_lens, mtp=0, new_kv_included=True, output=logits),
        topk=lambda: hpc.mla_indexer_topk(logits, x_lens, TOPK, mtp=0, new_kv_included=True, output=ids),
        fused=lambda: hpc.mla_indexer_topk_fp8(q, w, k_cache, x_bid, x_lens, TOPK, mtp=0, new_kv_included=True, output=ids3))
    # the results must agree before their times mean anything
    new_ops["logits"](), new_ops["topk"](), new_ops["fused"](), row_ops["fused"]()
    torch.cuda.synchronize()
    assert torch.equal(ids, ids2) and torch.equal(ids2, ids3) and int((ids >= 0).sum()) > 0, name

    def eager_indexer():
        cd = k_cache[:, : P * ir.DIM].view(ir.F8).reshape(pool, P, ir.DIM)
        sc = k_cache[:, P * ir.DIM:].view(torch.float32).reshape(pool, P)
        out = []
        for b in range(B):
            L, n, c0 = int(lens[b]), int(new_t[b]), int(ctx_t[b])
            pages = bid_d[b, : -(-L // P)].long()
            k = cd[pages].reshape(-1, ir.DIM)[:L].to(torch.bfloat16)
            ks = sc[pages].reshape(-1)[:L]
            for r0 in range(0, n, 512):
                r1 = min(n, r0 + 512)
                rows = slice(int(qi[b]) + r0, int(qi[b]) + r1)
                d = torch.einsum("rhd,jd->rhj", q[rows].to(torch.bfloat16), k).float()
                lg = (d.relu() * w[rows, :, None]).sum(1) * ks[None, :]
                seen = torch.arange(L, device=dev)[None, :] <= (c0 + torch.arange(r0, r1, device=dev))[:, None]
                val, at = lg.masked_fill(~seen, float("-inf")).topk(min(TOPK, L), dim=-1)
                out.append(torch.where(seen.gather(1, at), at, torch.full_like(at, -1)).sort(-1)[0])
        return out

    res = [f"{name:14s} T {T:6d} cols {cols:6d} pairs {pairs / 1e6:8.1f} M"]
    tn = {k: t(f) for k, f in new_ops.items()}
    tr = {k: t(f) for k, f in row_ops.items()}
    te = float("nan") if no_eager else t(eager_indexer, graph=False, n=3)
    for k in ("logits", "topk", "fused"):
        res.append(f"  indexer {k:6s} | prefill op {tn[k]:10.1f} us | per-row route {tr[k]:10.1f} us | per-row / prefill {tr[k] / tn[k]:6.2f}")
    res.append(f"  indexer eager  | {te:10.1f} us | eager / fused prefill {te / tn['fused']:6.2f}")
    hpc.release_decode_workspaces()
    del logits, ids3
    torch.cuda.empty_cache()

    # the sparse attention at 128 heads on the lists above, both caches
    qa = (torch.randn(T, H, 576, device=dev) / 24).bfloat16()
    out, lse = torch.empty(T, H, 512, dtype=torch.bfloat16, device=dev), torch.empty(T, H, device=dev)
    ckv16 = torch.randn(pool, P, 576, device=dev).bfloat16()
    ckv8 = torch.empty(pool, P, 656, dtype=torch.uint8, device=dev)
    ckv8[:, :, :512] = codes(pool, P, 512)
    ckv8[:, :, 512:528].view(torch.float32).copy_(torch.exp2(-6 + 2 * torch.rand(pool, P, 4, device=dev)))
    ckv8[:, :, 528:].view(torch.bfloat16).copy_(torch.randn(pool, P, 64, device=dev).bfloat16())
    scale = 1 / 192 ** 0.5
    for kind, ckv in (("bf16", ckv16), ("fp8", ckv8)):
        f_new = lambda: getattr(hpc, "attention_prefill_mla_sparse_" + kind)(qa, ckv, bid_d, lens_d, qi_d, ids2, scale, output=out,  # noqa: E731
                                                                             output_lse=lse)
        f_row = lambda: getattr(hpc, "attention_decode_mla_sparse_" + kind)(qa, ckv, x_bid, x_lens, ids2, scale, new_kv_included=True,  # noqa: E731
                                                                            output=out, output_lse=lse)
        f_new()
        a = out.clone()
        f_row()
        torch.cuda.synchronize()
        assert torch.equal(a, out), (name, kind)
        del a
        t_new, t_row = t(f_new), t(f_row)
        line = f"  attn {kind:4s} H {H} | prefill op {t_new:10.1f} us | per-row route {t_row:10.1f} us | per-row / prefill {t_row / t_new:6.2f}"
        if kind == "bf16" and not no_eager:
            def f_eager():
                return [sr.sparse_eager(qa[r0: r0 + 256], ckv16, x_bid[r0: r0 + 256], x_lens[r0: r0 + 256], ids2[r0: r0 + 256], 1, scale)
                        for r0 in range(0, T, 256)]
            t_e = t(f_eager, graph=False, n=2)
            line += f" | eager {t_e:10.1f} us, eager / prefill {t_e / t_new:6.2f}"
        res.append(line)
    print("\n".join(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="", help="indices into SHAPES (default: all)")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.no_eager)
    shapes = [int(v) for v in a.shapes.split(",") if v] or list(range(len(SHAPES)))
    lines = ["# DSA prefill: mla_indexer_logits_prefill_fp8 / mla_indexer_topk_prefill / mla_indexer_topk_prefill_fp8 and "
             "attention_prefill_mla_sparse_bf16 / _fp8 (product library), pages of %d, Hi = %d, topk = %d, %d attention heads; "
             "us per call: one call in a replayed hipGraph, median; per-row route: the decode ops with B = T one-row requests; "
             "pairs: visible (row, key) pairs" % (P, HI, TOPK, H)]
    for idx in shapes:  # a child process and a time limit per shape; nothing more is started after a failure
        cmd = [sys.executable, __file__, "--child", str(idx)] + (["--no-eager"] if a.no_eager else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"# shape {idx} ({SHAPES[idx][0]}): ended at its time limit of {a.limit} s; the run stops here")
            break
        if r.returncode != 0:
            lines.append(f"# shape {idx} ({SHAPES[idx][0]}): exit status {r.returncode}; the run stops here\n# " +
                         "\n# ".join(r.stderr.strip().splitlines()[-6:]))
            break
        lines.append(r.stdout.rstrip())
        print(lines[-1], flush=True)
    if lines[-1].startswith("#") and len(lines) > 1:
        print(lines[-1], flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
