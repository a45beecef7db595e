"""Development tool: the DSA lightning indexer timed per shape, in the same run:
  logits  hpc.mla_indexer_logits_fp8 into a given output;
  topk    hpc.mla_indexer_topk over those logits;
  fused   hpc.mla_indexer_topk_fp8 (the two launches through the cached scratch);
  eager   the eager-torch indexer on the same inputs (tests/mla_indexer_ref.py::indexer_eager: a gather of the index keys through
          the page table, a [T, Hi, L] einsum in bf16, ReLU and a weighted head sum, a mask, torch.topk, a sort) - the way to run
          the indexer without the ops.  Its lists are compared with the fused op's (the share of common positions is printed:
          its logits are rounded differently, so near-ties may fall either way);
  stream  the logits time's fraction of the index-key stream, visible tokens x 132 B at 8 TB/s.
Times are device-event times of a replayed hipGraph holding one call, median of 20 replays after warm-up (bench.timed): the
method of tools/tune_mla_sparse.py.  `spread` is the largest difference between three such medians of the fused call.
In front of the table: the logits op's worst err / (2^-24 A) against the float64 statement on the random inputs of
tests/test_mla_indexer.py, per configuration (A: the statement with absolute values everywhere and no ReLU).
usage: python tools/tune_mla_indexer.py [--out FILE] [--shapes 0,1,...] [--no-eager] [--no-error]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, bench, hpc  # noqa: E402,E401
import mla_indexer_ref as ir  # noqa: E402
from hpc import _C  # noqa: E402

P, HI, TOPK = 64, 64, 2048
# (name, B, context (None: bench.py's 128 - 32k mix), mtp)
SHAPES = [("8k", 64, 8192, 0), ("mix", 64, None, 0), ("4k", 8, 4096, 1), ("64k", 1, 65536, 0), ("1k", 64, 1024, 0)]


def inputs(B, ctx, sq, dev):
    """(lens on the host, q codes, weights, the cache, block_ids, lens on the device): lens include the sq new tokens"""
    lens = torch.full((B,), ctx, dtype=torch.int32) if ctx else bench.c3_lens()[:B]
    nb = (lens + P - 1) // P
    total = int(nb.sum())
    pool = total + 8

    def codes(*shape):
        raw = torch.randint(0, 256, shape, dtype=torch.int32, device=dev)
        raw[(raw & 0x7F) == 0x7F] = 0x38  # no NaN code
        return raw.to(torch.uint8)

    cache = torch.empty(pool, P * ir.TOKEN_BYTES, dtype=torch.uint8, device=dev)
    cache[:, : P * ir.DIM] = codes(pool, P * ir.DIM)
    cache[:, P * ir.DIM:].view(torch.float32).copy_(torch.exp2(-6 + 4 * torch.rand(pool, P, device=dev)))
    q = codes(B * sq, HI, ir.DIM).view(ir.F8)
    w = torch.randn(B * sq, HI, device=dev)
    perm = torch.randperm(pool)[:total].to(torch.int32)
    bid = torch.zeros(B, int(nb.max()), dtype=torch.int32)
    off = 0
    for i, n in enumerate(nb.tolist()):
        bid[i, :n] = perm[off: off + n]
        off += n
    return lens, q, w, cache, bid.to(dev), lens.to(dev)


def error_lines(dev):
    lines, worst = [], 0.0
    for Hi, mtp, p in ir.CONFIGS:
        inp = ir.inputs(Hi, mtp, p, exact=False)
        want, A = ir.statement(inp), ir.statement(inp, absolute=True)
        out = torch.full(want.shape, float("nan"), dtype=torch.float32, device=dev)
        hpc.mla_indexer_logits_fp8(inp["q"].to(dev), inp["weights"].to(dev), inp["k_cache"].to(dev), inp["block_ids"].to(dev),
                                   inp["lens_total"].to(dev), mtp=mtp, new_kv_included=True, output=out)
        ratio = ir.worst_ratio(out, want, A)
        worst = max(worst, ratio)
        lines.append(f"# logits error, random inputs, (Hi, mtp, P) = ({Hi}, {mtp}, {p}): worst err / (2^-24 A) = {ratio:.1f}")
    lines.append(f"# logits error: largest ratio {worst:.1f} (the rounding model's 256 is not kept by the matrix instruction; "
                 "the tests' bar is twice this rounded up to a power of two)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="", help="indices into SHAPES (default: all)")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-error", action="store_true")
    a = ap.parse_args()
    shapes = [int(v) for v in a.shapes.split(",") if v]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = ["# mla_indexer_logits_fp8 / mla_indexer_topk / mla_indexer_topk_fp8 on %d CUs (%s library), pages of %d, Hi = %d, "
             "topk = %d; us per call: one call in a replayed hipGraph, median of 20"
             % (_C.cu_count(dev), "development" if _C.DEV_BUILD else "product", P, HI, TOPK)]
    if not a.no_error:
        lines += error_lines(dev)
        print("\n".join(lines), flush=True)
    lines.append("# shape B ctx mtp | logits us  topk us  sum | fused us (spread)  fused/sum | eager us  eager/fused  common | "
                 "stream us  frac of logits")
    for idx, (name, B, ctx, mtp) in enumerate(SHAPES):
        if shapes and idx not in shapes:
            continue
        sq = mtp + 1
        lens, q, w, cache, bid, lens_d = inputs(B, ctx, sq, dev)
        cols = bid.shape[1] * P
        logits = torch.full((B * sq, cols), float("nan"), dtype=torch.float32, device=dev)
        ids = torch.empty(B * sq, TOPK, dtype=torch.int32, device=dev)
        ids2 = torch.empty_like(ids)

        def f_logits():
            return hpc.mla_indexer_logits_fp8(q, w, cache, bid, lens_d, mtp=mtp, new_kv_included=True, output=logits)

        def f_topk():
            return hpc.mla_indexer_topk(logits, lens_d, TOPK, mtp=mtp, new_kv_included=True, output=ids)

        def f_fused():
            return hpc.mla_indexer_topk_fp8(q, w, cache, bid, lens_d, TOPK, mtp=mtp, new_kv_included=True, output=ids2)

        def f_eager():
            return ir.indexer_eager(q, w, cache, bid, lens_d, sq, TOPK)

        # the results must agree before their times mean anything
        f_logits(), f_topk(), f_fused()
        torch.cuda.synchronize()
        assert torch.equal(ids, ids2) and int((ids >= 0).sum()) > 0, name
        common = float("nan")
        if not a.no_eager:
            want = f_eager()
            torch.cuda.synchronize()
            kk = want.shape[1]
            hit = (ids2[:, :kk, None].long() == want[:, None, :256]).any(1) | (want[:, :256] < 0)  # a sample of each eager list
            common = float(hit.float().mean())
            assert common > 0.98, (name, common)
            del want, hit
        t_l = bench.timed(f_logits, iters=20, graph=True)
        t_k = bench.timed(f_topk, iters=20, graph=True)
        rep = [bench.timed(f_fused, iters=20, graph=True) for _ in range(3)]
        t_f, spread = sorted(rep)[1], max(rep) - min(rep)
        t_e = float("nan") if a.no_eager else bench.timed(f_eager, iters=5, warm=2, graph=True)
        seen = sum(min(int(L), cols) for L in lens.tolist())  # the tokens the request's last q row sees: each is read once
        stream = seen * ir.TOKEN_BYTES / 8e12 * 1e6
        lines.append(f"{name:4s} {B:3d} {ctx or 0:6d} {mtp} | {t_l:8.1f} {t_k:8.1f} {t_l + t_k:8.1f} | {t_f:8.1f} ({spread:4.1f}) "
                     f"{t_f / (t_l + t_k):5.2f} | {t_e:9.1f} {t_e / t_f:6.2f} {common:5.3f} | {stream:6.2f} {stream / t_l:5.3f}")
        print(lines[-1], flush=True)
        del cache, q, w, logits, ids, ids2
        hpc.release_decode_workspaces()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
