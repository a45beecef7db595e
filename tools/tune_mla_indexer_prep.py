"""Development tool: the indexer's front end timed per shape, in the same run:
  op      hpc.mla_indexer_prep_fp8 with every output given (one launch);
  chain   the eager-torch chain it replaces on the same inputs (tests/mla_indexer_prep_ref.py::prep_eager: LayerNorm, RoPE, a
          matmul by the Hadamard matrix, hpc.blockwise_fp8_quant, the fold, hpc.mla_indexer_store_k_fp8);
  store   hpc.mla_indexer_store_k_fp8 alone on a ready key: the floor of anything that writes the cache;
  hbm     the bytes the op must move, T * ((1 + Hi) * 128 * 2 + Hi * 128 + 132 + 8 * Hi), at 8 TB/s, and its fraction of the
          op's time.
Times are device-event times of a replayed hipGraph, median of 20 replays after warm-up (bench.timed), with one call per replay
(`x1`: what a decode step pays, launch floor included) and with 16 calls per replay divided by 16 (`x16`: the kernel itself).
`spread` is the largest difference between three such x1 medians of the op.  Before a shape is timed the op's codes are
compared with the chain's (the share of equal bytes is printed: the chain rounds LayerNorm and the matmul differently, so a
code next to a rounding boundary may fall either way) and its cache with the chain's.
usage: python tools/tune_mla_indexer_prep.py [--out FILE] [--shapes 0,1,...]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, bench, hpc  # noqa: E402,E401
import mla_indexer_prep_ref as pr  # noqa: E402
from hpc import _C  # noqa: E402

P, HI, CTX, MAX_POS = 64, 64, 8192, 16384
# (name, requests, new tokens per request)
SHAPES = [("T 1", 1, 1), ("T 64", 64, 1), ("T 256", 256, 1), ("64 x mtp 3", 64, 4), ("prefill 4096", 1, 4096), ("prefill 8192", 2, 4096)]


def inputs(B, new, dev):
    T = B * new
    total = CTX if new < P else new  # decode: the new tokens end a context of 8192; prefill: the chunk is the context
    nb = -(-total // P)
    bid = torch.randperm(B * nb + 4)[: B * nb].to(torch.int32).view(B, nb)
    return dict(T=T, k=torch.randn(T, 128, device=dev).bfloat16(), q=torch.randn(T, HI, 128, device=dev).bfloat16(),
                hw=torch.randn(T, HI, device=dev), w=torch.randn(128, device=dev), b=torch.randn(128, device=dev),
                cs=pr.ms.orc.generate_cos_sin_cache(MAX_POS, 64).to(dev), ns=torch.full((B,), total, dtype=torch.int32, device=dev),
                qi=(torch.arange(B + 1, dtype=torch.int32) * new).to(dev), bid=bid.to(dev), pool=B * nb + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="", help="indices into SHAPES (default: all)")
    a = ap.parse_args()
    shapes = [int(v) for v in a.shapes.split(",") if v]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    H = pr.hadamard_matrix().to(device=dev, dtype=torch.float32)
    ss = 128 ** -0.5
    lines = ["# mla_indexer_prep_fp8 on %d CUs (%s library), pages of %d, Hi = %d; us per call in a replayed hipGraph, median of 20: "
             "x1 one call per replay, x16 sixteen per replay / 16" % (_C.cu_count(dev), "development" if _C.DEV_BUILD else "product", P, HI),
             "# shape  T | op x1 (spread)  op x16 | chain x1  chain x16  chain/op x1  x16 | store x1  store x16 | hbm us  frac of op x16 | "
             "codes equal"]
    for idx, (name, B, new) in enumerate(SHAPES):
        if shapes and idx not in shapes:
            continue
        d = inputs(B, new, dev)
        T = d["T"]
        cache = torch.zeros(d["pool"], P * 132, dtype=torch.uint8, device=dev)
        cache2 = torch.zeros_like(cache)
        out_k = torch.empty(T, 128, dtype=torch.bfloat16, device=dev)
        q8 = torch.empty(T, HI, 128, device=dev).to(pr.F8)
        wt = torch.empty(T, HI, device=dev)

        def f_op():
            return hpc.mla_indexer_prep_fp8(cache, d["k"], d["w"], d["b"], d["cs"], d["ns"], d["qi"], d["bid"], q=d["q"],
                                            head_weights=d["hw"], softmax_scale=ss, out_k=out_k, out_q=q8, out_weights=wt)

        def f_chain():
            return pr.prep_eager(cache2, d["k"], d["w"], d["b"], d["cs"], d["ns"], d["qi"], d["bid"], d["q"], d["hw"], ss, hadamard=H)

        def f_store():
            return hpc.mla_indexer_store_k_fp8(cache2, out_k, d["ns"], d["qi"], d["bid"])

        # the results must agree before their times mean anything
        f_op()
        c8, cw = f_chain()
        torch.cuda.synchronize()
        same = float((c8.view(torch.uint8) == q8.view(torch.uint8)).float().mean())
        same_cache = float((cache == cache2).float().mean())
        close_w = bool(torch.allclose(cw, wt, rtol=2e-2, atol=1e-6))
        assert same > 0.97 and same_cache > 0.97 and close_w and int((cache != 0).sum()) > 0, (name, same, same_cache, close_w)
        del c8, cw
        rep = [bench.timed(f_op, iters=20, graph=True) for _ in range(3)]
        t1, spread = sorted(rep)[1], max(rep) - min(rep)
        t16 = bench.timed(f_op, iters=20, graph=True, reps=16)
        c1 = bench.timed(f_chain, iters=10, warm=2, graph=True)
        c16 = bench.timed(f_chain, iters=5, warm=1, graph=True, reps=16)
        s1 = bench.timed(f_store, iters=20, graph=True)
        s16 = bench.timed(f_store, iters=20, graph=True, reps=16)
        hbm = T * ((1 + HI) * 128 * 2 + HI * 128 + 132 + 8 * HI) / 8e12 * 1e6
        lines.append(f"{name:13s} {T:5d} | {t1:7.1f} ({spread:4.1f}) {t16:7.1f} | {c1:8.1f} {c16:8.1f} {c1 / t1:6.2f} {c16 / t16:6.2f} | "
                     f"{s1:6.1f} {s16:6.1f} | {hbm:6.2f} {hbm / t16:5.3f} | {same:6.4f}")
        print(lines[-1], flush=True)
        if not (t1 < c1 and t16 < c16):
            lines.append(f"# {name}: the op is NOT faster than the chain")
        del cache, cache2, out_k, q8, wt, d
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
