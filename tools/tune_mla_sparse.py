"""Development tool: hpc.attention_decode_mla_sparse_bf16 / _fp8 timed per shape at splits = 0 (the route's rule) and over a sweep
of caller split counts, beside in the same run:
  dense   hpc.attention_decode_mla_bf16 / _fp8 at splits = 0 over the FULL context of the same requests - what a caller without
          the sparse op can run natively (it computes another attention: every token, not the listed ones);
  eager   the eager-torch statement on the same inputs (tests/mla_sparse_ref.py::sparse_eager: index arithmetic, a row gather
          through the page table, two batched matmuls, a masked softmax) - the way to run THIS attention without the op;
  stream  the time's fraction of the gathered-row stream, B * Sq * valid entries x 1,152 B (bf16) or x 656 B (FP8), at 8 TB/s.
          Rows two heads tiles or two q rows share are counted once per workgroup that fetches them only in the time, not here.
Times are device-event times of a replayed hipGraph holding one call, median of 20 replays after warm-up (bench.timed): the
method of tools/tune_mla.py.  `spread` is the largest difference between three such medians of the splits = 0 call of the bf16
op; a difference between two split counts below it says nothing.
The lists: per q row a random sample without replacement of topk visible positions, in random order; a row that sees fewer than
topk tokens lists them all and ends in -1 padding (the 1k shape: half of every list).  The FP8 cache is the project's 128-column
quantisation of the same random latents; the bf16 ops run on its dequantisation and the two sparse outputs must be bit-equal, and
within 3e-2 of the eager result, before their times are taken.
usage: python tools/tune_mla_sparse.py [--out FILE] [--splits 1,2,4,8,16,32] [--shapes 0,1,...] [--no-eager]"""
import argparse
import ctypes
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import torch, bench, hpc  # noqa: E402,E401
import mla_sparse_ref as sr  # noqa: E402
import tune_mla  # noqa: E402  (inputs, to_fp8_cache: the dense tool's generators)
from hpc import _C  # noqa: E402

BF16, P, SCALE = tune_mla.BF16, tune_mla.P, tune_mla.SCALE
# (name, B, context (None: bench.py's 128 - 32k mix), H, mtp, topk)
SHAPES = [("8k", 64, 8192, 16, 0, 2048), ("8k", 64, 8192, 128, 0, 2048), ("mix", 64, None, 128, 0, 2048),
          ("4k", 8, 4096, 128, 1, 2048), ("64k", 1, 65536, 128, 0, 2048), ("1k", 64, 1024, 128, 0, 2048)]


def plan(B, sq, H, topk, splits):
    s, mx, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    rc = _C.lib.hpc_attention_decode_mla_sparse_plan(B, sq, H, topk, splits, 0, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws),
                                                     None, None)
    assert rc == 0, rc
    return s.value


def lists(lens, sq, topk, dev):
    """(indices int32 [B * sq, topk] on the device, valid entries in all): lens include the sq new tokens"""
    rows, valid = [], 0
    for L in lens.tolist():
        for s in range(sq):
            vis = L - sq + s + 1
            pick = torch.randperm(vis)[:topk].to(torch.int32)
            valid += len(pick)
            rows.append(torch.nn.functional.pad(pick, (0, topk - len(pick)), value=-1))
    return torch.stack(rows).to(dev), valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--splits", default="1,2,4,8,16,32")
    ap.add_argument("--shapes", default="", help="indices into SHAPES (default: all)")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    sweep = [int(v) for v in a.splits.split(",") if v]
    shapes = [int(v) for v in a.shapes.split(",") if v]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = ["# attention_decode_mla_sparse_bf16 / _fp8 on %d CUs (%s library), pages of %d; us per call: one call in a replayed "
             "hipGraph, median of 20" % (_C.cu_count(dev), "development" if _C.DEV_BUILD else "product", P),
             "# dense: attention_decode_mla_bf16 / _fp8 at splits 0 over the full context; eager: the torch statement of the sparse "
             "attention (bf16); stream: valid entries x 1,152 B (bf16) / 656 B (fp8) at 8 TB/s",
             "# shape B ctx H mtp topk valid/list | splits(0) | sparse bf16 us (spread)  fp8 us | best split: bf16 us, fp8 us | "
             "dense bf16 us  fp8 us | sparse/dense bf16 fp8 | eager us  eager/op | stream frac bf16 fp8 | "
             "bf16 us at splits " + ",".join(map(str, sweep)) + " | fp8 us at the same"]
    for idx, (name, B, ctx, H, mtp, topk) in enumerate(SHAPES):
        if shapes and idx not in shapes:
            continue
        sq = mtp + 1
        lens, ckv, q, bid, lens_d = tune_mla.inputs(B, ctx, H, sq, dev)
        cache, deq = tune_mla.to_fp8_cache(ckv)
        del ckv
        ind, valid = lists(lens, sq, topk, dev)
        out = {k: torch.empty(B * sq, H, 512, dtype=BF16, device=dev) for k in ("s16", "s8", "d16", "d8")}

        def sparse(kind, splits):
            fn, c, o = ((hpc.attention_decode_mla_sparse_fp8, cache, out["s8"]) if kind == "fp8"
                        else (hpc.attention_decode_mla_sparse_bf16, deq, out["s16"]))
            return lambda: fn(q, c, bid, lens_d, ind, SCALE, mtp=mtp, new_kv_included=True, output=o, splits=splits)

        def dense(kind):
            fn, c, o = ((hpc.attention_decode_mla_fp8, cache, out["d8"]) if kind == "fp8"
                        else (hpc.attention_decode_mla_bf16, deq, out["d16"]))
            return lambda: fn(q, c, bid, lens_d, SCALE, mtp=mtp, new_kv_included=True, output=o, splits=0)

        def eager():
            return sr.sparse_eager(q, deq, bid, lens_d, ind, sq, SCALE)

        # the results must agree before their times mean anything
        sparse("bf16", 0)(), sparse("fp8", 0)()
        torch.cuda.synchronize()
        assert torch.equal(out["s8"], out["s16"]) and bool(out["s16"].float().abs().max() > 0), (name, H)
        if not a.no_eager:
            want = eager()
            torch.cuda.synchronize()
            diff = (out["s16"].float() - want.float()).abs().max().item() / want.float().abs().max().item()
            assert diff < 3e-2, (name, H, diff)
            del want
        rep = [bench.timed(sparse("bf16", 0), iters=20, graph=True) for _ in range(3)]
        us16, spread = sorted(rep)[1], max(rep) - min(rep)
        us8 = bench.timed(sparse("fp8", 0), iters=20, graph=True)
        t16 = [bench.timed(sparse("bf16", s), iters=20, graph=True) for s in sweep]
        t8 = [bench.timed(sparse("fp8", s), iters=20, graph=True) for s in sweep]
        d16, d8 = bench.timed(dense("bf16"), iters=20, graph=True), bench.timed(dense("fp8"), iters=20, graph=True)
        us_e = float("nan") if a.no_eager else bench.timed(eager, iters=5, warm=2, graph=True)
        b16, b8 = min(zip(t16, sweep)), min(zip(t8, sweep))
        s16, s8 = valid * 1152 / 8e12 * 1e6, valid * 656 / 8e12 * 1e6
        lines.append(f"{name:4s} {B:3d} {ctx or 0:6d} {H:4d} {mtp} {topk:5d} {valid / (B * sq * topk):4.2f} | {plan(B, sq, H, topk, 0):2d} | "
                     f"{us16:8.1f} ({spread:4.1f}) {us8:8.1f} | {b16[1]:2d}: {b16[0]:8.1f}, {b8[1]:2d}: {b8[0]:8.1f} | "
                     f"{d16:8.1f} {d8:8.1f} | {us16 / d16:5.2f} {us8 / d8:5.2f} | {us_e:9.1f} {us_e / us16:6.2f} | "
                     f"{s16 / us16:5.3f} {s8 / us8:5.3f} | " + " ".join("%8.1f" % t for t in t16) + " | "
                     + " ".join("%8.1f" % t for t in t8))
        print(lines[-1], flush=True)
        del cache, deq, q, ind, out
        hpc.release_decode_workspaces()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
