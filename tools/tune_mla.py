"""Development tool: hpc.attention_decode_mla_bf16 timed per shape at splits = 0 (the route's rule) and over a sweep of caller
split counts, beside three yardsticks in the same run:
  eager   the eager-torch statement on the same inputs (tests/mla_ref.py::mla_eager: page gather, two batched matmuls,
          softmax) - the only way to run this attention without the op;
  stream  the time's fraction of the latent-byte stream (tokens x 1,152 B read once) at 8 TB/s and at 6.05 TB/s, the rate
          measured for 1,152-byte rows gathered into 64-row LDS tiles from HBM;
  matrix  the time's fraction of the 2.5 PF bf16 matrix peak at 2 * rows * L * (576 + 512) flop.
Times are device-event times of a replayed hipGraph holding one call, median of 20 replays after warm-up (bench.timed).  A cache
smaller than the 256 MiB Infinity Cache (the single 64k request: 75 MB) is served from it, not from HBM.
usage: python tools/tune_mla.py [--out FILE] [--splits 1,2,4,8,16,32,64] [--no-eager]"""
import argparse
import ctypes
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, bench, hpc  # noqa: E402,E401
import mla_ref  # noqa: E402
from hpc import _C  # noqa: E402

BF16, P, SCALE = torch.bfloat16, 64, 192 ** -0.5
# (name, B, context (None: bench.py's 128 - 32k mix), H, mtp)
SHAPES = [("8k", 64, 8192, 16, 0), ("8k", 64, 8192, 128, 0), ("mix", 64, None, 16, 0), ("mix", 64, None, 128, 0),
          ("4k", 8, 4096, 128, 1), ("64k", 1, 65536, 16, 0)]


def plan(B, sq, H, splits):
    s, mx, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    rc = _C.lib.hpc_attention_decode_mla_plan(B, sq, H, splits, 0, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws))
    assert rc == 0, rc
    return s.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--splits", default="1,2,4,8,16,32,64")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    sweep = [int(v) for v in a.splits.split(",") if v]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = ["# attention_decode_mla_bf16 on %d CUs, pages of %d; us per call: one call in a replayed hipGraph, median of 20" %
             (_C.cu_count(dev), P),
             "# shape B ctx H mtp | splits(0) us | eager us  eager/op | stream frac @8TB/s @6.05TB/s | matrix frac @2.5PF | "
             "us at splits " + ",".join(map(str, sweep)) + " | best"]
    for name, B, ctx, H, mtp in SHAPES:
        sq = mtp + 1
        lens = torch.full((B,), ctx, dtype=torch.int32) if ctx else bench.c3_lens()[:B]
        nb = (lens + P - 1) // P
        total = int(nb.sum())
        pool = total + 8
        ckv = torch.randn(pool, P, 576, dtype=BF16, device=dev)
        q = (torch.randn(B * sq, H, 576, device=dev) / 24).to(BF16)
        perm = torch.randperm(pool)[:total].to(torch.int32)
        bid = torch.zeros(B, int(nb.max()), dtype=torch.int32)
        off = 0
        for i, n in enumerate(nb.tolist()):
            bid[i, :n] = perm[off: off + n]
            off += n
        bid, lens_d = bid.to(dev), lens.to(dev)
        out = torch.empty(B * sq, H, 512, dtype=BF16, device=dev)
        lens_l = lens.tolist()

        def op(splits):
            return lambda: hpc.attention_decode_mla_bf16(q, ckv, bid, lens_d, SCALE, mtp=mtp, new_kv_included=True, output=out,
                                                         splits=splits)

        def eager():
            return mla_ref.mla_eager(q, ckv, bid, lens_l, sq, SCALE)

        # the two must agree before their times mean anything
        op(0)()
        if not a.no_eager:
            want = eager()
            torch.cuda.synchronize()
            diff = (out.float() - want.float()).abs().max().item() / want.float().abs().max().item()
            assert diff < 3e-2, (name, H, diff)
        us0 = bench.timed(op(0), iters=20, graph=True)
        us_e = float("nan") if a.no_eager else bench.timed(eager, iters=5, warm=2, graph=True)
        tokens = int(lens.sum())
        t_stream8, t_stream6 = tokens * 1152 / 8e12 * 1e6, tokens * 1152 / 6.05e12 * 1e6
        t_mat = 2.0 * sq * H * tokens * (576 + 512) / 2.5e15 * 1e6
        times = [bench.timed(op(s), iters=20, graph=True) for s in sweep]
        best = min(zip(times, sweep))
        lines.append(f"{name:4s} {B:3d} {ctx or 0:6d} {H:4d} {mtp} | {plan(B, sq, H, 0):2d} {us0:8.1f} | {us_e:9.1f} {us_e / us0:6.2f} | "
                     f"{t_stream8 / us0:5.3f} {t_stream6 / us0:5.3f} | {t_mat / us0:5.3f} | "
                     + " ".join("%8.1f" % t for t in times) + f" | {best[1]}: {best[0]:.1f}")
        print(lines[-1], flush=True)
        del ckv, q
        hpc.release_decode_workspaces()
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
