"""Development tool: hpc.attention_decode_mla_bf16 timed per shape at splits = 0 (the route's rule) and over a sweep of caller
split counts, beside three yardsticks in the same run:
  eager   the eager-torch statement on the same inputs (tests/mla_ref.py::mla_eager: page gather, two batched matmuls,
          softmax) - the only way to run this attention without the op;
  stream  the time's fraction of the latent-byte stream (tokens x 1,152 B read once) at 8 TB/s and at 6.05 TB/s, the rate
          measured for 1,152-byte rows gathered into 64-row LDS tiles from HBM;
  matrix  the time's fraction of the 2.5 PF bf16 matrix peak at 2 * rows * L * (576 + 512) flop.
Times are device-event times of a replayed hipGraph holding one call, median of 20 replays after warm-up (bench.timed).  A cache
smaller than the 256 MiB Infinity Cache (the single 64k request: 75 MB) is served from it, not from HBM.

--cache fp8: hpc.attention_decode_mla_fp8 beside hpc.attention_decode_mla_bf16 in the same run on the same shapes.  The FP8
cache is the project's 128-column quantisation of the same random latents (hpc.blockwise_fp8_quant, the 656-byte row of
csrc/mla_fp8_format.h); the bf16 op runs on its dequantisation, and the two outputs must be bit-equal before their times are
taken.  Per shape: both ops at splits = 0 and at their best caller split of the sweep, the ratio, and the FP8 time's fraction of
the 656-byte-per-token stream at 8 TB/s.
usage: python tools/tune_mla.py [--cache bf16|fp8] [--out FILE] [--splits 1,2,4,8,16,32,64] [--shapes 0,1,...] [--no-eager]"""
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


def inputs(B, ctx, H, sq, dev):
    """(lens, ckv bf16 [pool, P, 576], q, block_ids, lens on the device) of one shape"""
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
    return lens, ckv, q, bid.to(dev), lens.to(dev)


def to_fp8_cache(ckv):
    """(uint8 [pool, P, 656], its dequantisation bf16 [pool, P, 576]) of a bf16 latent cache, on its device"""
    pool = ckv.shape[0]
    codes, scales = hpc.blockwise_fp8_quant(ckv[..., :512].reshape(-1, 512).contiguous())
    cache = torch.empty(pool, P, 656, dtype=torch.uint8, device=ckv.device)
    cache[..., :512] = codes.view(torch.uint8).view(pool, P, 512)
    cache[..., 512:528] = scales.view(torch.uint8).view(pool, P, 16)
    cache[..., 528:] = ckv[..., 512:].contiguous().view(torch.uint8).view(pool, P, 128)
    deq = ckv.clone()
    for t0 in range(0, pool, 1024):  # in slabs: the fp32 intermediate of the whole pool would not fit beside it
        c = codes.view(pool, P, 4, 128)[t0: t0 + 1024].float() * scales.view(pool, P, 4, 1)[t0: t0 + 1024]
        deq[t0: t0 + 1024, :, :512] = c.to(BF16).view(-1, P, 512)
    return cache, deq


def main_fp8(a, sweep, dev):
    lines = ["# attention_decode_mla_fp8 beside attention_decode_mla_bf16 on %d CUs (%s library), pages of %d; us per call: one call "
             "in a replayed hipGraph, median of 20" % (_C.cu_count(dev), "development" if _C.DEV_BUILD else "product", P),
             "# the FP8 cache: 656 B per token (bf16: 1,152 B); the bf16 op reads the dequantised cache; outputs bit-equal",
             "# shape B ctx H mtp | splits(0) | bf16 us  fp8 us  fp8/bf16 | best split: bf16 us, fp8 us  fp8/bf16 | "
             "fp8 frac of the 656 B/token stream @8TB/s: splits 0, best | fp8 us at splits " + ",".join(map(str, sweep))]
    for idx, (name, B, ctx, H, mtp) in enumerate(SHAPES):
        if a.shapes and idx not in a.shapes:
            continue
        sq = mtp + 1
        lens, ckv, q, bid, lens_d = inputs(B, ctx, H, sq, dev)
        cache, deq = to_fp8_cache(ckv)
        del ckv
        out8 = torch.empty(B * sq, H, 512, dtype=BF16, device=dev)
        out16 = torch.empty_like(out8)

        def op8(splits):
            return lambda: hpc.attention_decode_mla_fp8(q, cache, bid, lens_d, SCALE, mtp=mtp, new_kv_included=True, output=out8,
                                                        splits=splits)

        def op16(splits):
            return lambda: hpc.attention_decode_mla_bf16(q, deq, bid, lens_d, SCALE, mtp=mtp, new_kv_included=True, output=out16,
                                                         splits=splits)

        op8(0)(), op16(0)()
        torch.cuda.synchronize()
        assert torch.equal(out8, out16) and bool(out8.float().abs().max() > 0), (name, H)  # before the times mean anything
        us8, us16 = bench.timed(op8(0), iters=20, graph=True), bench.timed(op16(0), iters=20, graph=True)
        t8 = [bench.timed(op8(s), iters=20, graph=True) for s in sweep]
        t16 = [bench.timed(op16(s), iters=20, graph=True) for s in sweep]
        b8, b16 = min(zip(t8, sweep)), min(zip(t16, sweep))
        t_stream = int(lens.sum()) * 656 / 8e12 * 1e6
        lines.append(f"{name:4s} {B:3d} {ctx or 0:6d} {H:4d} {mtp} | {plan(B, sq, H, 0):2d} | {us16:8.1f} {us8:8.1f} {us8 / us16:5.2f} | "
                     f"{b16[1]:2d}: {b16[0]:8.1f}, {b8[1]:2d}: {b8[0]:8.1f} {b8[0] / b16[0]:5.2f} | "
                     f"{t_stream / us8:5.3f} {t_stream / b8[0]:5.3f} | " + " ".join("%8.1f" % t for t in t8))
        print(lines[-1], flush=True)
        del cache, deq, q
        hpc.release_decode_workspaces()
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="bf16", choices=("bf16", "fp8"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--splits", default="1,2,4,8,16,32,64")
    ap.add_argument("--shapes", default="", help="indices into SHAPES (default: all)")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    sweep = [int(v) for v in a.splits.split(",") if v]
    a.shapes = [int(v) for v in a.shapes.split(",") if v]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if a.cache == "fp8":
        lines = main_fp8(a, sweep, dev)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")
        return
    lines = ["# attention_decode_mla_bf16 on %d CUs, pages of %d; us per call: one call in a replayed hipGraph, median of 20" %
             (_C.cu_count(dev), P),
             "# shape B ctx H mtp | splits(0) us | eager us  eager/op | stream frac @8TB/s @6.05TB/s | matrix frac @2.5PF | "
             "us at splits " + ",".join(map(str, sweep)) + " | best"]
    for idx, (name, B, ctx, H, mtp) in enumerate(SHAPES):
        if a.shapes and idx not in a.shapes:
            continue
        sq = mtp + 1
        lens, ckv, q, bid, lens_d = inputs(B, ctx, H, sq, dev)
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
