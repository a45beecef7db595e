"""Development tool: hpc.mla_rope_norm_store_kv timed per shape beside two yardsticks in the same run:
  eager   the eager-torch statement of the same work on the same inputs (slice, square-mean, rsqrt, multiply, two rotations,
          the index computation, a scatter into the pages, the write into q_abs[..., 512:]) - what a caller runs without the op;
  stream  hpc.rope_norm_store_kv (the dense path's producer, 64 q + 8 kv heads of 128) at the same number of rows, and each
          op's fraction of 8 TB/s on its algorithmic bytes: rows x (1152 + 1152 + 2 x H x 128) plus the table reads here,
          rows x 80 x 256 x 2 there.
Times are device-event times of a replayed hipGraph holding one call, median of 20 replays after warm-up (bench.timed).  The op
and the eager statement must agree before their times are taken.

--cache fp8: hpc.mla_rope_norm_store_kv_fp8 (656-byte rows, csrc/mla_fp8_format.h) beside hpc.mla_rope_norm_store_kv in the same
run on the same shapes and inputs.  Before the times are taken the FP8 cells must be the project's 128-column quantisation
(hpc.blockwise_fp8_quant) of the bf16 cells, bit for bit, and out_q_pe equal.  Algorithmic bytes: the bf16 op's with the cache
write of 1,152 B per row replaced by 656 B.  The two ops are timed alternately, twice, and the lower median of each is kept.
usage: python tools/tune_mla_store.py [--cache bf16|fp8] [--out FILE] [--no-eager]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, bench, hpc  # noqa: E402,E401
from hpc import _C  # noqa: E402
from oracle import rope as orc  # noqa: E402

BF16, P, MAX_POS = torch.bfloat16, 64, 16384
# (name, requests, new tokens per request, context before them)
SHAPES = [("decode", 1, 1, 4000), ("decode", 64, 1, 4000), ("decode", 256, 1, 4000), ("mtp3", 64, 4, 4000),
          ("prefill", 2, 256, 0), ("prefill", 2, 512, 0), ("prefill", 2, 1024, 0), ("prefill", 4, 1024, 0), ("prefill", 4, 2048, 2048)]
HEADS = (16, 128)


def rot(t, cos, sin):  # interleaved pairing, fp32
    a, b = t[..., 0::2], t[..., 1::2]
    return torch.stack([a * cos - b * sin, b * cos + a * sin], -1).flatten(-2)


def main_fp8(dev, cs):
    lines = ["# mla_rope_norm_store_kv_fp8 beside mla_rope_norm_store_kv on %d CUs, pages of %d, interleaved pairing, kv_a = "
             "y[:, 1536:2112], q_pe = q[..., 128:], out_q_pe = q_abs[..., 512:]; us per call: one call in a replayed hipGraph, "
             "median of 20" % (_C.cu_count(dev), P),
             "# shape req new ctx H rows | bf16 us  fp8 us  fp8/bf16 | fp8: MB  frac of 8 TB/s"]
    for name, B, new, ctx in SHAPES:
        rows, total = B * new, ctx + new
        nb = (total + P - 1) // P
        bid = torch.randperm(B * nb + 8)[: B * nb].to(torch.int32).reshape(B, nb).to(dev)
        ns = torch.full((B,), total, dtype=torch.int32, device=dev)
        qi = torch.arange(0, rows + 1, new, dtype=torch.int32, device=dev)
        y = torch.randn(rows, 2112, device=dev).to(BF16)
        w = torch.randn(512, device=dev)
        kv_a = y[:, 1536:]
        r = torch.arange(rows, device=dev)
        req = r // new
        pos = ns[req].long() - (qi[req + 1].long() - r)
        page, slot = bid[req, pos // P].long(), pos % P
        for H in HEADS:
            q = (torch.randn(rows, H, 192, device=dev) / 24).to(BF16)
            q_pe = q[..., 128:]
            q_abs, q_abs8 = (torch.zeros(rows, H, 576, dtype=BF16, device=dev) for _ in range(2))
            ckv = torch.zeros(B * nb + 8, P, 576, dtype=BF16, device=dev)
            ckv8 = torch.zeros(B * nb + 8, P, 656, dtype=torch.uint8, device=dev)

            def op16():
                return hpc.mla_rope_norm_store_kv(ckv, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_q_pe=q_abs[..., 512:])

            def op8():
                return hpc.mla_rope_norm_store_kv_fp8(ckv8, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_q_pe=q_abs8[..., 512:])

            op16(), op8()
            torch.cuda.synchronize()
            cells16, cells8 = ckv[page, slot], ckv8[page, slot]
            codes, scales = hpc.blockwise_fp8_quant(cells16[:, :512].contiguous())
            assert torch.equal(cells8[:, :512], codes.view(torch.uint8)), (name, B, H, "codes")
            assert torch.equal(cells8[:, 512:528], scales.view(torch.uint8)), (name, B, H, "scales")
            assert torch.equal(cells8[:, 528:], cells16[:, 512:].contiguous().view(torch.uint8)), (name, B, H, "k_pe")
            assert torch.equal(q_abs8, q_abs) and bool(q_abs.float().abs().max() > 0), (name, B, H, "q_pe")
            # alternating, the lower of two medians each: at decode sizes both sit on the ~15 us floor of a one-call replay
            # and whichever is timed first in a process state takes outliers of several us
            t = [bench.timed(op, iters=20, graph=True) for op in (op16, op8, op16, op8)]
            us16, us8 = min(t[0], t[2]), min(t[1], t[3])
            mb = (rows * (1152 + 656 + 2 * H * 128) + rows * 256 + (2 * B + 1 + rows) * 4) / 1e6
            lines.append(f"{name:7s} {B:3d} {new:4d} {ctx:4d} {H:3d} {rows:5d} | {us16:7.1f} {us8:7.1f} {us8 / us16:5.2f} | "
                         f"{mb:7.2f} {mb / us8 / 8:5.3f}")
            print(lines[-1], flush=True)
            del q, q_abs, q_abs8, ckv, ckv8
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default="bf16", choices=("bf16", "fp8"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cs = orc.generate_cos_sin_cache(MAX_POS, 64).to(dev)
    if a.cache == "fp8":
        lines = main_fp8(dev, cs)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")
        return
    cs128 = orc.generate_cos_sin_cache(MAX_POS, 128).to(dev)
    lines = ["# mla_rope_norm_store_kv on %d CUs, pages of %d, interleaved pairing, kv_a = y[:, 1536:2112], q_pe = q[..., 128:], "
             "out_q_pe = q_abs[..., 512:]; us per call: one call in a replayed hipGraph, median of 20" % (_C.cu_count(dev), P),
             "# one kernel form: one wave per latent row and per 16 heads of a row",
             "# shape req new ctx H rows | op us | eager us  eager/op | MB  frac of 8 TB/s | rope_norm_store_kv (64+8 heads) us  MB  frac"]
    for name, B, new, ctx in SHAPES:
        rows, total = B * new, ctx + new
        nb = (total + P - 1) // P
        bid = torch.randperm(B * nb + 8)[: B * nb].to(torch.int32).reshape(B, nb).to(dev)
        ns = torch.full((B,), total, dtype=torch.int32, device=dev)
        qi = torch.arange(0, rows + 1, new, dtype=torch.int32, device=dev)
        qlens = torch.full((B,), new, dtype=torch.int64, device=dev)
        y = torch.randn(rows, 2112, device=dev).to(BF16)
        w = torch.randn(512, device=dev)
        kv_a = y[:, 1536:]
        # yardstick: the dense path's producer at the same rows
        qkv = torch.randn(rows, 80 * 128, device=dev).to(BF16)
        kc = torch.zeros(B * nb + 8, P, 8, 128, dtype=BF16, device=dev)
        vc = torch.zeros_like(kc)
        oq = torch.empty(rows, 64, 128, dtype=BF16, device=dev)
        us_r = bench.timed(lambda: hpc.rope_norm_store_kv(kc, vc, qkv, cs128, ns, qi, bid, new > 1, out_q=oq), iters=20, graph=True)
        mb_r = rows * 80 * 256 * 2 / 1e6
        del qkv, kc, vc, oq
        for H in HEADS:
            q = (torch.randn(rows, H, 192, device=dev) / 24).to(BF16)
            q_abs = torch.zeros(rows, H, 576, dtype=BF16, device=dev)
            q_abs_e = torch.zeros_like(q_abs)
            ckv = torch.zeros(B * nb + 8, P, 576, dtype=BF16, device=dev)
            ckv_e = torch.zeros_like(ckv)
            q_pe = q[..., 128:]

            def op():
                return hpc.mla_rope_norm_store_kv(ckv, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_q_pe=q_abs[..., 512:])

            def eager():
                r = torch.arange(rows, device=dev)
                req = torch.repeat_interleave(torch.arange(B, device=dev), qlens, output_size=rows)
                pos = ns[req].long() - (qi[req + 1].long() - r)
                x = kv_a.float()
                c = x[:, :512]
                lat = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + 1e-6) * w
                t = cs[pos]
                cos, sin = t[:, :32], t[:, 32:]
                ckv_e[bid[req, pos // P].long(), pos % P] = torch.cat([lat, rot(x[:, 512:], cos, sin)], -1).to(BF16)
                q_abs_e[..., 512:] = rot(q_pe.float(), cos[:, None], sin[:, None]).to(BF16)

            op()
            if not a.no_eager:  # the two must agree before their times mean anything
                eager()
                torch.cuda.synchronize()
                for got, want in ((ckv, ckv_e), (q_abs, q_abs_e)):
                    diff = (got.float() - want.float()).abs().max().item() / want.float().abs().max().item()
                    assert diff < 1e-2, (name, B, H, diff)
            us = bench.timed(op, iters=20, graph=True)
            us_e = float("nan") if a.no_eager else bench.timed(eager, iters=10, warm=2, graph=True)
            mb = (rows * (1152 + 1152 + 2 * H * 128) + rows * 256 + (2 * B + 1 + rows) * 4) / 1e6
            lines.append(f"{name:7s} {B:3d} {new:4d} {ctx:4d} {H:3d} {rows:5d} | {us:7.1f} | {us_e:8.1f} {us_e / us:6.1f} | "
                         f"{mb:7.2f} {mb / us / 8:5.3f} | {us_r:7.1f} {mb_r:7.2f} {mb_r / us_r / 8:5.3f}")
            print(lines[-1], flush=True)
            del q, q_abs, q_abs_e, ckv, ckv_e
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
