"""Development tool: hpc.attention_prefill_mla_bf16 and hpc.merge_attn_states timed per shape, beside their yardsticks in the
same run:
  eager   the eager-torch statement on the same inputs (tests/mla_prefill_ref.py::prefill_eager: the 192-wide k assembled by a
          concat, then scaled_dot_product_attention; the float32 statement where that cannot express the mask) - what a caller
          runs without the op.  The op must be faster in every row: the one pass/fail condition;
  dense   hpc.attention_prefill_bf16 at 128 / 128 on the same tokens and heads (causal rows only; FLOP ratio 1.25), no bar;
  matrix  the achieved rate 2 * visible (row, key) pairs * (192 + 128) flop over the time, as a fraction of the 2.5 PF bf16 peak;
  merge   hpc.merge_attn_states against eager torch and against its HBM bound (two states read, one written, at 8 TB/s).
Inputs are the views a caller has: k_nope / v the halves of a [Tk, H, 256] buffer, k_pe columns 512.. of a [Tk, 576] buffer.
Times are device-event times, median of 20 replays of a hipGraph holding one call after warm-up (bench.timed); the eager
baselines run uncaptured, median of 5.
usage: python tools/tune_mla_prefill.py [--out FILE] [--shapes 0,1,...] [--no-eager]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, bench, hpc  # noqa: E402,E401
import mla_prefill_ref as ref  # noqa: E402
from hpc import _C  # noqa: E402

BF16, SCALE = torch.bfloat16, ref.SCALE
# (name, B, Sq per request, Lk per request (None: self attention, causal), H)
SHAPES = [("1x4k", 1, 4096, None, 16), ("1x4k", 1, 4096, None, 128), ("4x4k", 4, 4096, None, 16), ("4x4k", 4, 4096, None, 128),
          ("1x16k", 1, 16384, None, 16), ("1x16k", 1, 16384, None, 128), ("ctx 4k/16k", 1, 4096, 16384, 16),
          ("ctx 4k/16k", 1, 4096, 16384, 128)]
PEAK = 2.5e15


def attention_rows(a, dev):
    lines = ["# attention_prefill_mla_bf16 on %d CUs (%s library); us per call: one call in a replayed hipGraph, median of 20" %
             (_C.cu_count(dev), "development" if _C.DEV_BUILD else "product"),
             "# shape B Sq Lk H causal | op us | eager us  eager/op | dense 128/128 us  op/dense | PFLOP/s  frac of 2.5 PF"]
    ok = True
    for idx, (name, B, Sq, Lk, H) in enumerate(SHAPES):
        if a.shapes and idx not in a.shapes:
            continue
        causal = Lk is None
        lk = Sq if causal else Lk
        q = torch.randn(B * Sq, H, 192, device=dev).to(BF16)
        kv = torch.randn(B * lk, H, 256, device=dev).to(BF16)
        ckv = torch.randn(B * lk, 576, device=dev).to(BF16)
        kn, v, kp = kv[..., :128], kv[..., 128:], ckv[:, 512:]
        cu_q = (torch.arange(B + 1) * Sq).to(torch.int32)
        cu_k = (torch.arange(B + 1) * lk).to(torch.int32)
        cu_q_d, cu_k_d = cu_q.to(dev), cu_k.to(dev)
        out = torch.empty(B * Sq, H, 128, dtype=BF16, device=dev)
        lse = torch.empty(B * Sq, H, dtype=torch.float32, device=dev)
        extra = {} if causal else dict(cu_seqlens_k=cu_k_d, max_seqlens_k=lk)

        def op():
            return hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu_q_d, Sq, SCALE, causal=causal, output=out, output_lse=lse, **extra)

        def eager():
            return ref.prefill_eager(q, kn, kp, v, cu_q.tolist(), cu_k.tolist(), SCALE, causal)

        op()
        us_e = float("nan")
        if not a.no_eager:
            try:  # the two must agree before their times mean anything
                want = eager()
                torch.cuda.synchronize()
                diff = (out.float() - want.float()).abs().max().item() / want.float().abs().max().item()
                assert diff < 3e-2, (name, H, diff)
                del want
                us_e = bench.timed(eager, iters=5, warm=1)
            except torch.cuda.OutOfMemoryError:
                us_e = float("inf")  # eager cannot run the shape at all
                torch.cuda.empty_cache()
        us = bench.timed(op, iters=20, graph=True)
        pairs = B * H * (Sq * (Sq + 1) // 2 if causal else Sq * lk)
        rate = 2.0 * pairs * 320 / (us * 1e-6)
        us_d = float("nan")
        if causal:  # the dense bf16 kernel at 128 / 128 on the same tokens and heads
            qd, kd, vd = q[..., :128].contiguous(), kn.contiguous(), v.contiguous()
            seqlens = torch.full((B,), Sq, dtype=torch.int32, device=dev)
            outd = torch.empty_like(out)
            us_d = bench.timed(lambda: hpc.attention_prefill_bf16(qd, kd, vd, seqlens, cu_q_d, Sq, output=outd), iters=20, graph=True)
            del qd, kd, vd, outd
        faster = not (us_e <= us)
        ok = ok and (a.no_eager or faster)
        lines.append(f"{name:10s} {B} {Sq:5d} {lk:5d} {H:3d} {int(causal)} | {us:9.1f} | {us_e:10.1f} {us_e / us:6.2f} | "
                     f"{us_d:9.1f} {us / us_d:5.2f} | {rate / 1e15:6.3f} {rate / PEAK:5.3f}" + ("" if faster or a.no_eager else "  SLOWER THAN EAGER"))
        print(lines[-1], flush=True)
        del q, kv, ckv, out, lse
        torch.cuda.empty_cache()
    return lines, ok


def merge_rows(dev):
    lines = ["# merge_attn_states; us per call as above | eager us  eager/op | HBM bound us @8TB/s  frac"]
    for T, H, D in ((4096, 16, 128), (4096, 128, 128), (16384, 128, 128)):
        a = torch.randn(T, H, D, device=dev).to(BF16)
        b = torch.randn(T, H, D, device=dev).to(BF16)
        la, lb = torch.randn(T, H, device=dev) * 5, torch.randn(T, H, device=dev) * 5
        out, lse = torch.empty_like(a), torch.empty_like(la)
        us = bench.timed(lambda: hpc.merge_attn_states(a, la, b, lb, output=out, output_lse=lse), iters=20, graph=True)
        want, wl = ref.merge_eager(a, la, b, lb)
        assert (out.float() - want.float()).abs().max().item() < 5e-2 and (lse - wl).abs().max().item() < 1e-4
        us_e = bench.timed(lambda: ref.merge_eager(a, la, b, lb), iters=5, warm=1)
        bound = (3 * T * H * D * 2 + 3 * T * H * 4) / 8e12 * 1e6
        lines.append(f"merge T {T:5d} H {H:3d} D {D} | {us:8.1f} | {us_e:9.1f} {us_e / us:6.2f} | {bound:7.1f} {bound / us:5.3f}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="", help="indices into SHAPES (default: all)")
    ap.add_argument("--no-eager", action="store_true")
    a = ap.parse_args()
    a.shapes = [int(v) for v in a.shapes.split(",") if v]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines, ok = attention_rows(a, dev)
    lines += merge_rows(dev)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    if not ok:
        sys.exit("attention_prefill_mla_bf16 is not faster than the eager statement in every row")


if __name__ == "__main__":
    main()
