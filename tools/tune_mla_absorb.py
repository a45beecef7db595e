"""Development tool: hpc.mla_absorb_q and hpc.mla_unabsorb_o (bf16 and quant=True) timed per shape, beside the eager lines they
replace, on the same inputs in the same run and captured the same way:
  absorb_q      torch.bmm(q[..., :128].transpose(0, 1), w_uk, out=<head-major view of q_abs[..., :512]>)
  unabsorb_o    torch.bmm(o_lat.transpose(0, 1), w_uv^T) + the copy to [T, H * 128]; for quant=True + hpc.blockwise_fp8_quant
The weights are the two halves of one [H, 256, 512] tensor, q the view [..., :128] of [T, H, 192], the absorb output the view
[..., :512] of [T, H, 576].  Both sides agree (allclose at bf16 resolution) before anything is timed.  Times are device-event
times around one replay of a hipGraph holding one call, median of 20 after warm-up; each side is timed three times per row and
the run's own spread is (max - min) of those medians.  A second column holds 16 calls per replay, divided: the replay's own cost
taken out.  Pass/fail, rows with T <= 256: the op's SLOWEST median is below the yardstick's FASTEST one.  T = 1024 is reported
only.  bound: the bytes moved once (operands in, result out) at 8 TB/s.
usage: python tools/tune_mla_absorb.py [--out FILE] [--tokens 1,16,...] [--heads 16,128]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, hpc  # noqa: E402,E401
from hpc import _C  # noqa: E402

BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
REPS = 16


def _median_us(run, iters=20):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def _graph(call, reps=1):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            call()
    g.replay()
    torch.cuda.synchronize()
    return g


def _time(call):
    """(three medians of one call per replay, per-call median of 16 calls per replay)"""
    one, many = _graph(call), _graph(call, REPS)
    singles = [_median_us(one.replay) for _ in range(3)]
    return singles, _median_us(many.replay) / REPS


def row(T, H, dev):
    g = torch.Generator().manual_seed(T * 1000 + H)
    w = (torch.randn(H, 256, 512, generator=g) * 0.05).to(BF16).to(dev)
    w_uk, w_uv = w[:, :128], w[:, 128:]
    q = torch.randn(T, H, 192, generator=g).to(BF16).to(dev)[..., :128]
    o_lat = torch.randn(T, H, 512, generator=g).to(BF16).to(dev)
    q_abs, q_abs_y = torch.zeros(T, H, 576, dtype=BF16, device=dev), torch.zeros(T, H, 576, dtype=BF16, device=dev)
    o, o_y = torch.empty(T, H * 128, dtype=BF16, device=dev), torch.empty(T, H * 128, dtype=BF16, device=dev)
    codes, codes_y = torch.empty(T, H * 128, dtype=F8, device=dev), torch.empty(T, H * 128, dtype=F8, device=dev)
    scale, scale_y = torch.empty(T, H, device=dev), torch.empty(T, H, device=dev)

    def y_unabsorb():
        o_y.view(T, H, 128).copy_(torch.bmm(o_lat.transpose(0, 1), w_uv.transpose(1, 2)).transpose(0, 1))

    def y_unabsorb_quant():
        y_unabsorb()
        hpc.blockwise_fp8_quant(o_y, codes_y, scale_y)

    pairs = [
        ("absorb_q", lambda: hpc.mla_absorb_q(q, w_uk, output=q_abs[..., :512]),
         lambda: torch.bmm(q.transpose(0, 1), w_uk, out=q_abs_y[..., :512].transpose(0, 1)),
         2 * (T * H * 128 + H * 128 * 512 + T * H * 512)),
        ("unabsorb_o", lambda: hpc.mla_unabsorb_o(o_lat, w_uv, output=o), y_unabsorb,
         2 * (T * H * 512 + H * 128 * 512 + T * H * 128)),
        ("unabsorb_o quant", lambda: hpc.mla_unabsorb_o(o_lat, w_uv, output=codes, quant=True, output_scale=scale), y_unabsorb_quant,
         2 * (T * H * 512 + H * 128 * 512) + T * H * 132),
    ]
    for _, op, yard, _ in pairs:
        op()
        yard()
    torch.cuda.synchronize()
    assert torch.allclose(q_abs.float(), q_abs_y.float(), rtol=2 ** -7, atol=1e-2), "absorb_q != bmm"
    assert torch.allclose(o.float(), o_y.float(), rtol=2 ** -7, atol=1e-2), "unabsorb_o != bmm"
    assert torch.allclose(scale, scale_y, rtol=2 ** -6, atol=1e-6), "unabsorb_o quant scale != bmm + blockwise_fp8_quant"
    lines, ok = [], True
    for name, op, yard, nbytes in pairs:
        a, a16 = _time(op)
        y, y16 = _time(yard)
        bound = nbytes / 8e12 * 1e6
        spread = max(max(a) - min(a), max(y) - min(y))
        faster = max(a) < min(y)
        verdict = "" if faster else ("  NOT FASTER THAN THE YARDSTICK" if T <= 256 else "  (slower; reported only)")
        ok = ok and (faster or T > 256)
        lines.append(f"{name:17s} T {T:4d} H {H:3d} | op {min(a):6.1f} {sorted(a)[1]:6.1f} {max(a):6.1f}  /16 {a16:6.2f} | "
                     f"eager {min(y):6.1f} {sorted(y)[1]:6.1f} {max(y):6.1f}  /16 {y16:6.2f} | spread {spread:4.1f} "
                     f"eager/op {sorted(y)[1] / sorted(a)[1]:5.2f}  /16 {y16 / a16:5.2f} | bound {bound:6.3f} frac/16 {bound / a16:5.3f}{verdict}")
        print(lines[-1], flush=True)
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="1,16,64,256,1024")
    ap.add_argument("--heads", default="16,128")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = ["# mla_absorb_q / mla_unabsorb_o on %d CUs (%s library); us per call, device events around one replay of a hipGraph "
             "holding one call, median of 20, three times: min median max" % (_C.cu_count(dev), "development" if _C.DEV_BUILD else "product"),
             "# op T H | op us x3, per call of 16 per replay | eager yardstick us x3, per call of 16 per replay | the run's spread us, "
             "eager/op (medians), (16 per replay) | HBM bound us @8TB/s, fraction of it reached (16 per replay)"]
    print("\n".join(lines), flush=True)
    ok = True
    for H in [int(v) for v in a.heads.split(",")]:
        for T in [int(v) for v in a.tokens.split(",")]:
            more, good = row(T, H, dev)
            lines += more
            ok = ok and good
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    if not ok:
        sys.exit("an op is not faster than its eager yardstick by more than the run's spread in every decode row")


if __name__ == "__main__":
    main()
