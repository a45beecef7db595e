"""Development tool: hpc.gemm_blockwise_fp8, the dense FP8 linear with 128-block scales, timed against two yardsticks in one run:
  (a)  hpc.group_gemm_blockwise_fp8 with ONE group on the same operands - the only way to run such a layer without the op; its
       activation scales go through hpc.reformat_x_scale outside the timed region,
  (b)  the weight-stream bound N * K bytes / 8 TB/s.
Every call is timed the way bench.py times its router row: a hipGraph of 20 back-to-back calls, median of 30 replays, each form
twice, alternating.  The 20 calls go round a ring of weight sets that together exceed the 256 MiB Infinity Cache (at least 2
sets), so the weights are read from HBM, not from the previous call's lines.  `wg` = workgroups launched: the op's from its
plan, (a)'s from the rule of csrc/group_gemm_route.h for one group (nan / 0 where (a) refuses the shape: it takes n % 128 == 0 only).  --splits LIST adds columns with the caller's split counts
(the A/B a change of the route's rule has to show).
usage: python tools/tune_linear.py [--out FILE] [--splits 1,2,4,8,16] [--shapes N,K;N,K] [--tokens 1,16,64,256]"""
import argparse
import ctypes
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT))
import torch, bench, hpc  # noqa: E402,E401
from hpc import _C  # noqa: E402
from hpc.group_gemm import aligned_size  # noqa: E402

F8, BF16, REPS, PEAK = torch.float8_e4m3fn, torch.bfloat16, 20, 8e12
SHAPES = [(2112, 7168), (24576, 1536), (7168, 16384), (7168, 2048), (4096, 4096)]
TOKENS = [1, 16, 64, 256]


def plan(m, n, k, splits):
    s, mx, cnt, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    rc = _C.lib.hpc_gemm_blockwise_fp8_plan(m, n, k, splits, 0, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws), ctypes.byref(cnt))
    assert rc == 0, rc
    return s.value, mx.value


def grouped_workgroups(m, n):
    """one group of m rows: ggemm_route() of csrc/group_gemm_route.h"""
    if m >= 16 and n % 256 == 0:
        return (m // 256 + 1) * (n // 256) + 16  # the 256 x 256 kernel's items
    if m > 20 and n % 128 == 0:
        return (m // 128 + 1) * (n // 128)
    return n // 64  # the streaming kernel, no split along K


def ring(fn, sets):
    state = {"i": 0}

    def call():
        s = sets[state["i"] % len(sets)]
        state["i"] += 1
        return fn(s)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--splits", default="")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--tokens", default="")
    a = ap.parse_args()
    extra = [int(v) for v in a.splits.split(",") if v]
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes.split(";") if s] or SHAPES
    tokens = [int(v) for v in a.tokens.split(",") if v] or TOKENS
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    cus = _C.cu_count(dev)
    lines = ["# gemm_blockwise_fp8 on %d CUs; us per call, hipGraph of %d calls round a ring of weight sets, median of 30 replays, "
             "each form twice" % (cus, REPS),
             "# N K M sets | splits wg | new us, again | (a) grouped GEMM, one group: us, again [wg] | (b) N*K/8TB/s us | "
             "new/(a) (best of two each) | new/(b)" + (" | new at splits " + ",".join(map(str, extra)) if extra else "")]
    for n, k in shapes:
        kb, nb = k // 128, (n + 127) // 128
        nset = max(2, min(REPS, -(-(512 << 20) // (n * k))))
        ws_pad = torch.zeros(nb, (kb + 3) // 4 * 4, device=dev)
        ws_pad[:, :kb] = torch.rand(nb, kb, device=dev) * 0.01 + 0.001
        sets = [dict(w=(torch.randn(n, k, device=dev) * 40).to(F8)) for _ in range(nset)]
        for m in tokens:
            x = (torch.randn(m, k, device=dev) * 40).to(F8)
            xs = torch.rand(m, kb, device=dev) + 0.5
            y = torch.empty(m, n, dtype=BF16, device=dev)
            ya = torch.empty(m, n, dtype=BF16, device=dev)
            tile_m = aligned_size(m)
            m_pad = -(-m // tile_m) * tile_m
            xs_rows = torch.zeros(m_pad, kb, device=dev)
            xs_rows[:m] = xs
            seqlens = torch.tensor([m], dtype=torch.int32, device=dev)
            cu_seqlens = torch.tensor([0, m], dtype=torch.int32, device=dev)
            xs_t = hpc.reformat_x_scale(xs_rows, seqlens, cu_seqlens, m)
            w_view = ws_pad[:, :kb]
            forms = {
                "new": lambda s: hpc.gemm_blockwise_fp8(x, xs, s["w"], w_view, output=y),
                "a": lambda s: hpc.group_gemm_blockwise_fp8(x, s["w"].unsqueeze(0), seqlens, cu_seqlens, xs_t, ws_pad.unsqueeze(0), m, ya),
            }
            for sp in extra:
                forms["s%d" % sp] = (lambda sp: lambda s: hpc.gemm_blockwise_fp8(x, xs, s["w"], w_view, output=y, splits=sp))(sp)
            # the two forms must agree before their times mean anything: same operands, same statement
            forms["new"](sets[0])
            try:
                forms["a"](sets[0])
                has_a = True
            except RuntimeError:  # the grouped GEMM takes n % 128 == 0 only: no yardstick (a) for 2112 rows
                has_a = False
            torch.cuda.synchronize()
            diff = (y.float() - ya.float()).abs().max().item() / max(ya.float().abs().max().item(), 1e-30) if has_a else 0.0
            assert diff < 2e-2, (n, k, m, diff)
            splits, mx = plan(m, n, k, 0)
            us = {}
            for name in ("new", "a", "a2", "new2"):
                us[name] = (bench.timed(ring(forms[name.rstrip("2")], sets), graph=True, reps=REPS)
                            if has_a or name.startswith("new") else float("nan"))
            more = ""
            if extra:
                more = " | " + " ".join(("%7.2f" % bench.timed(ring(forms["s%d" % sp], sets), graph=True, reps=REPS)) if sp <= mx
                                        else "      -" for sp in extra)
            bound = n * k / PEAK * 1e6
            best_new, best_a = min(us["new"], us["new2"]), min(us["a"], us["a2"])
            wg = -(-m // 64) * (n // 64) * splits
            lines.append(f"{n:6d} {k:6d} {m:4d} {nset:2d} | {splits:2d} {wg:5d} | {us['new']:7.2f} {us['new2']:7.2f} | "
                         f"{us['a']:7.2f} {us['a2']:7.2f} [{grouped_workgroups(m, n) if has_a else 0:4d}] | {bound:6.2f} | "
                         f"{best_new / best_a:5.2f} | {best_new / bound:5.2f}" + more)
            print(lines[-1], flush=True)
        del sets
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
