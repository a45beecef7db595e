"""Development tool: hpc.fuse_moe_mxfp4 (MXFP4 expert weights, W4A8) against hpc.fuse_moe_blockwise (blockwise FP8) on the same
routing in the same run, and against a pure stream of the MXFP4 weight bytes at 8 TB/s.

E experts / top-k / hidden H / intermediate I (default 64 / 8 / 4096 / 11008: 8.66 GB of FP8 expert weights, 4.60 GB of MXFP4),
T = 1, 16, 64, 256 tokens.  Every op is captured into a hipGraph with `output` given (one call per graph: the ops take a
millisecond) and replayed; the figure is the median of 20 replays, each op twice, alternating (a b b a).  The weights exceed the
256 MiB Infinity Cache many times over, so every replay reads them from HBM.  `active` = experts with at least one token; the
stream bound counts their weights only: active * 3 * H * I * (1/2 + 1/32) bytes / 8 TB/s.  There is no speed bar: every row is
reported, faster or not.
usage: python tools/bench_mxfp4.py [--out profiles/mxfp4_moe.txt] [--tokens 1,16,64,256] [--experts 64] [--topk 8] [--hidden 4096] [--inter 11008]"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd"))
import torch  # noqa: E402

import hpc  # noqa: E402

F8, BF16, PEAK = torch.float8_e4m3fn, torch.bfloat16, 8e12


def graph_of(step):
    """one call captured on a side stream after a warm-up there (as torch asks); no silent fall-back to eager timing"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    return g


def median_us(g, iters=20, warm=3):
    for _ in range(warm):
        g.replay()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        g.replay()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return ts[len(ts) // 2] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tokens", default="1,16,64,256")
    ap.add_argument("--experts", type=int, default=64)
    ap.add_argument("--topk", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=11008)
    a = ap.parse_args()
    E, topk, H, I = a.experts, a.topk, a.hidden, a.inter
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    u8 = dict(dtype=torch.uint8, device=dev)
    # MXFP4: any code, scale bytes 2^-8 ... 2^-6 (weights of magnitude 1e-2); FP8: normal data of the same magnitude, scale 1
    guw4, dw4 = torch.randint(0, 256, (E, 2 * I, H // 2), **u8), torch.randint(0, 256, (E, H, I // 2), **u8)
    gus4, ds4 = torch.randint(119, 122, (E, 2 * I, H // 32), **u8), torch.randint(119, 122, (E, H, I // 32), **u8)
    guw8, dw8 = torch.empty(E, 2 * I, H, dtype=F8, device=dev), torch.empty(E, H, I, dtype=F8, device=dev)
    for e in range(E):  # expert by expert: the fp32 draw of all of them at once would be 35 GB
        guw8[e] = (torch.randn(2 * I, H, device=dev) * 0.02).to(F8)
        dw8[e] = (torch.randn(H, I, device=dev) * 0.02).to(F8)
    pad4 = lambda v: (v + 3) // 4 * 4  # noqa: E731
    gus8 = torch.ones(E, 2 * I // 128, pad4(H // 128), device=dev)
    ds8 = torch.ones(E, H // 128, pad4(I // 128), device=dev)
    bytes4 = sum(t.numel() for t in (guw4, dw4, gus4, ds4))
    bytes8 = guw8.numel() + dw8.numel() + 4 * E * ((2 * I // 128) * (H // 128) + (H // 128) * (I // 128))
    lines = [f"# fuse_moe_mxfp4 vs fuse_moe_blockwise, E{E} top-{topk} H{H} I{I} on {torch.cuda.get_device_name(0)}; us per call, one call per "
             "hipGraph, median of 20 replays, each op twice (a b b a)",
             f"# expert weights: MXFP4 {bytes4 / 1e9:.3f} GB (codes + e8m0 scales), blockwise FP8 {bytes8 / 1e9:.3f} GB (codes + f32 128 x 128 "
             f"scales): byte ratio {bytes8 / bytes4:.3f}",
             "# T active | mxfp4 us, again | blockwise fp8 us, again | fp8 / mxfp4 (best of two each) | MXFP4 stream of the active "
             "experts at 8 TB/s us | mxfp4 / stream | share of 8 TB/s"]
    for T in [int(v) for v in a.tokens.split(",") if v]:
        x = (torch.randn(T, H, device=dev) * 40).to(F8)
        xs = torch.rand(T, H // 128, device=dev) * 0.01 + 0.005
        ids = torch.sort(torch.multinomial(torch.ones(T, E, device=dev), topk).to(torch.int32), dim=1)[0]
        sc = torch.rand(T, topk, device=dev)
        sc = sc / sc.sum(1, keepdim=True)
        active = int(torch.unique(ids).numel())
        y4, y8 = torch.empty(T, H, dtype=BF16, device=dev), torch.empty(T, H, dtype=BF16, device=dev)
        g4 = graph_of(lambda: hpc.fuse_moe_mxfp4(x, xs, guw4, gus4, dw4, ds4, ids, sc, 0, E, output=y4))
        g8 = graph_of(lambda: hpc.fuse_moe_blockwise(x, xs, guw8, gus8, dw8, ds8, ids, sc, 0, E, output=y8))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y4.float()).all()) and bool(torch.isfinite(y8.float()).all())
        a1, b1, b2, a2 = median_us(g4), median_us(g8), median_us(g8), median_us(g4)
        stream = active * 3 * H * I * (0.5 + 1 / 32) / PEAK * 1e6
        best4, best8 = min(a1, a2), min(b1, b2)
        lines.append(f"{T:4d} {active:3d} | {a1:8.1f} {a2:8.1f} | {b1:8.1f} {b2:8.1f} | {best8 / best4:5.2f} | {stream:7.1f} | "
                     f"{best4 / stream:5.2f} | {stream / best4:5.2f}")
        print(lines[-1], flush=True)
    print("\n".join(lines[:3]))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
