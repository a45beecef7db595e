"""Development tool: hpc.mla_gather_ckv and hpc.mla_gather_ckv_fp8 timed per shape, beside their yardsticks in the same run:
  eager   the eager-torch gather the op replaces, on the same inputs: index tensors built per call + advanced indexing for the
          bf16 cache, plus the eager dequantisation c[d] = bf16(fp32(code[d]) * scale[d // 128]) for the FP8 cache - what a
          caller runs without the op.  The op must be faster in every row: the one pass/fail condition;
  bound   the HBM bound at 8 TB/s: 2 x 1,152 bytes per row for the bf16 cache, 656 + 1,152 for FP8.
The cache is a pool of 1 GiB of pages of 64 tokens, four times the Infinity Cache.  Every timed call reads through a page table
of its own, drawn at random from the pool and copied into block_ids in front of the timed window ("cold": the rows come from
HBM); the "warm" column repeats one table (19 - 38 MB of rows, served from the Infinity Cache).  Both agree with the eager
result bit for bit before anything is timed.  Times are device-event times around one replay of a hipGraph holding one call,
median of 20 after warm-up; a third column holds 16 calls in one graph and divides, which takes the cost of a replay itself
out of the figure; the eager baseline runs uncaptured, median of 5.
usage: python tools/tune_mla_gather.py [--out FILE] [--shapes 0,1,...]"""
import argparse
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import torch, hpc  # noqa: E402,E401
from hpc import _C  # noqa: E402

BF16, P = torch.bfloat16, 64
POOL_BYTES = 1 << 30
WORKSPACE = 32768
REPS = 16


def _mixed():
    rng = random.Random(3)
    lens = [rng.choice([128, 700, 2048, 5000, 12000, 32768]) for _ in range(64)]
    starts, cu, _ = hpc.mla_context_chunks(lens, WORKSPACE)[0]  # the first pass of a 32k-row workspace: 512 rows each at most
    return starts.tolist(), (cu[1:] - cu[:-1]).tolist()


def shapes():
    """(name, seq_starts, counts) per shape"""
    ms, mc = _mixed()
    return [("1 x 4096", [0], [4096]), ("4 x 4096", [0] * 4, [4096] * 4), ("1 x 16384", [0], [16384]),
            ("64 mixed 128..32k in 32k rows", ms, mc)]


def eager_gather(cache, bid, starts, counts, fp8):
    """the gather in eager torch from host lengths, as a caller writes it today"""
    dev = cache.device
    c = torch.tensor(counts, device=dev)
    req = torch.repeat_interleave(torch.arange(len(counts), device=dev), c)
    first = torch.cumsum(c, 0) - c
    pos = torch.tensor(starts, device=dev)[req] + (torch.arange(int(sum(counts)), device=dev) - first[req])
    rows = cache[bid[req, pos // P].long(), pos % P]
    if not fp8:
        return rows
    codes = rows[:, :512].contiguous().view(torch.float8_e4m3fn).float().view(-1, 4, 128)
    scales = rows[:, 512:528].contiguous().view(torch.float32)
    lat = (codes * scales[:, :, None]).to(BF16).view(-1, 512)
    return torch.cat([lat, rows[:, 528:].contiguous().view(BF16)], -1)


def _median_us(run, before, iters):
    ts = []
    for i in range(iters):
        before(i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def rows_for(fp8, a, dev):
    row = 656 if fp8 else 576
    nblocks = POOL_BYTES // (P * row * (1 if fp8 else 2))
    if fp8:  # finite codes (no 0x7f / 0xff) and scales of a writer's size
        cache = torch.randint(0, 0x7F, (nblocks, P, row), dtype=torch.uint8, device=dev)
        cache[:, :, 512:528] = torch.full((4,), 2.0 ** -7, dtype=torch.float32, device=dev).view(torch.uint8)
        cache[:, :, 528:] = torch.randn(nblocks, P, 64, device=dev).to(BF16).view(torch.uint8)
    else:
        cache = torch.randn(nblocks, P, row, device=dev).to(BF16)
    op = hpc.mla_gather_ckv_fp8 if fp8 else hpc.mla_gather_ckv
    lines, ok = [], True
    for idx, (name, starts, counts) in enumerate(shapes()):
        if a.shapes and idx not in a.shapes:
            continue
        B, T = len(counts), int(sum(counts))
        width = max(-(-(s + n) // P) for s, n in zip(starts, counts))
        g = torch.Generator().manual_seed(idx)
        tables = []
        for _ in range(21):  # one page table per timed call (and one to warm up on), each over pages of its own draw
            tables.append(torch.randperm(nblocks, generator=g)[: B * width].to(torch.int32).view(B, width).to(dev))
        bid = tables[0].clone()
        cu = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        st = torch.tensor(starts, dtype=torch.int32, device=dev)
        out = torch.empty(T, 576, dtype=BF16, device=dev)

        def call():
            return op(cache, bid, cu, seq_starts=st, output=out)

        call()
        want = eager_gather(cache, bid, starts, counts, fp8)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), want.view(torch.int16)), (name, "op != eager")
        del want
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        graph.replay()
        torch.cuda.synchronize()
        us_cold = _median_us(graph.replay, lambda i: bid.copy_(tables[1 + i]), 20)
        us_warm = _median_us(graph.replay, lambda i: None, 20)
        many = torch.cuda.CUDAGraph()  # the replay's own cost taken out: REPS calls in one graph, per call
        with torch.cuda.graph(many):
            for _ in range(REPS):
                call()
        many.replay()
        us_each = _median_us(many.replay, lambda i: None, 20) / REPS
        eager_gather(cache, bid, starts, counts, fp8)
        us_eager = _median_us(lambda: eager_gather(cache, bid, starts, counts, fp8), lambda i: bid.copy_(tables[1 + i]), 5)
        bound = T * ((656 if fp8 else 1152) + 1152) / 8e12 * 1e6
        faster = us_cold < us_eager
        ok = ok and faster
        lines.append(f"{'fp8 ' if fp8 else 'bf16'} {name:30s} B {B:2d} rows {T:5d} | {us_cold:7.1f} {us_warm:7.1f} {us_each:7.1f} | {us_eager:8.1f} "
                     f"{us_eager / us_cold:6.2f} | {bound:6.2f} {bound / us_cold:5.3f} {bound / us_each:5.3f}" + ("" if faster else "  SLOWER THAN EAGER"))
        print(lines[-1], flush=True)
        del tables, out
    del cache
    torch.cuda.empty_cache()
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="", help="indices into shapes() (default: all)")
    a = ap.parse_args()
    a.shapes = [int(v) for v in a.shapes.split(",") if v]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    lines = ["# mla_gather_ckv / mla_gather_ckv_fp8 on %d CUs (%s library), P = 64, pool of 1 GiB; us per call: one call in a "
             "replayed hipGraph, median of 20" % (_C.cu_count(dev), "development" if _C.DEV_BUILD else "product"),
             "# cache shape B rows | op us cold (a fresh page table per call)  warm (one table)  warm, 16 calls per replay, per call | "
             "eager us  eager/op (cold) | HBM bound us @8TB/s  frac (cold)  frac (16 per replay)"]
    print("\n".join(lines), flush=True)
    ok = True
    for fp8 in (False, True):
        more, good = rows_for(fp8, a, dev)
        lines += more
        ok = ok and good
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    if not ok:
        sys.exit("the gather is not faster than the eager statement in every row")


if __name__ == "__main__":
    main()
