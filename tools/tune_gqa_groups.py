"""Development tool: decode timing across GQA groups (1 / 2 / 4 / 8 / 16) at a fixed kv head count - the rows of
profiles/gqa_groups_decode.txt.  Same K / V bytes in every row of a block, so the times compare directly:
  * group 16 at num_seq_q 1 against group 8 at num_seq_q 2 (16 q rows per kv head both: the same tiles);
  * groups 1 and 2 at num_seq_q 1 against group 4;
  * sliced calls (group 16 at num_seq_q >= 3: every kv head's K / V requested once per slice) against group 8 at the same
    num_seq_q (one pass) - the ratio says how much of the second pass the L2 absorbs.
Device-event time of the op call (hipGraph replay of 10 back-to-back calls, median of 30; bench.timed), `rounds` passes over
all rows in turn so that neighbours in the table were measured alternately; HBM fraction = one pass over K / V + q + y bytes
at 8 TB/s.
usage: python tools/tune_gqa_groups.py [pkg=DIR] [hkv=8] [rounds=3] [cases=mixed,uniform8k] [P=64] ["k=v,k=v"]
pkg=DIR: import `hpc` from DIR (a build of another commit, for the yardstick rows; head ratios it refuses print as such).
A trailing "k=v" sets development registers (needs HPC_AMD_DEV=1), e.g. 28=1: bf16 on the first generation (16 x 3 rows: three blocks)."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
kw = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a and not a[0].isdigit())
regs = [a for a in sys.argv[1:] if a and a[0].isdigit()]
sys.path.insert(0, str(ROOT / "hpc-ops_amd")); sys.path.insert(0, str(ROOT))
import torch, bench
if "pkg" in kw:
    sys.path.insert(0, str(Path(kw["pkg"]).resolve()))
import hpc
from hpc import _C
dev = torch.device("cuda", 0)
HKV, ROUNDS, P = int(kw.get("hkv", 8)), int(kw.get("rounds", 3)), int(kw.get("P", 64))
B = 64
for cfg in regs:
    for k, v in (tuple(int(x) for x in kv.split("=")) for kv in cfg.split(",") if kv):
        assert _C.lib.hpc_dev_tuning_set(k, v) == 0
CASES = {"mixed": bench.c3_lens(), "uniform8k": torch.full((B,), 8192, dtype=torch.int32)}
cases = [(n, CASES[n]) for n in kw.get("cases", "mixed,uniform8k").split(",")]
# (block, kind, group, num_seq_q)
ROWS = [("16 rows", k, g, s) for k in ("fp8", "bf16") for g, s in ((8, 2), (16, 1))]
ROWS += [("one q token", k, g, 1) for k in ("fp8", "bf16") for g in (4, 2, 1)]
ROWS += [("sliced", "fp8", g, s) for s in (3, 4) for g in (8, 16)]
ROWS += [("sliced", "bf16", g, s) for s in (3, 4, 5) for g in (8, 16)]


def make(kind, g, sq, lens):
    w = dict(bench.C3 if kind == "fp8" else bench.C2, num_head_kv=HKV, num_head_q=HKV * g, num_seq_q=sq, block_size=P, batch=B)
    inp = bench.c3_inputs(dev, w, lens=lens) if kind == "fp8" else bench.c2_inputs(dev, lens, w)
    tm = hpc.get_attention_decode_task_workspace(B, int(lens.max()), HKV, 64)
    hpc.assign_attention_decode_task(inp["kv_lens"], tm, HKV, sq, True, 64)
    o = torch.empty(B * sq, HKV * g, 128, dtype=torch.bfloat16, device=dev)
    if kind == "fp8":
        fn = lambda: hpc.attention_decode_fp8(inp["q"], inp["k_cache"], inp["v_cache"], inp["block_ids"], inp["kv_lens"], inp["q_scale"],
                                              inp["k_scale"], inp["v_scale"], sq - 1, True,
                                              hpc.QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR, True, tm, None, o)
    else:
        fn = lambda: hpc.attention_decode_bf16(inp["q"], inp["k_cache"], inp["v_cache"], inp["block_ids"], inp["kv_lens"], sq - 1, True,
                                               True, tm, None, o)
    eb = 1 if kind == "fp8" else 2
    nbytes = int(lens.sum()) * HKV * 256 * eb + B * sq * HKV * g * 128 * (eb + 2)
    return fn, nbytes, (inp, tm, o)


print(f"# hpc {hpc.__version__} from {Path(hpc.__file__).parent}; {HKV} kv heads, pages of {P}, {ROUNDS} rounds, registers {regs or '-'}")
for cname, lens in cases:
    fns = []
    for block, kind, g, sq in ROWS:
        try:
            fn, nbytes, keep = make(kind, g, sq, lens)
            fn()
            torch.cuda.synchronize()
            fns.append((block, kind, g, sq, fn, nbytes, keep))
        except RuntimeError as e:
            print(f"{cname:<10} {block:<12} {kind:<4} {HKV}/{HKV * g:<4} sq {sq}: refused ({str(e).splitlines()[0][:70]})", flush=True)
    times = {i: [] for i in range(len(fns))}
    for _ in range(ROUNDS):
        for i, (_, _, _, _, fn, _, _) in enumerate(fns):
            times[i].append(bench.timed(fn, graph=True, iters=30, reps=10))
    for i, (block, kind, g, sq, _, nbytes, _) in enumerate(fns):
        ts = sorted(times[i])
        us = ts[len(ts) // 2]
        print(f"{cname:<10} {block:<12} {kind:<4} {HKV}/{HKV * g:<4} sq {sq}: {us:8.1f} us (min {ts[0]:.1f} max {ts[-1]:.1f})  "
              f"{nbytes / us / 1e3:7.0f} GB/s one pass = {nbytes / us / 1e3 / bench.HBM_PEAK_GBPS:.3f} of 8 TB/s", flush=True)
    del fns
    torch.cuda.empty_cache()
