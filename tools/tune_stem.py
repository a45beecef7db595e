"""Time the Stem mask kernels (hpc.stem) at a prompt shape: B = 1, a 64k-token prompt, 32 q / 4 kv heads, pages of 64,
both quant types.  Each op runs inside a captured hipGraph replayed `--iters` times; prints microseconds per call and
the fraction of the kernel's bound (HBM bytes / 8 TB/s, or FLOPs / 2.5 PFLOP/s when larger).  Report only.

    python tools/tune_stem.py [--tokens 65536] [--iters 50]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "hpc-ops_amd"))
sys.path.insert(0, str(ROOT))

import hpc  # noqa: E402
from oracle import attention as oattn  # noqa: E402

HBM, MFMA = 8.0e12, 2.5e15


def graph_us(fn, iters):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda")
    L, hq, hkv, P, D = args.tokens, 32, 4, 64, 128
    npg = (L + P - 1) // P
    kb = (L + 127) // 128
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(L, hq, D, device=dev, generator=g).to(torch.float8_e4m3fn)
    qscale = torch.rand(1, hq, kb * 128, device=dev, generator=g) * 0.1
    ql = torch.tensor([L], dtype=torch.int32, device=dev)
    cu = torch.tensor([0, L], dtype=torch.int32, device=dev)
    ids = torch.randperm(npg, device=dev, generator=g).to(torch.int32)[None]
    out = []
    for qt in (1, 0):
        kf = torch.randn(npg, P, hkv, D, device=dev, generator=g)
        vf = torch.randn(npg, P, hkv, D, device=dev, generator=g)
        if qt == 1:
            kc, vc = kf.to(torch.float8_e4m3fn), vf.to(torch.float8_e4m3fn)
            ks, vs = torch.tensor([0.7], device=dev), torch.tensor([1.3], device=dev)
        else:
            c8, ks = oattn.quant_paged_cache_pertoken(torch.cat([kf, torch.zeros(npg, P // 32, hkv, D, device=dev)], 1), P)
            kc = c8[:, :P]
            vc, vs = oattn.quant_paged_cache_perhead(vf, P)
        qtype = hpc.QuantType(qt)
        kflat, vbias = hpc.stem_oam_prep_paged_kv(kc, vc, ks, vs, ids, ql, quant_type=qtype)
        qflat = hpc.stem_oam_prep_varlen_q(q, qscale, ql, cu)
        lg = hpc.stem_oam_gemm(qflat, kflat, vbias, ql, ql)
        # the prep ops read the lengths' maximum on the host, which a graph cannot capture: time their C-ABI entries
        from hpc import _C
        vn = torch.empty(1, hkv, kb * 8, device=dev)
        es = 1 if ks.element_size() == 1 else 0
        kss = [st // 4 for st in ks.stride()[:3]] if qt == 0 and es else list(ks.stride()[:3]) if qt == 0 else [0, 0, 0]
        st = lambda: _C.stream_of(kc)  # noqa: E731

        def prep_kv():
            _C.check(_C.lib.hpc_stem_oam_prep_paged_kv_async(
                _C.ptr(kflat), _C.ptr(vbias), _C.ptr(vn), _C.ptr(kc), _C.ptr(vc), _C.ptr(ks), _C.ptr(vs), _C.ptr(ids),
                _C.ptr(ql), qt, 1, D, D, hkv, P, ids.size(1), 128, 16, kb, 0.3, kc.stride(0), kc.stride(1), kc.stride(2),
                vc.stride(0), vc.stride(1), vc.stride(2), *kss, st()), "prep_kv")

        def prep_q():
            _C.check(_C.lib.hpc_stem_oam_prep_varlen_q_async(
                _C.ptr(qflat), _C.ptr(q), _C.ptr(qscale), _C.ptr(ql), _C.ptr(cu), 1, hq, D, 128, 16, kb, q.stride(0),
                qscale.stride(0), qscale.stride(1), st()), "prep_q")

        nq = kb * (kb + 1) // 2  # causal (q block, kv block) pairs per head
        rows = [
            ("prep_kv", lambda: prep_kv(), 2 * L * hkv * D + kflat.numel() * 2, 0),
            ("prep_q", lambda: prep_q(), L * hq * D + qscale.numel() * 4 + qflat.numel() * 2, 0),
            ("oam_gemm", lambda: hpc.stem_oam_gemm(qflat, kflat, vbias, ql, ql), qflat.numel() * 2 + kflat.numel() * 2
             + lg.numel() * 2, 2 * nq * hq * 2048),
            ("tpd", lambda: hpc.stem_tpd(lg, ql, ql, ql), lg.numel() * 3, 0),
        ]
        for name, fn, nbytes, flops in rows:
            us = graph_us(fn, args.iters)
            bound = max(nbytes / HBM, flops / MFMA) * 1e6
            out.append({"quant_type": qt, "kernel": name, "us": round(us, 2), "bound_us": round(bound, 2),
                        "fraction_of_bound": round(bound / us, 3), "MB": round(nbytes / 1e6, 1)})
            print(json.dumps(out[-1]), flush=True)
    return out


if __name__ == "__main__":
    main()
