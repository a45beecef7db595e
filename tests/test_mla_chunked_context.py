"""Chunked prefill over a cached context, end to end, as INTEGRATION.md writes the loop: hpc.mla_rope_norm_store_kv[_fp8] fills the
paged latent cache; the chunk attends causally to itself; hpc.mla_context_chunks cuts the context into passes of a bounded
workspace, and each pass runs hpc.mla_gather_ckv[_fp8] -> kv_b -> hpc.attention_prefill_mla_bf16(causal=False, cu_seqlens_k=...)
-> hpc.merge_attn_states in place.  The result is compared with tests/mla_prefill_ref.py::prefill_statement on the whole keys in
float64, under the bars tests/mla_prefill_needles.py states and tests/test_attention_prefill_mla.py::test_chunked_equals_whole
uses for chunked-and-merged against whole (TAU_NEEDLE on out, LSE_BAR_NEEDLE on lse).  No new tolerance.

Inputs: the builders of mla_prefill_needles do not fit - they plant k_nope / v directly, and here both come out of kv_b applied
to gathered latent rows.  So the inputs are random, and the statement is evaluated on the identical bf16 operands: kv_b is a
torch bf16 matmul with a fixed random weight that has one entry +-1 or +-1/2 per output column, so that every product is exact
in bf16 and the sum has one term - the GPU matmul of a pass and the CPU one of the statement give the same bits whatever the
row count (asserted).  The statement's latent rows never pass through the gather: the new tokens' and, for the bf16 cache, the
context's are the writer's out_ckv; for the FP8 cache the context's are mla_fp8_ref.dequantise of the cache, addressed on the
CPU."""
import functools

import pytest
import torch

import mla_gather_ref as gr
import mla_prefill_needles as mn
import mla_prefill_ref as ref
import mla_store_ref as ms
from utils import attn_close, attn_rel_err

BF16 = torch.bfloat16
CONTEXT, CHUNK = [0, 200, 700], [64, 33, 128]
H, P, WORKSPACE = 16, 64, 384


@functools.lru_cache(maxsize=None)
def _inputs():
    g = torch.Generator().manual_seed(29)
    total = [c + n for c, n in zip(CONTEXT, CHUNK)]
    rows, tq = sum(total), sum(CHUNK)
    kv_a = torch.randn(rows, 576, generator=g).to(BF16)
    norm_w = 1 + 0.1 * torch.randn(512, generator=g)
    q = (0.3 * torch.randn(tq, H, 192, generator=g)).to(BF16)
    # kv_b: one latent column per output column, times +-1 or +-1/2
    cols = H * 256
    pick = torch.randint(0, 512, (cols,), generator=g)
    coef = (torch.randint(0, 2, (cols,), generator=g) * 2 - 1) * torch.tensor([1.0, 0.5])[torch.randint(0, 2, (cols,), generator=g)]
    w_kvb = torch.zeros(512, cols)
    w_kvb[pick, torch.arange(cols)] = coef
    pages = [-(-t // P) for t in total]
    nblocks = sum(pages) + 2
    perm, o = torch.randperm(nblocks, generator=g).tolist(), 0
    bid = torch.full((3, max(pages) + 1), -1, dtype=torch.int32)
    for b, n in enumerate(pages):
        bid[b, :n] = torch.tensor(perm[o: o + n], dtype=torch.int32)
        o += n
    cum = lambda xs: torch.tensor([0] + torch.tensor(xs).cumsum(0).tolist(), dtype=torch.int32)  # noqa: E731
    return dict(kv_a=kv_a, norm_w=norm_w, q=q, w_kvb=w_kvb.to(BF16), bid=bid, nblocks=nblocks, total=total,
                cu_all=cum(total), cu_q=cum(CHUNK), seqlen=torch.tensor(total, dtype=torch.int32))


def _kv_b(lat, w):
    """[n, 576] latent rows -> (k_nope, v) views of the [n, H, 256] projection"""
    kv = (lat[:, :512] @ w).view(lat.shape[0], H, 256)
    return kv[..., :128], kv[..., 128:]


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_chunk_loop_equals_the_statement_on_the_whole_keys(fp8):
    import hpc

    x = _inputs()
    dev = "cuda"
    store, gather = ((hpc.mla_rope_norm_store_kv_fp8, hpc.mla_gather_ckv_fp8) if fp8 else
                     (hpc.mla_rope_norm_store_kv, hpc.mla_gather_ckv))
    cache = torch.zeros(x["nblocks"], P, 656 if fp8 else 576, dtype=torch.uint8 if fp8 else BF16, device=dev)
    rows = sum(x["total"])
    out_ckv = torch.empty(rows, 576, dtype=BF16, device=dev)
    bid, cu_all = x["bid"].to(dev), x["cu_all"].tolist()
    store(cache, x["kv_a"].to(dev), ms.cos_sin_table(1024).to(dev), x["norm_w"].to(dev), x["seqlen"].to(dev),
          x["cu_all"].to(dev), bid, out_ckv=out_ckv)
    q, w, cu_q = x["q"].to(dev), x["w_kvb"].to(dev), x["cu_q"].to(dev)
    max_q = max(CHUNK)

    # the chunk's own pass: causal, over the new tokens' latent rows as the writer returned them
    lat_new = torch.cat([out_ckv[cu_all[b] + CONTEXT[b]: cu_all[b + 1]] for b in range(3)])
    kn, v = _kv_b(lat_new, w)
    out, lse = hpc.attention_prefill_mla_bf16(q, kn, lat_new[:, 512:], v, cu_q, max_q, ref.SCALE, return_lse=True)
    # the context, in passes through a workspace of WORKSPACE rows
    plan = hpc.mla_context_chunks(CONTEXT, WORKSPACE)
    assert len(plan) == 6
    ws = torch.empty(WORKSPACE, 576, dtype=BF16, device=dev)
    for starts, cu_k, max_len in plan:
        n, cu_k = int(cu_k[-1]), cu_k.to(dev)
        assert gather(cache, bid, cu_k, seq_starts=starts.to(dev), output=ws) is ws
        kn, v = _kv_b(ws[:n], w)
        o2, l2 = hpc.attention_prefill_mla_bf16(q, kn, ws[:n, 512:], v, cu_q, max_q, ref.SCALE, cu_seqlens_k=cu_k,
                                                max_seqlens_k=max_len, causal=False, return_lse=True)
        hpc.merge_attn_states(out, lse, o2, l2, output=out, output_lse=lse)
    torch.cuda.synchronize()

    # the statement on the whole keys, from latent rows that never passed through the gather
    ckv = out_ckv.cpu()
    if fp8:
        cu_ctx = torch.tensor([0, CONTEXT[0], CONTEXT[0] + CONTEXT[1], sum(CONTEXT)], dtype=torch.int32)
        ctx = gr.gather_statement(cache.cpu(), x["bid"], cu_ctx, None,
                                  out_bits=torch.zeros(sum(CONTEXT), 576, dtype=torch.int16)).view(BF16)
        o = 0
        for b in range(3):
            ckv[cu_all[b]: cu_all[b] + CONTEXT[b]] = ctx[o: o + CONTEXT[b]]
            o += CONTEXT[b]
    kv = (ckv[:, :512].double() @ x["w_kvb"].double())
    assert torch.equal(kv, kv.to(BF16).double())  # kv_b is exact in bf16 ...
    kv = kv.to(BF16).view(rows, H, 256)
    assert torch.equal(_kv_b(ckv.to(dev), w)[1].cpu(), kv[..., 128:])  # ... and the GPU matmul gives those bits
    want, want_lse = ref.prefill_statement(x["q"], kv[..., :128], ckv[:, 512:], kv[..., 128:], x["cu_q"], x["cu_all"], ref.SCALE, True)
    want = want.to(BF16)
    w_out, w_lse = float(attn_rel_err(want, out.cpu()).max()), ref.lse_err(want_lse, lse)
    print(f"\n{'fp8' if fp8 else 'bf16'} cache, {len(plan)} passes: out worst {w_out:.5f} (tau {mn.TAU_NEEDLE}), "
          f"lse worst {w_lse:.3g} (bar {mn.LSE_BAR_NEEDLE})")
    assert attn_close(want, out.cpu(), mn.TAU_NEEDLE, label="chunk loop")
    assert w_lse <= mn.LSE_BAR_NEEDLE, (w_lse, mn.LSE_BAR_NEEDLE)
