"""The four prefill ops on needle inputs (tests/prefill_needles.py) against the pinned oracles' arithmetic, under the
scale-aware bar tests/utils.py::attn_close at the taus that tests/test_prefill_bar.py derives on the CPU: GQA groups 1 ... 16,
pages of 16 / 32 / 64 tokens in NHD and HND strides, per-tensor and per-token K scales, ragged batches at the edges of
the tiling (prefill_needles.edge_batch), 20 000 cached tokens, a 4 000-token plain prefill, q as a view of a fused qkv
buffer, output= given and not, both row maps, block masks with cached prefixes that are not multiples of 128."""
import pytest
import torch

import prefill_needles as pn
from utils import attn_close, dev_set

F8 = torch.float8_e4m3fn
_CASES = {}


def _case(name, kind, k_per_token, P):
    """inputs and the oracle's answer, once per case: shared between layouts, output= variants and row maps"""
    key = (name, kind, k_per_token, P)
    if key not in _CASES:
        inp = pn.case_inputs(name, kind, k_per_token, P)
        _CASES[key] = (inp, pn.oracle(inp))
    return _CASES[key]


def _hnd(t):
    return t.view(torch.uint8).transpose(1, 2).contiguous().transpose(1, 2).view(t.dtype) if t.dtype == F8 else \
        t.transpose(1, 2).contiguous().transpose(1, 2)


def _fused_view(q, extra_heads=3):
    """q as the first Hq heads of a [total, Hq + extra, D] buffer whose other heads hold the largest finite value"""
    total, hq, d = q.shape
    buf = torch.full((total, hq + extra_heads, d), 448.0).to(q.dtype)
    buf[:, :hq] = q
    view = buf.cuda()[:, :hq]
    assert view.stride(0) > hq * d and view.stride(1) == d
    return view


def _run(inp, layout="nhd", fused_q=False, use_output=False, sparse=False, block_mask="inp"):
    import hpc

    kind = inp["kind"]
    q = _fused_view(inp["q"]) if fused_q else inp["q"].cuda()
    out = torch.full(inp["q"].shape, float("nan"), dtype=torch.bfloat16, device="cuda") if use_output else None
    cu, msq = inp["cu"].cuda(), inp["max_seqlens_q"]
    if kind == "bf16c":
        k, v = (_fused_view(inp["k"], 1), _fused_view(inp["v"], 2)) if fused_q else (inp["k"].cuda(), inp["v"].cuda())
        my = hpc.attention_prefill_bf16(q, k, v, inp["seq_q"].cuda(), cu, msq, output=out)
    else:
        P = inp["P"]
        kf, vf = inp["k_full"].cuda(), inp["v_full"].cuda()
        kc, vc = kf[:, :P], vf[:, :P]
        if layout == "hnd":
            kc, vc = _hnd(kc), _hnd(vc)
        bid, lens = inp["block_ids"].cuda(), inp["lens"].cuda()
        if kind == "bf16":
            my = hpc.attention_with_kvcache_prefill_bf16(q, kc, vc, cu, bid, lens, msq, output=out)
        else:
            kscale = kf[:, P:] if inp["k_per_token"] else inp["kscale"].cuda()
            qt = (hpc.QuantType.QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD if inp["k_per_token"]
                  else hpc.QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR)
            args = (q, kc, vc, inp["qscale"].cuda(), kscale, inp["vscale"].cuda(), cu, bid, lens, msq)
            if sparse:
                bm = inp["block_mask"] if isinstance(block_mask, str) else block_mask
                my = hpc.attention_with_kvcache_blocksparse_prefill_fp8(
                    *args, quant_type=qt, block_mask=None if bm is None else bm.to(torch.uint8).cuda(), output=out)
            else:
                my = hpc.attention_with_kvcache_prefill_fp8(*args, quant_type=qt, output=out)
    if use_output:
        assert my.data_ptr() == out.data_ptr()
    assert my.dtype == torch.bfloat16 and my.shape == inp["q"].shape
    return my.cpu()


# (case, kind, per-token K, page size, layout): every GQA group with every kind, every page size with both layouts
_DENSE = [
    ("edges_g1", "fp8", False, 16, "nhd"), ("edges_g2", "fp8", False, 32, "hnd"), ("edges_g4", "fp8", False, 64, "nhd"),
    ("edges_g8", "fp8", False, 32, "nhd"), ("edges_g16", "fp8", False, 64, "hnd"), ("edges_g16", "fp8", False, 16, "hnd"),
    ("long_20k", "fp8", False, 64, "nhd"), ("full_4k", "fp8", False, 64, "hnd"),
    ("edges_g1", "fp8", True, 32, "hnd"), ("edges_g2", "fp8", True, 64, "nhd"), ("edges_g4", "fp8", True, 32, "nhd"),
    ("edges_g8", "fp8", True, 64, "hnd"), ("edges_g16", "fp8", True, 32, "nhd"), ("long_20k", "fp8", True, 64, "hnd"),
    ("edges_g1", "bf16", False, 64, "hnd"), ("edges_g2", "bf16", False, 16, "nhd"), ("edges_g4", "bf16", False, 32, "hnd"),
    ("edges_g8", "bf16", False, 16, "hnd"), ("edges_g16", "bf16", False, 64, "nhd"), ("long_20k", "bf16", False, 64, "nhd"),
    ("full_4k", "bf16", False, 32, "nhd"),
    ("edges_g1", "bf16c", False, 1, "-"), ("edges_g2", "bf16c", False, 1, "-"), ("edges_g4", "bf16c", False, 1, "-"),
    ("edges_g8", "bf16c", False, 1, "-"), ("edges_g16", "bf16c", False, 1, "-"), ("full_4k", "bf16c", False, 1, "-"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind,k_per_token,P,layout", _DENSE)
def test_prefill_needles(case, kind, k_per_token, P, layout):
    """the dense ops: a plain call, and one with output= given and q (contiguous op: q, k and v) as views of fused buffers"""
    inp, ref = _case(case, kind, k_per_token, P)
    tau = pn.needle_tau(kind, k_per_token)
    plain = _run(inp, layout)
    assert attn_close(ref, plain, tau, label=f"{case} {kind} ktok={k_per_token} P={P} {layout}")
    fused = _run(inp, layout, fused_q=True, use_output=True)
    assert attn_close(ref, fused, tau, label=f"{case} {kind} ktok={k_per_token} P={P} {layout} fused q, output=")
    assert torch.equal(plain, fused)


_SPARSE = [("sparse_g4", False, 64, "nhd"), ("sparse_g4", True, 32, "hnd"), ("sparse_g8", False, 32, "hnd"),
           ("sparse_g8", True, 64, "nhd"), ("sparse_g16", False, 16, "nhd"), ("sparse_g16", True, 32, "hnd")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,k_per_token,P,layout", _SPARSE)
def test_blocksparse_prefill_needles(case, k_per_token, P, layout):
    """block masks at skip 0.5 / 0.9 over ragged requests with cached prefixes that are not multiples of 128, more mask
    columns than the longest request needs, needles in both 64-token halves of the columns; block_mask=None is the dense op"""
    inp, ref = _case(case, "fp8", k_per_token, P)
    tau = pn.needle_tau("fp8", k_per_token)
    assert inp["block_mask"].shape[-1] > (int(inp["lens"].max()) + 127) // 128
    my = _run(inp, layout, sparse=True)
    assert attn_close(ref, my, tau, label=f"{case} ktok={k_per_token} P={P} {layout}")
    assert torch.equal(my, _run(inp, layout, sparse=True, fused_q=True, use_output=True))
    dense = _run(inp, layout)
    assert torch.equal(dense, _run(inp, layout, sparse=True, block_mask=None))
    assert attn_close(pn.oracle(inp, block_mask=None), dense, tau, label=f"{case} dense")


@pytest.mark.gpu
def test_blocksparse_prefill_mask_column_limit():
    """a mask of 512 columns (64k tokens) is accepted, one of 513 refused before any launch"""
    inp = pn.needle_inputs([5, 130], [3, 0], 64, (1, 4), "fp8", seed=1)
    ref = pn.oracle(inp)
    full = torch.ones(2, 4, 2, 512, dtype=torch.bool)
    assert attn_close(ref, _run(inp, sparse=True, block_mask=full), pn.TAU_PREFILL_NEEDLE_FP8)
    with pytest.raises(RuntimeError):
        _run(inp, sparse=True, block_mask=torch.ones(2, 4, 2, 513, dtype=torch.bool))


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("row_map", [1, 2])
@pytest.mark.parametrize("case,sparse,P", [("edges_g4", False, 64), ("edges_g8", False, 32), ("sparse_g4", True, 64),
                                           ("sparse_g8", True, 32)])
def test_prefill_fp8_row_maps(case, sparse, P, row_map):
    """development key 7 pins the workgroup's row map: 1 = head-major (the block-sparse default at G <= 8), 2 =
    position-major (the dense default); each op is run on the map it does not ship with, too"""
    inp, ref = _case(case, "fp8", False, P)
    dev_set(7, row_map)
    try:
        my = _run(inp, sparse=sparse)
    finally:
        dev_set(7, 0)
    assert attn_close(ref, my, pn.TAU_PREFILL_NEEDLE_FP8, label=f"{case} row map {row_map}")
