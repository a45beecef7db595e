"""hpc.attention_prefill_mla_sparse_bf16 / _fp8: the token-sparse MLA attention over a ragged prefill chunk, and the DSA prefill
chain it ends: hpc.mla_indexer_prep_fp8 -> hpc.mla_indexer_topk_prefill_fp8 -> this op.

The statement is tests/mla_sparse_ref.py on the expanded form (tests/mla_indexer_prefill_ref.py).
CPU: surface and fakes; refusals of the new C entry points.
GPU: on a uniform q_index (Sq = 1 .. 4) bit-identical to hpc.attention_decode_mla_sparse_* at the same splits on both caches, and
through the needle lists of tests/mla_sparse_needles.py within the needle bars of the statement; on the ragged case bit-identical
to that op on the expanded form; empty rows and rows of no request; the chain end to end against the statements; a chunk whose
rows all see no more than topk tokens against the dense causal statement tests/mla_ref.py; a captured graph of the fused indexer
plus the attention replayed after everything changed in place."""
import ctypes
import functools
from ctypes import c_float, c_int, c_int64, c_void_p

import pytest
import torch

import mla_fp8_ref as f8
import mla_indexer_prefill_ref as pr
import mla_indexer_ref as ir
import mla_needles as mn
import mla_ref
import mla_sparse_needles as sn
from utils import attn_close, attn_rel_err

UNSUPPORTED, INVALID = -1, -2
OPS = ("bf16", "fp8")
DIM, DIM_V = 576, 512
C_BAR = 1024  # the logits bar of tests/test_mla_indexer.py


# ---- CPU: surface, fakes, refusals -------------------------------------------------------------------------------------------------
def test_surface():
    import hpc

    for name in ("attention_prefill_mla_sparse_bf16", "attention_prefill_mla_sparse_fp8"):
        assert name in hpc.__all__ and callable(getattr(hpc, name)), name
        assert hasattr(torch.ops.hpc_mla, name), name
    doc = hpc.attention_prefill_mla_sparse_bf16.__doc__
    for word in ("q_index[b] <= r", "num_seqlen_per_req[b] - (q_index[b + 1] - r)", "expanded form", "empty row", "lse = -inf",
                 "mla_unabsorb_o", "merge_attn_states", "bit-identical", "hipGraph", "H % 16 == 0", "{16, 32, 64, 128}", "splits"):
        assert word in doc, word
    doc = hpc.attention_prefill_mla_sparse_fp8.__doc__
    for word in ("656", "torch.uint8", "c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] )", "attention_decode_mla_sparse_fp8"):
        assert word in doc, word


@pytest.mark.parametrize("kind", OPS)
def test_fakes(kind):
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    fn = getattr(hpc, "attention_prefill_mla_sparse_" + kind)
    with FakeTensorMode():
        q = torch.empty(50, 32, DIM, dtype=torch.bfloat16, device="cuda")
        ckv = (torch.empty(9, 64, 656, dtype=torch.uint8, device="cuda") if kind == "fp8"
               else torch.empty(9, 64, DIM, dtype=torch.bfloat16, device="cuda"))
        bid = torch.empty(3, 5, dtype=torch.int32, device="cuda")
        lens = torch.empty(3, dtype=torch.int32, device="cuda")
        qi = torch.empty(4, dtype=torch.int32, device="cuda")
        idx = torch.empty(50, 100, dtype=torch.int32, device="cuda")
        out = fn(q, ckv, bid, lens, qi, idx, 0.1)
        assert (out.shape, out.dtype, out.device.type) == ((50, 32, DIM_V), torch.bfloat16, "cuda")
        out, lse = fn(q, ckv, bid, lens, qi, idx, 0.1, return_lse=True)
        assert (lse.shape, lse.dtype) == ((50, 32), torch.float32)
        o, l = torch.empty_like(out), torch.empty_like(lse)
        got = fn(q, ckv, bid, lens, qi, idx, 0.1, output=o, output_lse=l)
        assert got[0] is o and got[1] is l


@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def _ip(v):
    return ctypes.cast(c_void_p(v), ctypes.POINTER(c_int)) if v else None


def _vp(v):
    return c_void_p(v) if v else None


def call_attn(lib, kind, *, out=4096, lse=4096, q=4096, ckv=4096, bid=4096, lens=4096, qi=4096, idx=4096, T=40, req=2, H=64, topk=64,
              P=64, max_blocks=4, num_blocks=8, block_stride=None, token_stride=None, splits=1, ws=4096, ws_bytes=1 << 40):
    """hpc_attention_prefill_mla_sparse_{bf16,fp8}_async with pointers that are never dereferenced on the host"""
    row = 656 if kind == "fp8" else DIM
    ts = row if token_stride is None else token_stride
    bs = P * ts if block_stride is None else block_stride
    fn = getattr(lib, f"hpc_attention_prefill_mla_sparse_{kind}_async")
    return fn(_vp(out), ctypes.cast(c_void_p(lse), ctypes.POINTER(c_float)) if lse else None, _vp(q), _vp(ckv), _ip(bid), _ip(lens),
              _ip(qi), _ip(idx), T, req, H, topk, P, max_blocks, num_blocks, c_int64(bs), c_int64(ts), c_float(0.1), splits, _vp(ws),
              c_int64(ws_bytes), None)


@pytest.mark.parametrize("kind", OPS)
@pytest.mark.parametrize("kwargs,code", [
    (dict(qi=0), INVALID), (dict(req=-1), INVALID), (dict(T=-1), INVALID), (dict(out=0), INVALID), (dict(q=0), INVALID),
    (dict(idx=0), INVALID), (dict(lens=0), INVALID), (dict(bid=0), INVALID), (dict(topk=0), INVALID), (dict(num_blocks=-1), INVALID),
    (dict(splits=-1), INVALID), (dict(splits=65), INVALID), (dict(max_blocks=0), INVALID), (dict(H=24), UNSUPPORTED),
    (dict(H=144), UNSUPPORTED), (dict(topk=65537), UNSUPPORTED), (dict(P=48), UNSUPPORTED), (dict(max_blocks=1 << 26), UNSUPPORTED),
    (dict(q=4096 + 8), UNSUPPORTED), (dict(idx=4096 + 2), UNSUPPORTED), (dict(topk=256, splits=3, ws=0), INVALID),
    (dict(topk=256, splits=3, ws_bytes=100), INVALID), (dict(T=0), 0), (dict(req=0), 0), (dict(T=0, req=0, max_blocks=0), 0)])
def test_cabi_refuses_on_the_host(lib, kind, kwargs, code):
    """every refusal is the decode launcher's, made before any device call (the pointers point nowhere); a chunk without rows or
    without requests is accepted and launches nothing"""
    assert call_attn(lib, kind, **kwargs) == code, kwargs


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _caches(orig, seed):
    """(inputs whose ckv is the FP8 cache's dequantisation, {kind: the kind's cache on the GPU}): one statement for both kinds"""
    cache = f8.quantise(orig["ckv"], vary_seed=seed)
    inp = dict(orig, ckv=f8.dequantise(cache))
    return inp, {"bf16": inp["ckv"].cuda(), "fp8": cache.cuda()}


def _fill_scratch_with_nan():
    import hpc  # noqa: F401  (registers the ops)

    for ws in torch.ops.hpc_mla._workspaces():
        ws.fill_(0xFF)  # every float of it a NaN


def _prefill(kind, q, cache, block_ids, lens_total, q_index, indices, scale, splits=0, **kw):
    import hpc

    fn = getattr(hpc, "attention_prefill_mla_sparse_" + kind)
    return fn(q.cuda(), cache, block_ids.cuda(), lens_total.cuda(), q_index.cuda(), indices.cuda(), scale, return_lse=True,
              splits=splits, **kw)


def _decode(kind, q, cache, block_ids, lens_total, indices, scale, sq, splits):
    import hpc

    fn = getattr(hpc, "attention_decode_mla_sparse_" + kind)
    return fn(q.cuda(), cache, block_ids.cuda(), lens_total.cuda(), indices.cuda(), scale, mtp=sq - 1, new_kv_included=True,
              return_lse=True, splits=splits)


def _same_bits(a, b):
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


_UNIFORM = [(1, 16, 64, 64), (2, 64, 16, 128), (3, 32, 128, 65), (4, 128, 64, 320)]  # (Sq, H, P, topk)
_LENS = [0, 1, 63, 64, 65, 300, 700]


@functools.lru_cache(maxsize=None)
def _uniform_case(sq, H, P, topk):
    inp, caches = _caches(sn.sparse_needle_inputs(_LENS, sq, P, H, topk, seed=500 + H), 900 + H)
    return inp, caches, sn.statement(inp)


@pytest.mark.gpu
@pytest.mark.parametrize("sq,H,P,topk", _UNIFORM)
def test_uniform_q_index_is_the_decode_op_bit_for_bit_and_within_the_needle_bars(sq, H, P, topk):
    """q_index = [0, Sq, 2 Sq, ...]: every request has Sq rows, so the op IS the decode op at mtp = Sq - 1 - the same bits at
    splits 1, 3 and 0 on both caches; and the needle lists (needles on the edge slots, traps inside) go through the statement"""
    inp, caches, (ref, rlse) = _uniform_case(sq, H, P, topk)
    B = len(inp["lens_total"])
    q_index = torch.arange(B + 1, dtype=torch.int32) * sq
    for splits in (1, 3, 0):
        for kind in OPS:
            _fill_scratch_with_nan()
            got = _prefill(kind, inp["q"], caches[kind], inp["block_ids"], inp["lens_total"], q_index, inp["indices"], inp["scale"], splits)
            want = _decode(kind, inp["q"], caches[kind], inp["block_ids"], inp["lens_total"], inp["indices"], inp["scale"], sq, splits)
            assert _same_bits(got, want), (kind, splits)
            w_out, w_lse = float(attn_rel_err(ref, got[0].cpu(), 1).max()), sn.lse_err(rlse, got[1])
            print(f"{kind} Sq {sq} H {H} P {P} topk {topk} splits {splits}: out worst {w_out:.5f} (tau {mn.TAU_NEEDLE}), "
                  f"lse worst {w_lse:.3g} (bar {mn.LSE_BAR_NEEDLE})")
            assert attn_close(ref, got[0].cpu(), mn.TAU_NEEDLE, 1, label=f"{kind} splits {splits}")
            assert w_lse <= mn.LSE_BAR_NEEDLE, (kind, splits, w_lse)


@functools.lru_cache(maxsize=None)
def _ragged_case(H, P, topk):
    """the ragged case of tests/mla_indexer_prefill_ref.py over a latent cache: random q for every row of the chunk, one poisoned
    page id per request of more than one page, and lists of positions drawn from [-3, vis + 5) - invalid entries of every kind, duplicates - with rows
    of no request and two deliberately empty live rows (all -1; all at or past vis)"""
    lens_total, q_index, T = pr.chunk_of(pr.CASE_NEW, pr.CASE_CTX, pr.PAD_ROWS)
    base = mn.uniform_inputs((lens_total - 1).tolist(), 1, P, H, seed=77)
    assert torch.equal(base["lens_total"], lens_total)
    g = torch.Generator().manual_seed(78)
    block_ids = torch.cat([base["block_ids"], torch.full((len(lens_total), 1), -1, dtype=torch.int32)], 1)
    for b, nb in enumerate(base["nblocks"].tolist()):
        if nb > 1:  # a request of one page keeps it: its rows must see something
            block_ids[b, int(torch.randint(0, nb, (1,), generator=g))] = (1 << 20) if b % 2 else -7
    q = (torch.randn(T, H, DIM, generator=g) / DIM ** 0.5).bfloat16()
    bid, lens, _ = pr.expand(block_ids, lens_total, q_index, T)
    indices = torch.stack([torch.randint(-3, int(v) + 5, (topk,), generator=g) for v in lens.tolist()]).to(torch.int32)
    indices[40] = -1
    indices[41] = int(lens[41]) + torch.arange(topk, dtype=torch.int32)
    inp = dict(q=q, ckv=base["ckv"], block_ids=block_ids, lens_total=lens_total, q_index=q_index, T=T, scale=mn.SCALE)
    inp, caches = _caches(inp, 79)
    return inp, caches, indices, (bid, lens)


@pytest.mark.gpu
@pytest.mark.parametrize("H,P,topk", [(16, 16, 96), (64, 64, 200), (128, 64, 65)])
def test_the_ragged_case_is_the_decode_op_on_the_expanded_form(H, P, topk):
    """rows of nine requests, a tile of heads per row: out and lse have the bits of hpc.attention_decode_mla_sparse_* on T
    one-row requests; rows of no request and rows without a valid entry give out = 0 and lse = -inf; the statement within the
    bars of the dense uniform inputs"""
    inp, caches, indices, (bid, lens) = _ragged_case(H, P, topk)
    dead = [154, 155, 158, 159, 160, 40, 41]
    ref, rlse = pr.sparse_statement(inp["q"], inp["ckv"], inp, indices, inp["scale"])
    assert bool((ref[dead] == 0).all()) and bool((rlse[dead] == float("-inf")).all())
    # (a row that sees only a poisoned page is empty too: at pages of 64 about a third of the rows)
    assert int(torch.isfinite(rlse).all(-1).sum()) >= inp["T"] // 2
    for splits in (1, 3):
        for kind in OPS:
            _fill_scratch_with_nan()
            got = _prefill(kind, inp["q"], caches[kind], inp["block_ids"], inp["lens_total"], inp["q_index"], indices, inp["scale"], splits)
            want = _decode(kind, inp["q"], caches[kind], bid, lens, indices, inp["scale"], 1, splits)
            assert _same_bits(got, want), (kind, splits)
            out, lse = got[0].cpu(), got[1].cpu()
            assert bool((out[dead] == 0).all()) and bool((lse[dead] == float("-inf")).all())
            w_out, w_lse = float(attn_rel_err(ref.to(torch.bfloat16), out, 1).max()), sn.lse_err(rlse, lse)
            print(f"{kind} ragged H {H} P {P} topk {topk} splits {splits}: out worst {w_out:.5f} (tau {mn.TAU_UNIFORM}), "
                  f"lse worst {w_lse:.3g} (bar {mn.LSE_BAR_UNIFORM})")
            assert attn_close(ref.to(torch.bfloat16), out, mn.TAU_UNIFORM, 1, label=f"{kind} ragged splits {splits}")
            assert w_lse <= mn.LSE_BAR_UNIFORM, (kind, splits, w_lse)


@pytest.mark.gpu
def test_no_request_and_refusals():
    import hpc

    i32 = dict(dtype=torch.int32, device="cuda")
    ckv = torch.randn(3, 64, DIM, device="cuda").bfloat16()
    q = torch.randn(5, 16, DIM, device="cuda").bfloat16()
    idx = torch.zeros(5, 8, **i32)
    none = (torch.empty(0, 2, **i32), torch.empty(0, **i32), torch.zeros(1, **i32))
    out, lse = hpc.attention_prefill_mla_sparse_bf16(q, ckv, *none, idx, 0.1, return_lse=True)
    assert bool((out == 0).all()) and bool((lse == float("-inf")).all())
    one = (torch.zeros(1, 2, **i32), torch.full((1,), 5, **i32), torch.tensor([0, 5], **i32))
    assert hpc.attention_prefill_mla_sparse_bf16(q[:0], ckv, *one, idx[:0], 0.1).shape == (0, 16, DIM_V)
    with pytest.raises(RuntimeError, match="q_index"):
        hpc.attention_prefill_mla_sparse_bf16(q, ckv, one[0], one[1], one[2][:1], idx, 0.1)
    with pytest.raises(RuntimeError, match="indices"):
        hpc.attention_prefill_mla_sparse_bf16(q, ckv, *one, idx[:4], 0.1)
    with pytest.raises(RuntimeError, match="num_head"):
        hpc.attention_prefill_mla_sparse_bf16(q[:, :8].contiguous(), ckv, *one, idx, 0.1)
    with pytest.raises(RuntimeError, match="splits"):
        hpc.attention_prefill_mla_sparse_bf16(q, ckv, *one, idx, 0.1, splits=65)
    with pytest.raises(RuntimeError, match="ckv_cache dtype"):
        hpc.attention_prefill_mla_sparse_fp8(q, ckv, *one, idx, 0.1)


# ---- GPU: the chain end to end -----------------------------------------------------------------------------------------------------
def _chain_inputs(new, ctx, P, Hi, H, seed):
    """a chunk continuing cached prefixes: the index keys and latent rows of EVERY token (the prefix written as an earlier chunk),
    the chunk's index queries and attention queries"""
    g = torch.Generator().manual_seed(seed)
    lens_total, q_index, T = pr.chunk_of(new, ctx, 0)
    lat = mn.uniform_inputs((lens_total - 1).tolist(), 1, P, H, seed=seed)
    total = int(lens_total.sum())
    return dict(lens_total=lens_total, q_index=q_index, T=T, block_ids=lat["block_ids"], ckv=lat["ckv"], P=P, Hi=Hi, scale=mn.SCALE,
                all_index=torch.tensor([0] + lens_total.cumsum(0).tolist(), dtype=torch.int32), total=total,
                k_all=torch.randn(total, 128, generator=g).bfloat16(), q_idx=torch.randn(T, Hi, 128, generator=g).bfloat16(),
                head_w=torch.randn(T, Hi, generator=g), norm_w=1 + 0.1 * torch.randn(128, generator=g),
                norm_b=0.1 * torch.randn(128, generator=g), cos_sin=torch.cat([torch.cos(a := torch.rand(4096, 32, generator=g) * 6.283),
                                                                              torch.sin(a)], -1).contiguous(),
                q=(torch.randn(T, H, DIM, generator=g) / DIM ** 0.5).bfloat16())


def _run_chain(c, topk, kind="bf16", cache=None):
    """prep (every token's key as an earlier chunk, then the chunk with its queries) -> fused top-k -> sparse attention.
    Returns (q8, weights, k_cache, indices, out, lse) on the GPU."""
    import hpc

    bid, lens, qi = c["block_ids"].cuda(), c["lens_total"].cuda(), c["q_index"].cuda()
    k_cache = torch.zeros(c["ckv"].shape[0], c["P"] * 132, dtype=torch.uint8, device="cuda")
    nw, nb, cs = c["norm_w"].cuda(), c["norm_b"].cuda(), c["cos_sin"].cuda()
    hpc.mla_indexer_prep_fp8(k_cache, c["k_all"].cuda(), nw, nb, cs, lens, c["all_index"].cuda(), bid)
    rows = torch.cat([torch.arange(int(c["all_index"][b + 1]) - n, int(c["all_index"][b + 1])) for b, n in
                      enumerate((c["q_index"][1:] - c["q_index"][:-1]).tolist())])
    q8, weights = hpc.mla_indexer_prep_fp8(k_cache, c["k_all"][rows].cuda(), nw, nb, cs, lens, qi, bid, q=c["q_idx"].cuda(),
                                           head_weights=c["head_w"].cuda(), softmax_scale=128 ** -0.5)
    idx = hpc.mla_indexer_topk_prefill_fp8(q8, weights, k_cache, bid, lens, qi, topk)
    ckv = c["ckv"].cuda() if cache is None else cache
    out, lse = getattr(hpc, "attention_prefill_mla_sparse_" + kind)(c["q"].cuda(), ckv, bid, lens, qi, idx, c["scale"], return_lse=True)
    return q8, weights, k_cache, idx, out, lse


@pytest.mark.gpu
def test_end_to_end_prep_indexer_sparse_attention():
    """the chain on a chunk of three requests over cached prefixes of 0, 30 and 200 tokens.  The indexer's lists are the top-k
    statement's selection over logits that are within C_BAR * 2^-24 * A of the logits statement on what prep wrote (prep itself is
    pinned by tests/test_mla_indexer_prep.py); the attention on those lists is within the uniform bars of the sparse statement"""
    import hpc

    topk = 32
    c = _chain_inputs([5, 40, 17], [0, 30, 200], 64, 16, 16, seed=91)
    q8, weights, k_cache, idx, out, lse = _run_chain(c, topk)
    ind = dict(c, q=q8.cpu(), weights=weights.cpu(), k_cache=k_cache.cpu())
    want = pr.logits_statement(ind)
    logits = hpc.mla_indexer_logits_prefill_fp8(q8, weights, k_cache, c["block_ids"].cuda(), c["lens_total"].cuda(), c["q_index"].cuda(),
                                                output=torch.full(want.shape, float("nan"), device="cuda"))
    ratio = ir.worst_ratio(logits, want, pr.absolute_statement(ind))
    print(f"\nend to end: logits worst err / (2^-24 A) = {ratio:.3f} (bar {C_BAR})")
    assert ratio <= C_BAR
    assert torch.equal(idx.cpu(), pr.topk_statement(logits.cpu(), ind, topk))
    vis = pr.expand(c["block_ids"], c["lens_total"], c["q_index"], c["T"])[1]
    assert int((vis > topk).sum()) > 20 and int((vis <= topk).sum()) > 5 and bool(((idx >= 0).sum(1).cpu() == vis.clamp_max(topk)).all())
    ref, rlse = pr.sparse_statement(c["q"], c["ckv"], c, idx.cpu(), c["scale"])
    w_out, w_lse = float(attn_rel_err(ref.to(torch.bfloat16), out.cpu(), 1).max()), sn.lse_err(rlse, lse)
    print(f"end to end: out worst {w_out:.5f} (tau {mn.TAU_UNIFORM}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_UNIFORM})")
    assert attn_close(ref.to(torch.bfloat16), out.cpu(), mn.TAU_UNIFORM, 1, label="prefill chain")
    assert w_lse <= mn.LSE_BAR_UNIFORM


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
def test_a_chunk_that_sees_no_more_than_topk_is_the_dense_causal_attention(kind):
    """every row sees at most topk tokens: the lists are 0 .. vis - 1 and the chain gives the dense causal result - the
    statement tests/mla_ref.py on the expanded form"""
    topk = 256
    c = _chain_inputs([64, 3, 100], [0, 250, 156], 32, 32, 32, seed=92)
    c, caches = _caches(c, 93)
    _, _, _, idx, out, lse = _run_chain(c, topk, kind, caches[kind])
    bid, vis, _ = pr.expand(c["block_ids"], c["lens_total"], c["q_index"], c["T"])
    assert int(vis.max()) == topk and int(vis.min()) == 1
    ident = torch.arange(topk, dtype=torch.int32)[None, :].repeat(c["T"], 1)
    ident[ident >= vis[:, None]] = -1
    assert torch.equal(idx.cpu(), ident)
    ref, rlse = mla_ref.mla_statement(c["q"], c["ckv"], bid, vis, 1, c["scale"])
    w_out, w_lse = float(attn_rel_err(ref.to(torch.bfloat16), out.cpu(), 1).max()), sn.lse_err(rlse, lse)
    print(f"\n{kind} dense causal: out worst {w_out:.5f} (tau {mn.TAU_UNIFORM}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_UNIFORM})")
    assert attn_close(ref.to(torch.bfloat16), out.cpu(), mn.TAU_UNIFORM, 1, label=f"{kind} dense causal")
    assert w_lse <= mn.LSE_BAR_UNIFORM


@pytest.mark.gpu
def test_graph_replays_after_lengths_q_index_pages_cache_and_q_changed_in_place():
    """the fused indexer (three slabs) plus the attention (three pieces) captured once with outputs given; replayed after
    everything changed in place: the new chunk's result, bit for bit what the eager calls give, lists equal to the statement"""
    import hpc

    Hi, P, H, topk, T = 16, 16, 16, 40, 96
    a = pr.inputs(Hi, P, exact=True, new=[30, 1, 50], ctx=[100, 0, 7], pad_rows=15, seed=31)
    b = pr.inputs(Hi, P, exact=True, new=[2, 60, 34], ctx=[70, 90, 0], pad_rows=0, seed=32)
    assert a["T"] == T and b["T"] == T
    pool = max(a["k_cache"].shape[0], b["k_cache"].shape[0])
    cols = max(a["block_ids"].shape[1], b["block_ids"].shape[1])
    g = torch.Generator().manual_seed(5)

    def padded(c):  # the case's pool inside the graph's pool, its table inside the graph's table, a latent cache and q beside it
        cache = torch.full((pool, P * 132), 0x38, dtype=torch.uint8)
        cache[: c["k_cache"].shape[0]] = c["k_cache"]
        bid = torch.full((3, cols), -1, dtype=torch.int32)
        bid[:, : c["block_ids"].shape[1]] = c["block_ids"]
        return dict(c, k_cache=cache, block_ids=bid, ckv=torch.randn(pool, P, DIM, generator=g).bfloat16(),
                    qa=(torch.randn(T, H, DIM, generator=g) / DIM ** 0.5).bfloat16())

    cases = [padded(a), padded(b)]
    dev = dict(device="cuda")
    q = torch.zeros(T, Hi, 128, **dev).to(ir.F8)
    w = torch.zeros(T, Hi, **dev)
    cache = torch.zeros(pool, P * 132, dtype=torch.uint8, **dev)
    ckv = torch.zeros(pool, P, DIM, dtype=torch.bfloat16, **dev)
    qa = torch.zeros(T, H, DIM, dtype=torch.bfloat16, **dev)
    bid = torch.full((3, cols), -1, dtype=torch.int32, **dev)
    lens, qi = torch.zeros(3, dtype=torch.int32, **dev), torch.zeros(4, dtype=torch.int32, **dev)
    idx = torch.zeros(T, topk, dtype=torch.int32, **dev)
    out, lse = torch.zeros(T, H, DIM_V, dtype=torch.bfloat16, **dev), torch.zeros(T, H, **dev)

    def load(c):
        q.view(torch.uint8).copy_(c["q"].view(torch.uint8))
        w.copy_(c["weights"])
        cache.copy_(c["k_cache"])
        ckv.copy_(c["ckv"])
        qa.copy_(c["qa"])
        bid.copy_(c["block_ids"])
        lens.copy_(c["lens_total"])
        qi.copy_(c["q_index"])

    def step(idx, out, lse):
        hpc.mla_indexer_topk_prefill_fp8(q, w, cache, bid, lens, qi, topk, scratch_rows=40, output=idx)
        return hpc.attention_prefill_mla_sparse_bf16(qa, ckv, bid, lens, qi, idx, mn.SCALE, output=out, output_lse=lse, splits=3)

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(idx, out, lse)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()
        step(idx, out, lse)
        grown = torch.cuda.memory_allocated() - before
    ws_bytes = sum(t.numel() for t in torch.ops.hpc_mla._mla_indexer_prefill_workspaces() + torch.ops.hpc_mla._workspaces())
    assert grown <= ws_bytes, (grown, ws_bytes)  # nothing allocated in the capture beyond the cached scratch
    for c in (cases[0], cases[1], cases[0]):
        load(c)
        idx.fill_(-7)
        out.fill_(7)
        lse.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        want = pr.topk_statement(pr.logits_statement(c).float(), c, topk)
        assert torch.equal(idx.cpu(), want)
        eager = step(torch.empty_like(idx), torch.empty_like(out), torch.empty_like(lse))
        assert torch.equal(eager[0].view(torch.int16), out.view(torch.int16)) and torch.equal(eager[1].view(torch.int32), lse.view(torch.int32))
        assert bool(torch.isfinite(lse[: int(c["q_index"][-1])]).any())
    del graph
    hpc.release_decode_workspaces()
