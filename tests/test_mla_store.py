"""GPU: hpc.mla_rope_norm_store_kv against the float64 statement (tests/mla_store_ref.py::check_outputs, the bar
tests/test_mla_store_bar.py shows to have teeth): the main matrix, strided and padded layouts with every combination of
destinations, the in-kernel guards (page ids that are not pages, positions past the page table and past the cos / sin table,
each with in-range addresses only), a hipGraph replayed after the lengths changed, refusals, and the wire format - the
op's cache and q RoPE columns read by hpc.attention_decode_mla_bf16."""
import functools
from types import SimpleNamespace

import pytest
import torch

import mla_needles as mn
import mla_ref
import mla_store_ref as ms
from utils import attn_close, attn_rel_err

BF16 = torch.bfloat16


@functools.lru_cache(maxsize=2)
def _table_on_gpu(max_pos):
    return ms.cos_sin_table(max_pos).cuda()


def _call(c, sp, g, interleaved, cos_sin=None, bid=None, **kw):
    """the op on the GPU stores `g`; returns (what it returned, its out_q_pe argument).  cos_sin / bid: another table than the
    case's"""
    import hpc

    v = ms.views(c, sp, g)
    ret = hpc.mla_rope_norm_store_kv(v.cache, v.kv_a, _table_on_gpu(c.cos_sin.shape[0]) if cos_sin is None else cos_sin, g["w"],
                                     g["ns"], g["q_index"], g["bid"] if bid is None else bid,
                                     q_pe=v.q_pe, out_q_pe=v.out_q_pe, out_ckv=v.out_ckv, interleaved=interleaved, **kw)
    return ret, v.out_q_pe


def _run(c, sp, interleaved, label, stores=None):
    stores = ms.make_stores(c, sp) if stores is None else stores
    g = {k: t.cuda() for k, t in stores.items()}
    ret, out_q = _call(c, sp, g, interleaved)
    torch.cuda.synchronize()
    if sp.q in ("abs", "inplace"):
        assert ret is out_q  # the same object
    after = {k: t.cpu() for k, t in g.items()}
    failed = ms.check_outputs(c, sp, after, stores, ret.cpu() if sp.q == "fresh" else None, interleaved, label=label)
    assert not failed, (label, failed)
    return after


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("P", [16, 64, 128])
@pytest.mark.parametrize("H", [3, 16, 20, 128])
def test_main_matrix(H, P, interleaved):
    """every case builder; H = 3 a partial group of heads, 16 one full q-unit wave, 20 a ragged last wave, 128 the model's full
    head count"""
    for name in ms.CASES:
        _run(ms.case(name, H, P), ms.spec(), interleaved, f"{name} H {H} P {P} {'interleaved' if interleaved else 'neox'}")


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("layout", ms.LAYOUTS)
def test_layouts_and_destinations(layout, interleaved):
    """token stride 640 / a view into a larger pool, kv_a, q_pe and out_q_pe as slices of their parents, with the cache, out_ckv or
    both as destinations and every q mode (none, into q_abs, a fresh tensor, in place)"""
    c = ms.case("prefill", 20, 16)
    for cache, out_ckv in ((True, False), (False, True), (True, True)):
        for q in (None, "abs", "fresh", "inplace"):
            _run(c, ms.spec(layout, cache, out_ckv, q), interleaved, f"{layout} cache {cache} out_ckv {out_ckv} q {q}")


def _check_with_rows_unstored(c, sp, stores, after, unstored, label):
    """`unstored`: indices into the live rows whose token the kernel must NOT have stored.  Their cells (where the full page table
    puts them) must be as before the call; they are then filled in as if stored, and everything else must check out - every
    other token, out_ckv and out_q_pe of ALL rows, and every byte outside the written cells of every store."""
    ref = ms.reference(c, True)
    cache_after, cache_before = ms.views(c, sp, after).cache, ms.views(c, sp, stores).cache
    assert len(unstored)
    for i in unstored:
        p, s = int(ref.page[i]), int(ref.slot[i])
        assert torch.equal(cache_after[p, s].view(torch.int16), cache_before[p, s].view(torch.int16)), (label, int(ref.idx[i]))
        cache_after[p, s] = ref.lat[ref.idx[i]].bfloat16()
    failed = ms.check_outputs(c, sp, after, stores, None, True, label=label)
    assert not failed, (label, failed)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["-1", "num_blocks"])
def test_page_ids_that_are_no_pages_store_nothing(bad):
    """a page-table entry of -1 (how frameworks pad tables) or = num_blocks on a new token: that token is not stored, nothing
    else changes, every other output is as without it.  The cache is the view [1:-1, 2:2+P, :576] of a larger, sentinel-filled
    pool, so both ids address the pool's own first / last page: in-range memory that check_outputs compares byte for byte -
    a kernel without the guard writes there and fails, and no address outside the allocation is formed either way."""
    c, sp = ms.case("decode_mtp1_16", 16, 16), ms.spec("pool", out_ckv=True)
    ref = ms.reference(c, True)
    stores = ms.make_stores(c, sp)
    assert stores["cache"].shape[0] == c.nblocks + 2 and ms.views(c, sp, stores).cache.shape[0] == c.nblocks
    victim = 5  # a live row, alone on its page
    r, blk = int(ref.req[victim]), int(ref.pos[victim]) // c.P
    on_page = [i for i in range(ref.idx.numel()) if int(ref.req[ref.idx[i]]) == r and int(ref.pos[ref.idx[i]]) // c.P == blk]
    assert victim in [int(ref.idx[i]) for i in on_page]
    g = {k: t.cuda() for k, t in stores.items()}
    g["bid"][r, blk] = -1 if bad == "-1" else c.nblocks
    _call(c, sp, g, True)
    torch.cuda.synchronize()
    after = {k: t.cpu() for k, t in g.items()}
    after["bid"][r, blk] = c.bid[r, blk]  # the table as check_outputs knows it
    _check_with_rows_unstored(c, sp, stores, after, on_page, f"page id {bad}")


@pytest.mark.gpu
def test_positions_past_the_page_table_store_nothing():
    """block_ids with fewer columns than the positions need (a contiguous copy of the first 300 of them: pages of positions
    below 4800): the tokens at 8192+ are not stored - and their table entry is not read -, nothing else changes"""
    c, sp = ms.case("decode_mtp1_16", 16, 16), ms.spec("pool", out_ckv=True)
    ref = ms.reference(c, True)
    cols = 300
    beyond = [i for i in range(ref.idx.numel()) if int(ref.pos[ref.idx[i]]) // c.P >= cols]
    assert 4 <= len(beyond) < ref.idx.numel() - 4
    stores = ms.make_stores(c, sp)
    g = {k: t.cuda() for k, t in stores.items()}
    _call(c, sp, g, True, bid=g["bid"][:, :cols].contiguous())
    torch.cuda.synchronize()
    _check_with_rows_unstored(c, sp, stores, {k: t.cpu() for k, t in g.items()}, beyond, "short page table")


@pytest.mark.gpu
def test_positions_past_the_cos_sin_table_read_its_last_row():
    """cos_sin given as the first 4200 rows of the longer table (the rows behind them exist: in-range memory): rows at
    8192+ are unspecified by the contract; the kernel's rule is the table's last row, so the result is the statement's over
    a table whose rows from 4200 on repeat row 4199 - a kernel without the clamp reads the real rows and differs.  Every
    other row, and every byte outside the written cells, is as always."""
    c, sp = ms.case("decode_mtp1_16", 16, 16), ms.spec("pool", out_ckv=True)
    k = 4200
    assert int((ms.reference(c, True).pos >= k).sum()) >= 4
    table = c.cos_sin.clone()
    table[k:] = table[k - 1]
    clamped = SimpleNamespace(**{**vars(c), "cos_sin": table, "refs": {}})
    assert not torch.equal(ms.reference(clamped, True).q, ms.reference(c, True).q)
    stores = ms.make_stores(c, sp)
    g = {k_: t.cuda() for k_, t in stores.items()}
    _call(c, sp, g, True, cos_sin=_table_on_gpu(c.cos_sin.shape[0])[:k])
    torch.cuda.synchronize()
    failed = ms.check_outputs(clamped, sp, {k_: t.cpu() for k_, t in g.items()}, stores, None, True, label="short cos_sin table")
    assert not failed, failed


@pytest.mark.gpu
def test_graph_replays_with_new_lengths():
    """one call captured with every output given; the lengths are then changed in place: the replay follows the new lengths"""
    c, sp = ms.case("decode_mtp1_16", 16, 64), ms.spec("padded", out_ckv=True)
    stores = ms.make_stores(c, sp)
    g = {k: t.cuda() for k, t in stores.items()}
    fresh = {k: t.clone() for k, t in g.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(c, sp, g, True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()
        _call(c, sp, g, True)
        assert torch.cuda.memory_allocated() == before  # nothing allocated per call
    # shorter by 3 tokens where that stays on the pages the case owns, else longer by 2: other slots, other positions
    ns = c.ns.clone()
    for r, (s, n) in enumerate(c.reqs):
        lo = (s - n) // c.P * c.P
        ns[r] = s - 3 if s - 3 - n >= lo else s + 2 if (s + 1) // c.P == (s - 1) // c.P else s
    assert int((ns != c.ns).sum()) >= c.num_req // 2
    moved = ms.build_case("moved", [(int(ns[r]), n) for r, (_, n) in enumerate(c.reqs)], c.H, c.P, 0, pad_rows=c.rows - c.real_rows)
    for k in ("y", "q_src", "w", "cache0", "q_nope", "bid", "cos_sin"):
        setattr(moved, k, getattr(c, k))
    for case, lens in ((c, c.ns), (moved, ns), (c, c.ns)):
        for k, t in fresh.items():
            g[k].copy_(t)
        g["ns"].copy_(lens)
        graph.replay()
        torch.cuda.synchronize()
        want = dict(stores, ns=lens.clone())
        failed = ms.check_outputs(case, sp, {k: t.cpu() for k, t in g.items()}, want, None, True, label="graph " + case.name)
        assert not failed, failed


@pytest.mark.gpu
def test_refusals_and_empty_calls():
    import hpc

    c, sp = ms.case("decode_mtp0_7", 16, 16), ms.spec("plain", out_ckv=True)
    g = {k: t.cuda() for k, t in ms.make_stores(c, sp).items()}
    v = ms.views(c, sp, g)
    cs = _table_on_gpu(ms.MAX_POS)
    args = [v.cache, v.kv_a, cs, g["w"], g["ns"], g["q_index"], g["bid"]]

    def refused(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match):
            hpc.mla_rope_norm_store_kv(*a, **kw)

    def swap(i, t):
        return args[:i] + [t] + args[i + 1:]

    refused("one of ckv_cache and out_ckv", None, *args[1:])
    refused("out_q_pe needs q_pe", *args, out_q_pe=v.out_q_pe)
    refused("kv_a dtype", *swap(1, v.kv_a.float()))
    refused("ckv_cache dtype", *swap(0, v.cache.float()))
    refused("cos_sin dtype", *swap(2, cs.double()))
    refused("kv_norm_weight dtype", *swap(3, g["w"].bfloat16()))
    refused("num_seqlen_per_req dtype", *swap(4, g["ns"].long()))
    refused("q_index dtype", *swap(5, g["q_index"].long()))
    refused("block_ids dtype", *swap(6, g["bid"].long()))
    refused("cuda|device", *swap(3, g["w"].cpu()))
    refused("block_size", *swap(0, v.cache[:, :8]))
    refused("block_size", *swap(0, torch.zeros(4, 48, 576, dtype=BF16, device="cuda")))
    refused("token stride", *swap(0, torch.zeros(4, 16, 580, dtype=BF16, device="cuda")[:, :, :576]))
    refused("16-byte aligned", *swap(0, torch.zeros(4 * 16 * 576 + 8, dtype=BF16, device="cuda")[4:-4].view(4, 16, 576)))
    refused("contiguous last dim", *swap(0, torch.zeros(4, 16, 1152, dtype=BF16, device="cuda")[:, :, ::2]))
    refused("kv_a stride", *swap(1, torch.zeros(c.rows, 580, dtype=BF16, device="cuda")[:, :576]))
    refused("kv_a must be 16-byte aligned", *swap(1, torch.zeros(c.rows, 584, dtype=BF16, device="cuda")[:, 4:580]))
    refused("kv_a must be", *swap(1, torch.zeros(c.rows, 512, dtype=BF16, device="cuda")))
    refused("num_head", *args, q_pe=torch.zeros(c.rows, 129, 64, dtype=BF16, device="cuda"))
    refused("num_head", *args, q_pe=torch.zeros(c.rows, 0, 64, dtype=BF16, device="cuda"))
    refused("q_pe stride", *args, q_pe=torch.zeros(c.rows, 4, 68, dtype=BF16, device="cuda")[..., :64])
    refused("out_q_pe must have shape", *args, q_pe=v.q_pe, out_q_pe=torch.zeros(c.rows, 4, 64, dtype=BF16, device="cuda"))
    refused("lets its rows overlap", *args, q_pe=v.q_pe, 
            out_q_pe=torch.zeros((c.rows + 16) * 64, dtype=BF16, device="cuda").as_strided((c.rows, 16, 64), (64, 64, 1)))
    refused("overlaps q_pe", *args, q_pe=v.q_pe[:, :8], out_q_pe=v.q_pe[:, 4:12])
    refused("out_ckv stride", *args, out_ckv=torch.zeros(c.rows, 580, dtype=BF16, device="cuda")[:, :576])
    refused("q_index must be", *swap(5, g["q_index"][:-1]))
    refused("cos_sin must be", *swap(2, torch.zeros(64, 128, device="cuda")))

    # rows == 0 and num_req == 0: no launch, nothing written
    before = {k: t.clone() for k, t in g.items()}
    none = hpc.mla_rope_norm_store_kv(v.cache, v.kv_a[:0], cs, g["w"], g["ns"], g["q_index"], g["bid"], q_pe=v.q_pe[:0])
    assert none.shape == (0, 16, 64)
    assert hpc.mla_rope_norm_store_kv(v.cache, v.kv_a, cs, g["w"], g["ns"][:0], g["q_index"][:1], g["bid"][:0]) is None
    torch.cuda.synchronize()
    assert all(torch.equal(g[k].view(torch.int16) if g[k].dtype == BF16 else g[k],
                           before[k].view(torch.int16) if g[k].dtype == BF16 else before[k]) for k in g)


@pytest.mark.gpu
def test_wire_format_is_what_the_decode_op_reads():
    """the new tokens of a decode batch written by this op into a cache that holds the earlier tokens, and into
    q_abs[..., 512:]; then hpc.attention_decode_mla_bf16 over them, against tests/mla_ref.py::mla_statement over a cache and
    q assembled on the CPU from this op's float64 statement rounded to bf16 - at the decode test's own bars"""
    import hpc

    B, H, mtp, P = 3, 16, 1, 16
    sq = mtp + 1
    inp = mn.uniform_inputs([17, 40, 131], sq, P, H, seed=77)  # the earlier tokens, the q columns :512, the page table
    g = torch.Generator().manual_seed(78)
    rows = B * sq
    y = torch.randn(rows, 2112, generator=g).bfloat16()
    q_src = (torch.randn(rows, H, 192, generator=g) / 24).bfloat16()
    w = 1 + 0.1 * torch.randn(512, generator=g)
    cs = ms.cos_sin_table(ms.MAX_POS)
    q_index = torch.arange(0, rows + 1, sq, dtype=torch.int32)
    kv_a, q_pe = y[:, ms.KV_A_AT:], q_src[..., ms.Q_PE_AT:]
    lat, q64, req, pos = ms.statement(kv_a, q_pe, cs, w, inp["lens_total"], q_index, True)
    assert pos.tolist() == [17, 18, 40, 41, 131, 132]
    ckv_ref, q_ref = inp["ckv"].clone(), inp["q"].clone()
    ckv_ref[inp["block_ids"][req, pos // P].long(), pos % P] = lat.bfloat16()
    q_ref[..., 512:] = q64.bfloat16()
    want, want_lse = mla_ref.mla_statement(q_ref, ckv_ref, inp["block_ids"], inp["lens_total"], sq, mn.SCALE)

    ckv, q_abs = inp["ckv"].cuda(), inp["q"].cuda()
    bid, lens = inp["block_ids"].cuda(), inp["lens_total"].cuda()
    ret = hpc.mla_rope_norm_store_kv(ckv, y.cuda()[:, ms.KV_A_AT:], cs.cuda(), w.cuda(), lens, q_index.cuda(), bid,
                                     q_pe=q_src.cuda()[..., ms.Q_PE_AT:], out_q_pe=q_abs[..., 512:])
    assert ret.data_ptr() == q_abs[..., 512:].data_ptr()
    out, lse = hpc.attention_decode_mla_bf16(q_abs, ckv, bid, lens, mn.SCALE, mtp=mtp, new_kv_included=True, return_lse=True)
    w_out, w_lse = float(attn_rel_err(want.to(BF16), out.cpu(), sq).max()), mn.lse_err(want_lse, lse)
    print(f"wire format: out worst {w_out:.5f} (tau {mn.TAU_UNIFORM}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_UNIFORM})")
    assert attn_close(want.to(BF16), out.cpu(), mn.TAU_UNIFORM, sq, label="wire format")
    assert w_lse <= mn.LSE_BAR_UNIFORM, w_lse
    # and the op's own outputs on its bar: the decode op read what the statement says was written
    got = ckv.cpu()[inp["block_ids"][req, pos // P].long(), pos % P]
    from utils import rope_close

    assert rope_close(lat[:, None, :512], got[:, None, :512], label="wire latent")
    assert rope_close(lat[:, None, 512:], got[:, None, 512:], label="wire k_pe")
    assert rope_close(q64, q_abs.cpu()[..., 512:], label="wire q_pe")
    assert torch.equal(q_abs.cpu()[..., :512], inp["q"][..., :512])
