"""hpc.mla_rope_norm_store_kv_fp8: the writer of the FP8 latent KV cache (656 bytes per token, tests/mla_fp8_ref.py).

The FP8 row is an exact function of the bf16 row hpc.mla_rope_norm_store_kv stores (the quantiser works on the bf16-rounded
values), so every GPU check is bitwise against the bf16 op on the same inputs: each new token's cell = quantise(bf16 cell), every
other byte of the uint8 allocation as before the call, out_q_pe / out_ckv equal to the bf16 op's; the guards; and the round trip
through hpc.attention_decode_mla_fp8.  CPU: surface, fakes, host refusals through the C-ABI with never-dereferenced pointers."""
import ctypes
import functools
from pathlib import Path

import pytest
import torch

import mla_fp8_ref as f8
import mla_needles as mn
import mla_ref
import mla_store_ref as ms
from utils import attn_close, attn_rel_err

BF16 = torch.bfloat16
FILL = 0x5A
LAYOUTS = ("plain", "padded", "pool")  # contiguous / token stride 704 / a view into a larger pool


# ------------------------------------------------------------------------------------------------------ surface, fakes
def test_surface():
    import hpc

    assert "mla_rope_norm_store_kv_fp8" in hpc.__all__ and callable(hpc.mla_rope_norm_store_kv_fp8)
    doc = hpc.mla_rope_norm_store_kv_fp8.__doc__
    for word in ("656", "offset 0", "offset 512", "offset 528", "c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] )",
                 "amax / 448", "1e-8", "bit-identical", "torch.uint8", "{16, 32, 64, 128}", "out_q_pe", "out_ckv",
                 "tests/blockwise_quant_ref.py"):
        assert word in doc, word


def test_both_libraries_export_the_launcher():
    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for name in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        assert hasattr(ctypes.CDLL(str(pkg / name)), "hpc_mla_rope_norm_store_kv_fp8_async"), name


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        def T(*shape, dtype=BF16):
            return torch.empty(shape, dtype=dtype, device="cuda")

        rows, H = 6, 20
        ckv, kv_a = T(9, 64, 656, dtype=torch.uint8), T(rows, 2112)[:, 1536:]
        cs, w = T(4096, 64, dtype=torch.float32), T(512, dtype=torch.float32)
        ns, qi, bid = T(3, dtype=torch.int32), T(4, dtype=torch.int32), T(3, 64, dtype=torch.int32)
        q_pe, q_abs, ockv = T(rows, H, 192)[..., 128:], T(rows, H, 576), T(rows, 576)
        for cache in (ckv, None):
            for out_ckv in (ockv, None):
                if cache is None and out_ckv is None:
                    continue
                raw = torch.ops.hpc_mla.rope_norm_store_kv_fp8(cache, kv_a, cs, w, ns, qi, bid, None, None, out_ckv, 1e-6, True)
                assert raw.shape == (0,) and raw.dtype == BF16  # the entry's placeholder without q_pe
                assert hpc.mla_rope_norm_store_kv_fp8(cache, kv_a, cs, w, ns, qi, bid, out_ckv=out_ckv) is None
                y = hpc.mla_rope_norm_store_kv_fp8(cache, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_ckv=out_ckv, interleaved=False)
                assert (y.shape, y.dtype, y.device.type) == ((rows, H, 64), BF16, "cuda") and y.is_contiguous()
                out = q_abs[..., 512:]
                assert hpc.mla_rope_norm_store_kv_fp8(cache, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_q_pe=out, out_ckv=out_ckv) is out
                assert hpc.mla_rope_norm_store_kv_fp8(cache, kv_a, cs, w, ns, qi, bid, q_pe=q_pe, out_q_pe=q_pe, out_ckv=out_ckv) is q_pe


# ------------------------------------------------------------------------------------------------- the C-ABI on the host
UNSUPPORTED, INVALID = -1, -2


def _launch(**kw):
    """hpc_mla_rope_norm_store_kv_fp8_async (cache strides in bytes) with pointers that are never dereferenced on the host;
    every case here is refused, or has nothing to launch, before any device call"""
    from ctypes import POINTER, c_float, c_int, c_int64, c_void_p, cast

    from hpc import _C

    a = dict(cache=4096, out_ckv=0, out_q_pe=1 << 20, kv_a=4096, q_pe=4096, cos_sin=4096, w=4096, ns=4096, qi=4096, bid=4096, rows=6,
             num_req=3, H=16, P=64, max_blocks=8, num_blocks=9, max_pos=4096, bs=64 * 656, ts=656, kv_rs=2112, ockv_rs=576,
             q_rs=16 * 192, q_hs=192, oq_rs=16 * 576, oq_hs=576, eps=1e-6, interleaved=1)
    a.update(kw)
    vp = lambda v: c_void_p(v) if v else None  # noqa: E731
    ip = lambda v: cast(c_void_p(v), POINTER(c_int)) if v else None  # noqa: E731
    return _C.lib.hpc_mla_rope_norm_store_kv_fp8_async(
        vp(a["cache"]), vp(a["out_ckv"]), vp(a["out_q_pe"]), vp(a["kv_a"]), vp(a["q_pe"]), vp(a["cos_sin"]), vp(a["w"]), ip(a["ns"]),
        ip(a["qi"]), ip(a["bid"]), a["rows"], a["num_req"], a["H"], a["P"], a["max_blocks"], a["num_blocks"], a["max_pos"],
        c_int64(a["bs"]), c_int64(a["ts"]), c_int64(a["kv_rs"]), c_int64(a["ockv_rs"]), c_int64(a["q_rs"]), c_int64(a["q_hs"]),
        c_int64(a["oq_rs"]), c_int64(a["oq_hs"]), c_float(a["eps"]), a["interleaved"], None)


@pytest.mark.parametrize("kwargs,code", [
    # the cache's strides in bytes
    (dict(ts=655), UNSUPPORTED), (dict(ts=660), UNSUPPORTED), (dict(ts=672 - 8), UNSUPPORTED), (dict(ts=576), UNSUPPORTED),
    (dict(bs=64 * 656 + 8), UNSUPPORTED), (dict(bs=64 * 656 + 4), UNSUPPORTED), (dict(cache=4096 + 8), UNSUPPORTED),
    (dict(bs=-64 * 656), INVALID),
    # the bf16 launcher's table
    (dict(H=0), UNSUPPORTED), (dict(H=129), UNSUPPORTED), (dict(P=48), UNSUPPORTED), (dict(P=256), UNSUPPORTED),
    (dict(kv_a=4096 + 2), UNSUPPORTED), (dict(kv_rs=2116), UNSUPPORTED), (dict(kv_rs=568), UNSUPPORTED), (dict(q_pe=4096 + 4), UNSUPPORTED),
    (dict(out_q_pe=(1 << 20) + 8), UNSUPPORTED), (dict(q_hs=196), UNSUPPORTED), (dict(oq_hs=56), UNSUPPORTED), (dict(oq_rs=580), UNSUPPORTED),
    (dict(oq_rs=15 * 576 + 56), UNSUPPORTED), (dict(oq_hs=64, oq_rs=512), UNSUPPORTED), (dict(out_q_pe=4096 + 128), UNSUPPORTED),
    (dict(out_q_pe=4096, oq_rs=16 * 192, oq_hs=200), UNSUPPORTED), (dict(out_q_pe=4096 + 2 * (5 * 16 * 192 + 15 * 192 + 64) - 16), UNSUPPORTED),
    (dict(out_ckv=4096 + 4), UNSUPPORTED), (dict(out_ckv=4096, ockv_rs=568), UNSUPPORTED), (dict(cos_sin=4096 + 4), UNSUPPORTED),
    (dict(w=4096 + 8), UNSUPPORTED),
    (dict(cache=0), INVALID), (dict(q_pe=0), INVALID), (dict(out_q_pe=0), INVALID), (dict(kv_a=0), INVALID), (dict(cos_sin=0), INVALID),
    (dict(w=0), INVALID), (dict(ns=0), INVALID), (dict(qi=0), INVALID), (dict(bid=0), INVALID), (dict(rows=-1), INVALID),
    (dict(num_req=-1), INVALID), (dict(H=-1), INVALID), (dict(max_blocks=-1), INVALID), (dict(num_blocks=-1), INVALID),
    (dict(max_pos=0), INVALID),
    # nothing to launch: 0 without a device call - also with the strides a padded cache and a pool view have
    (dict(rows=0), 0), (dict(num_req=0), 0), (dict(cache=0, out_ckv=4096, bid=0, rows=0), 0), (dict(q_pe=0, out_q_pe=0, H=0, rows=0), 0),
    (dict(rows=0, ts=672, bs=64 * 672), 0), (dict(rows=0, ts=704, bs=67 * 704), 0),
    # the cache's rule (csrc/mla_cache.h), as the readers' tables pin it: it holds for a call without rows too, a negative
    # block stride is an invalid argument that wins over whatever is merely unsupported, and an absent cache has no page size
    (dict(ts=-656), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=0), UNSUPPORTED), (dict(rows=0, P=48), UNSUPPORTED),
    (dict(P=48, bs=-64 * 656), INVALID), (dict(rows=0, cache=0, out_ckv=4096, P=48), 0),
])
def test_cabi_refuses_on_the_host(kwargs, code):
    assert _launch(**kwargs) == code


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=2)
def _table_on_gpu(max_pos):
    return ms.cos_sin_table(max_pos).cuda()


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t


def _shape8(c, layout):
    return {"plain": (c.nblocks, c.P, 656), "padded": (c.nblocks, c.P, 704), "pool": (c.nblocks + 2, c.P + 3, 704)}[layout]


def _view8(c, layout, t):
    """the op's cache argument as a view of the allocation t"""
    return {"plain": t, "padded": t[:, :, :656], "pool": t[1:-1, 2: 2 + c.P, :656]}[layout]


def _both(c, layout, q, interleaved, bid8=None):
    """the bf16 op into a contiguous bf16 cache and the FP8 op into a uint8 cache of `layout`, on the same inputs.  Returns
    (bf16 stores after, fp8 stores after, uint8 allocation after, both returns).  bid8: another page table for the FP8 call."""
    import hpc

    sp16, sp8 = ms.spec("plain", True, True, q), ms.spec("plain", False, True, q)
    table = _table_on_gpu(c.cos_sin.shape[0])
    g16 = {k: t.cuda() for k, t in ms.make_stores(c, sp16).items()}
    v = ms.views(c, sp16, g16)
    r16 = hpc.mla_rope_norm_store_kv(v.cache, v.kv_a, table, g16["w"], g16["ns"], g16["q_index"], g16["bid"], q_pe=v.q_pe,
                                     out_q_pe=v.out_q_pe, out_ckv=v.out_ckv, interleaved=interleaved)
    g8 = {k: t.cuda() for k, t in ms.make_stores(c, sp8).items()}
    alloc = torch.full(_shape8(c, layout), FILL, dtype=torch.uint8, device="cuda")
    cache8 = _view8(c, layout, alloc)
    v = ms.views(c, sp8, g8)
    r8 = hpc.mla_rope_norm_store_kv_fp8(cache8, v.kv_a, table, g8["w"], g8["ns"], g8["q_index"], g8["bid"] if bid8 is None else bid8,
                                        q_pe=v.q_pe, out_q_pe=v.out_q_pe, out_ckv=v.out_ckv, interleaved=interleaved)
    torch.cuda.synchronize()
    if q in ("abs", "inplace"):
        assert r8 is v.out_q_pe  # the same object
    return {k: t.cpu() for k, t in g16.items()}, {k: t.cpu() for k, t in g8.items()}, alloc.cpu(), (r16, r8)


def _expect_alloc(c, layout, cells16, page, slot):
    """the uint8 allocation after a call that stored the tokens (page, slot) whose bf16 rows are cells16: quantise(cell) there,
    FILL everywhere else"""
    want = torch.full(_shape8(c, layout), FILL, dtype=torch.uint8)
    _view8(c, layout, want)[page, slot] = f8.quantise(cells16)
    return want


def _compare(c, layout, q, interleaved, label):
    ref = ms.reference(c, interleaved)
    a16, a8, alloc, (r16, r8) = _both(c, layout, q, interleaved)
    cells16 = ms.views(c, ms.spec("plain", True, True, q), a16).cache[ref.page, ref.slot]  # what the bf16 op stored
    got = _view8(c, layout, alloc)[ref.page, ref.slot]
    want = f8.quantise(cells16)
    assert torch.equal(got[:, :512], want[:, :512]), f"{label}: codes"
    assert torch.equal(got[:, 512:528], want[:, 512:528]), f"{label}: scale bits"
    assert torch.equal(got[:, 528:], want[:, 528:]), f"{label}: RoPE bytes"
    # every other byte of the allocation: token-stride padding, page tails, unlisted pages, the guard page, rows of no request
    assert torch.equal(alloc, _expect_alloc(c, layout, cells16, ref.page, ref.slot)), f"{label}: a byte outside the new cells changed"
    for k in a8:  # out_ckv, out_q_pe (abs / in place) and every input: bit-equal to the bf16 op's
        assert torch.equal(_bits(a8[k]), _bits(a16[k])), f"{label}: {k}"
    if q == "fresh":
        assert r8.shape == r16.shape and r8.dtype == BF16 and r8.is_contiguous()
        assert torch.equal(_bits(r8.cpu()), _bits(r16.cpu())), f"{label}: returned q_pe"


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [True, False])
@pytest.mark.parametrize("H,P", [(16, 64), (128, 16)])
def test_cells_are_the_quantised_bf16_cells_and_nothing_else_changes(H, P, interleaved):
    for name in ("decode_mtp1_16", "decode_mtp3_7", "prefill"):
        c = ms.case(name, H, P)
        assert c.rows > c.real_rows  # rows of no request: they store nothing (the whole-allocation check)
        for layout, q in zip(LAYOUTS, ("abs", "fresh", "inplace")):
            _compare(c, layout, q, interleaved, f"{name} H {H} P {P} {layout} q {q} {'interleaved' if interleaved else 'neox'}")


@pytest.mark.gpu
def test_without_a_cache_out_ckv_is_the_bf16_ops():
    import hpc

    c = ms.case("decode_mtp3_7", 16, 64)
    sp = ms.spec("plain", False, True, None)
    outs = []
    for op in (hpc.mla_rope_norm_store_kv, hpc.mla_rope_norm_store_kv_fp8):
        g = {k: t.cuda() for k, t in ms.make_stores(c, sp).items()}
        v = ms.views(c, sp, g)
        assert op(None, v.kv_a, _table_on_gpu(c.cos_sin.shape[0]), g["w"], g["ns"], g["q_index"], g["bid"], out_ckv=v.out_ckv) is None
        outs.append(g["ockv"].cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["-1", "num_blocks"])
def test_page_ids_that_are_no_pages_store_nothing(bad):
    """a page-table entry of -1 (how frameworks pad tables) or = num_blocks on a new token: that token is not stored and nothing
    else changes.  The cache is the view [1:-1, 2:2+P, :656] of a larger pool, so both ids address the pool's own first / last
    page: in-range memory that is compared byte for byte, and no address outside the allocation is formed either way."""
    c = ms.case("decode_mtp1_16", 16, 16)
    ref = ms.reference(c, True)
    victim = 5  # a live row
    r, blk = int(ref.req[victim]), int(ref.pos[victim]) // c.P
    on_page = torch.tensor([int(ref.req[i]) == r and int(ref.pos[i]) // c.P == blk for i in ref.idx.tolist()])
    assert bool(on_page[ref.idx.tolist().index(victim)]) and 1 <= int(on_page.sum()) < on_page.numel()
    bid = c.bid.clone()
    bid[r, blk] = -1 if bad == "-1" else c.nblocks
    a16, a8, alloc, _ = _both(c, "pool", "abs", True, bid8=bid.cuda())
    cells16 = ms.views(c, ms.spec("plain", True, True, "abs"), a16).cache[ref.page, ref.slot]
    keep = ~on_page
    assert torch.equal(alloc, _expect_alloc(c, "pool", cells16[keep], ref.page[keep], ref.slot[keep]))
    for k in a8:  # out_ckv and out_q_pe of ALL rows are as without the bad entry
        assert torch.equal(_bits(a8[k]), _bits(a16[k])), k


@pytest.mark.gpu
def test_positions_past_the_page_table_store_nothing():
    """block_ids with fewer columns than the positions need: the tokens at 8192+ are not stored, nothing else changes"""
    c = ms.case("decode_mtp1_16", 16, 16)
    ref = ms.reference(c, True)
    cols = 300
    keep = ref.pos[ref.idx] // c.P < cols
    assert 4 <= int((~keep).sum()) < keep.numel() - 4
    a16, a8, alloc, _ = _both(c, "padded", "abs", True, bid8=c.bid[:, :cols].contiguous().cuda())
    cells16 = ms.views(c, ms.spec("plain", True, True, "abs"), a16).cache[ref.page, ref.slot]
    assert torch.equal(alloc, _expect_alloc(c, "padded", cells16[keep], ref.page[keep], ref.slot[keep]))


@pytest.mark.gpu
def test_refusals_through_the_op():
    import hpc

    c, sp = ms.case("decode_mtp0_7", 16, 16), ms.spec("plain", False, True)
    g = {k: t.cuda() for k, t in ms.make_stores(c, sp).items()}
    v = ms.views(c, sp, g)
    cs = _table_on_gpu(ms.MAX_POS)
    rest = [v.kv_a, cs, g["w"], g["ns"], g["q_index"], g["bid"]]

    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8, device="cuda")

    def refused(match, cache, op=hpc.mla_rope_norm_store_kv_fp8):
        with pytest.raises(RuntimeError, match=match):
            op(cache, *rest)

    refused("ckv_cache dtype must be uint8", torch.zeros(c.nblocks, 16, 576, dtype=BF16, device="cuda"))
    refused("ckv_cache dtype must be bfloat16", u8(c.nblocks, 16, 656), op=hpc.mla_rope_norm_store_kv)
    refused("656", u8(c.nblocks, 16, 576))
    refused("block_size", u8(c.nblocks, 48, 656))
    refused("token stride", u8(c.nblocks, 16, 664)[:, :, :656])
    refused("16-byte aligned", u8(c.nblocks * 16 * 656 + 16)[8:-8].view(c.nblocks, 16, 656))
    refused("contiguous last dim", u8(c.nblocks, 16, 1312)[:, :, ::2])
    refused("one of ckv_cache and out_ckv", None)


# --------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.gpu
def test_round_trip_through_the_fp8_decode_op():
    """the FP8 writer fills the cache of requests of 63, 64 and 700 cached tokens plus the step's mtp + 1 new ones; then
    hpc.attention_decode_mla_fp8 over it equals hpc.attention_decode_mla_bf16 over dequantise(cache) bit for bit, and both meet
    the needle-free generator's bar against the float64 statement on that dequantised cache"""
    import hpc

    H, mtp, P = 16, 1, 64
    sq = mtp + 1
    totals = torch.tensor([63 + sq, 64 + sq, 700 + sq], dtype=torch.int32)
    B, rows = len(totals), int(totals.sum())
    g = torch.Generator().manual_seed(90)
    nb = (totals + P - 1) // P
    pool = int(nb.sum()) + 3
    perm = torch.randperm(pool, generator=g).int()
    bid = torch.full((B, int(nb.max())), -999999, dtype=torch.int32)
    o = 0
    for b, n in enumerate(nb.tolist()):
        bid[b, :n] = perm[o: o + n]
        o += n
    kv_a = torch.randn(rows, 576, generator=g).bfloat16()
    w = 1 + 0.1 * torch.randn(512, generator=g)
    q_index = torch.cat([torch.zeros(1, dtype=torch.int32), totals.cumsum(0).int()])
    cache = torch.zeros(pool, P, 656, dtype=torch.uint8, device="cuda")  # spare pages and page tails: zeros (scale 0)
    # -999999 entries lie past every request's pages and are never reached: every position is below the request's length
    assert hpc.mla_rope_norm_store_kv_fp8(cache, kv_a.cuda(), ms.cos_sin_table(ms.MAX_POS).cuda(), w.cuda(), totals.cuda(),
                                          q_index.cuda(), bid.cuda()) is None
    deq = f8.dequantise(cache.cpu())
    used = deq[bid[2, : int(nb[2])].long()].reshape(-1, 576)[: int(totals[2])]
    assert bool((used[:, :512].float().abs().amax(-1) > 0.5).all())  # every token of the long request was written

    q = (torch.randn(B * sq, H, 576, generator=g) / 24).bfloat16()
    args = (bid.cuda(), totals.cuda(), mn.SCALE)
    out8, lse8 = hpc.attention_decode_mla_fp8(q.cuda(), cache, *args, mtp=mtp, new_kv_included=True, return_lse=True)
    out16, lse16 = hpc.attention_decode_mla_bf16(q.cuda(), deq.cuda(), *args, mtp=mtp, new_kv_included=True, return_lse=True)
    assert torch.equal(_bits(out8), _bits(out16)) and torch.equal(lse8.view(torch.int32), lse16.view(torch.int32))
    want, want_lse = mla_ref.mla_statement(q, deq, bid, totals, sq, mn.SCALE)
    w_out, w_lse = float(attn_rel_err(want.to(BF16), out8.cpu(), sq).max()), mn.lse_err(want_lse, lse8)
    print(f"round trip: out worst {w_out:.5f} (tau {mn.TAU_UNIFORM}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_UNIFORM})")
    assert attn_close(want.to(BF16), out8.cpu(), mn.TAU_UNIFORM, sq, label="round trip")
    assert w_lse <= mn.LSE_BAR_UNIFORM, w_lse
