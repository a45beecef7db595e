"""hpc.mla_gather_ckv / hpc.mla_gather_ckv_fp8: the paged MLA latent cache gathered (and, for FP8, dequantised) into contiguous
bf16 [T, 576] rows.  Statement, mutants and case builder: tests/mla_gather_ref.py.

Every comparison of gathered rows is bitwise, on int16 views: the bf16 path moves bits, and the FP8 path must give
tests/mla_fp8_ref.py::dequantise of the row - the dequantisation hpc.attention_decode_mla_fp8 applies - bit for bit.

CPU: surface, launchers, fakes, host refusals through the C-ABI with never-dereferenced pointers, the planner
hpc.mla_context_chunks, and `test_inputs_have_teeth`: the GPU cases tell every mutant of the statement from the statement.  A
mutant can differ only in requests it touches at all, so each one is held to every request of every case in which the mutated
quantity differs from the true one:
    seq_starts ignored                 requests with a start != 0
    table column off at a page edge    requests that hold the last slot of a page
    pos % P <- offset in the request   requests with start % P != 0
    the next request's table row       every non-empty request
    the next group's scale, truncation, k_pe from byte 512 (FP8)      every non-empty request
    a guard row left unwritten         every guard row of the guard cases
GPU: the cases against the statement with every other byte of the output buffer unchanged, the guards, the round trip with the
two writers, a hipGraph replayed after the device lengths changed, and a pool whose third page lies beyond 4 GiB."""
import ctypes
import functools
import random
from pathlib import Path

import pytest
import torch

import mla_fp8_ref as f8
import mla_gather_ref as gr
import mla_store_ref as ms

BF16 = torch.bfloat16
NAMES = ("mla_gather_ckv", "mla_gather_ckv_fp8")
PAGES = (16, 128)


# ------------------------------------------------------------------------------------------------------ surface, fakes
def test_surface():
    import hpc

    for name in NAMES + ("mla_context_chunks",):
        assert name in hpc.__all__ and callable(getattr(hpc, name)), name
    for name in NAMES:
        doc = getattr(hpc, name).__doc__
        for word in ("cu_seqlens[b] <= r < cu_seqlens[b + 1]", "pos = seq_starts[b] + (r - cu_seqlens[b])", "pos < 0",
                     "pos // P >= max_blocks", "[0, num_blocks)", "576 zeros", "not written", "hipGraph", "num_rows",
                     "{16, 32, 64, 128}", "tests/mla_gather_ref.py" if name == NAMES[0] else "tests/mla_fp8_ref.py"):
            assert word in doc, (name, word)
    assert "ckv_cache[block_ids[b, pos // P], pos % P, :576]" in hpc.mla_gather_ckv.__doc__
    assert "bf16_rne( fp32(code[d]) * scale[d // 128] )" in hpc.mla_gather_ckv_fp8.__doc__
    assert "byte offset 528" in hpc.mla_gather_ckv_fp8.__doc__ and "torch.uint8" in hpc.mla_gather_ckv_fp8.__doc__


def test_both_libraries_export_the_launchers():
    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for lib in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        for fn in ("hpc_mla_gather_ckv_async", "hpc_mla_gather_ckv_fp8_async"):
            assert hasattr(ctypes.CDLL(str(pkg / lib)), fn), (lib, fn)


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        def T(*shape, dtype=BF16):
            return torch.empty(shape, dtype=dtype, device="cuda")

        bid, cu, st = T(3, 9, dtype=torch.int32), T(4, dtype=torch.int32), T(3, dtype=torch.int32)
        for name, cache in ((NAMES[0], T(9, 64, 576)), (NAMES[1], T(9, 64, 656, dtype=torch.uint8))):
            op = getattr(hpc, name)
            out = T(50, 640)[3:40, :576]
            assert op(cache, bid, cu, output=out) is out
            assert op(cache, bid, cu, seq_starts=st, output=out, num_rows=37) is out
            y = op(cache, bid, cu, seq_starts=st, num_rows=21)
            assert (y.shape, y.dtype, y.device.type) == ((21, 576), BF16, "cuda") and y.is_contiguous()
            with pytest.raises(RuntimeError, match="one of output and num_rows"):
                op(cache, bid, cu, seq_starts=st)


# ------------------------------------------------------------------------------------------------- the C-ABI on the host
UNSUPPORTED, INVALID = -1, -2


def _launch(fp8, **kw):
    """hpc_mla_gather_ckv[_fp8]_async with pointers that are never dereferenced on the host; every case here is refused, or has
    nothing to launch, before any device call"""
    from ctypes import POINTER, c_int, c_int64, c_void_p, cast

    from hpc import _C

    row = 656 if fp8 else 576
    a = dict(out=1 << 20, cache=4096, bid=4096, cu=4096, st=4096, rows=40, num_req=3, P=64, max_blocks=8, num_blocks=9,
             bs=64 * row, ts=row, out_rs=576)
    a.update(kw)
    vp = lambda v: c_void_p(v) if v else None  # noqa: E731
    ip = lambda v: cast(c_void_p(v), POINTER(c_int)) if v else None  # noqa: E731
    fn = _C.lib.hpc_mla_gather_ckv_fp8_async if fp8 else _C.lib.hpc_mla_gather_ckv_async
    return fn(vp(a["out"]), vp(a["cache"]), ip(a["bid"]), ip(a["cu"]), ip(a["st"]), a["rows"], a["num_req"], a["P"], a["max_blocks"],
              a["num_blocks"], c_int64(a["bs"]), c_int64(a["ts"]), c_int64(a["out_rs"]), None)


_BOTH = [
    # one case per rule
    (dict(P=48), UNSUPPORTED), (dict(P=256), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=0), UNSUPPORTED),
    (dict(cache=4096 + 8), UNSUPPORTED), (dict(out=(1 << 20) + 8), UNSUPPORTED),
    (dict(out_rs=580), UNSUPPORTED), (dict(out_rs=568), UNSUPPORTED), (dict(out_rs=-576), UNSUPPORTED),
    (dict(rows=2 ** 31 - 1), UNSUPPORTED), (dict(rows=2 ** 31 - 32), UNSUPPORTED), (dict(out_rs=1 << 40), UNSUPPORTED),
    (dict(out=0), INVALID), (dict(cache=0), INVALID), (dict(bid=0), INVALID), (dict(cu=0), INVALID),
    (dict(rows=-1), INVALID), (dict(num_req=-1), INVALID), (dict(max_blocks=-1), INVALID), (dict(num_blocks=-1), INVALID),
    # nothing to launch: 0 without a device call, null pointers included; seq_starts may always be null
    (dict(rows=0), 0), (dict(num_req=0), 0), (dict(rows=0, out=0, cache=0, bid=0, cu=0, st=0), 0), (dict(num_req=0, cu=0, bid=0), 0),
    (dict(rows=1, out_rs=0, num_req=0), 0),
]
_BF16 = [(dict(ts=568), UNSUPPORTED), (dict(ts=580), UNSUPPORTED), (dict(bs=64 * 576 + 4), UNSUPPORTED), (dict(bs=-64 * 576), INVALID),
         (dict(ts=1 << 56), UNSUPPORTED), (dict(bs=1 << 58), UNSUPPORTED), (dict(rows=0, ts=640, bs=67 * 640), 0)]
_FP8 = [(dict(ts=655), UNSUPPORTED), (dict(ts=664), UNSUPPORTED), (dict(ts=576), UNSUPPORTED), (dict(bs=64 * 656 + 8), UNSUPPORTED),
        (dict(bs=-64 * 656), INVALID), (dict(ts=1 << 56), UNSUPPORTED), (dict(bs=1 << 58), UNSUPPORTED),
        (dict(rows=0, ts=704, bs=67 * 704), 0)]
# The cache's rule (csrc/mla_cache.h), as the writer's and the decode's tables pin it: it holds for a call with nothing to launch
# too, and a negative block stride is an invalid argument that wins over whatever is merely unsupported.  Behind every case
# above, so that those keep their ids.
_CACHE_RULE = [(fp8, kw, c) for fp8, row, off in ((False, 576, 580), (True, 656, 664)) for kw, c in [
    (dict(ts=-row), UNSUPPORTED), (dict(rows=0, P=48), UNSUPPORTED), (dict(rows=0, ts=off), UNSUPPORTED),
    (dict(P=48, bs=-64 * row), INVALID)]]


@pytest.mark.parametrize("fp8,kwargs,code",
                         [(k, kw, c) for k in (False, True) for kw, c in _BOTH + (_FP8 if k else _BF16)] + _CACHE_RULE)
def test_cabi_refuses_on_the_host(fp8, kwargs, code):
    assert _launch(fp8, **kwargs) == code


# ---------------------------------------------------------------------------------------------------------- the planner
def _check_plan(lens, workspace):
    import hpc

    B = len(lens)
    plan = hpc.mla_context_chunks(lens, workspace)
    share = workspace // B // 128 * 128
    assert share >= 128 and share % 128 == 0
    assert len(plan) == -(-max(lens) // share)  # ceil(max L / share)
    covered = [0] * B
    for starts, cu, max_len in plan:
        assert starts.dtype == torch.int32 and cu.dtype == torch.int32 and starts.device.type == "cpu" and cu.device.type == "cpu"
        assert starts.shape == (B,) and cu.shape == (B + 1,) and isinstance(max_len, int)
        counts = (cu[1:] - cu[:-1]).tolist()
        assert int(cu[0]) == 0 and int(cu[-1]) <= workspace  # no pass exceeds the workspace
        assert max_len == max(counts) and max_len > 0 and all(0 <= c <= share for c in counts)
        for b in range(B):
            if counts[b]:
                assert int(starts[b]) == covered[b]  # in order, no gap, no overlap
                covered[b] += counts[b]
            else:
                assert covered[b] == lens[b]  # exhausted: 0 rows
    assert covered == list(lens)  # each [0, L_b) exactly once


def test_planner_properties():
    import hpc

    rng = random.Random(5)
    for _ in range(300):
        B = rng.randint(1, 12)
        lens = [rng.choice([0, 1, 127, 128, 129, rng.randint(0, 5000), rng.randint(0, 40000)]) for _ in range(B)]
        if max(lens) == 0:
            lens[rng.randrange(B)] = rng.randint(1, 3000)
        _check_plan(lens, rng.choice([128 * B, 128 * B + 127, rng.randint(128 * B, 40000 + 128 * B)]))
    assert hpc.mla_context_chunks([0, 0, 0], 4096) == [] and hpc.mla_context_chunks([], 4096) == []
    with pytest.raises(ValueError, match="below 128 rows"):
        hpc.mla_context_chunks([5, 9], 255)
    with pytest.raises(ValueError, match="negative"):
        hpc.mla_context_chunks([5, -1], 4096)
    _check_plan([0, 200, 700], 384)  # the end-to-end test's plan: share 128, six passes
    assert len(hpc.mla_context_chunks([0, 200, 700], 384)) == 6


# -------------------------------------------------------------------------------------------------- the cases have teeth
@functools.lru_cache(maxsize=None)
def _case(P, layout, fp8):
    c = gr.build_case(P, layout, fp8)
    before = torch.full((c.T, gr.WIDTH), gr.SENTINEL, dtype=torch.int16)
    return c, before, gr.gather_statement(c.cache, c.block_ids, c.cu_seqlens, c.seq_starts, out_bits=before)


@functools.lru_cache(maxsize=None)
def _guard_case(P, fp8, bad):
    bad = {"num_blocks": None, "-1": -1, "INT32_MAX": gr.INT32_MAX}[bad]
    c, zero_rows = gr.build_guard_case(P, fp8, 0)
    c.block_ids[0, 1] = c.num_blocks if bad is None else bad
    before = torch.full((c.T, gr.WIDTH), gr.SENTINEL, dtype=torch.int16)
    return c, zero_rows, before, gr.gather_statement(c.cache, c.block_ids, c.cu_seqlens, c.seq_starts, out_bits=before)


def _differs_in(c, want, got, which):
    """the requests among `which` (indices) in which `got` differs from `want` in at least one row"""
    cu = c.cu_seqlens.tolist()
    return {b for b in which if bool((want[cu[b]: cu[b + 1]] != got[cu[b]: cu[b + 1]]).any())}


def test_inputs_have_teeth():
    assert torch.equal(gr.dequantise_mutant(_case(16, "plain", True)[0].cache), f8.dequantise(_case(16, "plain", True)[0].cache))
    for P in PAGES:
        for layout in gr.LAYOUTS:
            for fp8 in (False, True):
                c, before, want = _case(P, layout, fp8)
                cu = c.cu_seqlens.tolist()
                assert bool((want[: cu[0]] == gr.SENTINEL).all()) and bool((want[cu[-1]:] == gr.SENTINEL).all())
                assert not bool((want[cu[0]: cu[-1]] == gr.SENTINEL).all(1).any())  # every owned row is written
                live = {b for b, (_, n) in enumerate(c.requests) if n > 0}
                touched = {
                    "ignore_starts": {b for b in live if c.requests[b][0] != 0},
                    "page_edge_off_by_one": {b for b in live if any((s + i) % P == P - 1 for s, n in [c.requests[b]] for i in range(n))},
                    "slot_is_row_offset": {b for b in live if c.requests[b][0] % P != 0},
                    "next_table_row": live,
                }
                if fp8:
                    touched.update(scale_shift=live, truncate=live, rope_at=live)
                for knob, which in touched.items():
                    assert which, (knob, P)  # the case exercises the knob at all
                    value = {"scale_shift": 1, "rope_at": 512}.get(knob, True)
                    got = gr.gather_statement(c.cache, c.block_ids, c.cu_seqlens, c.seq_starts, out_bits=before, **{knob: value})
                    assert _differs_in(c, want, got, which) == which, (knob, P, layout, fp8)
                for bad in ("num_blocks", "-1", "INT32_MAX"):
                    if layout != "plain":
                        continue
                    g, zero_rows, gbefore, gwant = _guard_case(P, fp8, bad)
                    assert zero_rows and not gwant[torch.tensor(zero_rows)].any()
                    others = sorted(set(range(g.cu_seqlens[0], g.cu_seqlens[-1])) - set(zero_rows))
                    assert bool(gwant[torch.tensor(others)].any(1).all())  # the neighbours hold data
                    got = gr.gather_statement(g.cache, g.block_ids, g.cu_seqlens, g.seq_starts, out_bits=gbefore, guard_unwritten=True)
                    assert bool((got[torch.tensor(zero_rows)] != gwant[torch.tensor(zero_rows)]).any(1).all())


# ---------------------------------------------------------------------------------------------------------------- GPU
def _op(fp8):
    import hpc

    return hpc.mla_gather_ckv_fp8 if fp8 else hpc.mla_gather_ckv


def _cache_on_gpu(c):
    alloc = c.alloc.cuda()
    view = gr.cache_view(alloc, c.P, c.layout, c.fp8)
    return alloc, (view if c.fp8 else view.view(BF16))


def _run_in_buffer(c):
    """the op into rows 3 .. 3 + T of a [T + 7, 640] buffer prefilled with the sentinel; returns (buffer before, buffer after)
    as int16 on the CPU, and checks that the cache allocation is unchanged"""
    buf = torch.full((c.T + 7, 640), gr.SENTINEL, dtype=torch.int16, device="cuda")
    before = buf.cpu()
    out = buf.view(BF16)[3: 3 + c.T, :gr.WIDTH]
    alloc, cache = _cache_on_gpu(c)
    got = _op(c.fp8)(cache, c.block_ids.cuda(), c.cu_seqlens.cuda(), seq_starts=c.seq_starts.cuda(), output=out)
    assert got is out
    torch.cuda.synchronize()
    assert torch.equal(alloc.cpu(), c.alloc)
    return before, buf.cpu()


def _assert_buffer(before, after, want, T):
    expect = before.clone()
    expect[3: 3 + T, :gr.WIDTH] = want
    bad = (after != expect)
    assert not bool(bad.any()), f"{int(bad.any(1).sum())} rows differ, first {int(bad.any(1).nonzero()[0])} (buffer row)"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", gr.LAYOUTS)
@pytest.mark.parametrize("P", PAGES)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_rows_are_the_statements_and_nothing_else_changes(fp8, P, layout):
    c, _, want = _case(P, layout, fp8)
    before, after = _run_in_buffer(c)
    _assert_buffer(before, after, want, c.T)


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_fresh_output_and_no_seq_starts(fp8):
    c, _, _ = _case(16, "padded", fp8)
    _, cache = _cache_on_gpu(c)
    y = _op(fp8)(cache, c.block_ids.cuda(), c.cu_seqlens.cuda(), num_rows=c.T)
    assert y.shape == (c.T, gr.WIDTH) and y.dtype == BF16 and y.is_contiguous()
    cu = c.cu_seqlens.tolist()
    want = gr.gather_statement(c.cache, c.block_ids, c.cu_seqlens, None, out_bits=torch.zeros(c.T, gr.WIDTH, dtype=torch.int16))
    assert torch.equal(y.view(torch.int16).cpu()[cu[0]: cu[-1]], want[cu[0]: cu[-1]])
    # nothing to launch
    assert _op(fp8)(cache, c.block_ids.cuda(), c.cu_seqlens.cuda(), num_rows=0).shape == (0, gr.WIDTH)
    empty = _op(fp8)(cache, c.block_ids.cuda()[:0], c.cu_seqlens.cuda()[:1], num_rows=4)
    assert empty.shape == (4, gr.WIDTH)
    with pytest.raises(RuntimeError, match="one of output and num_rows"):
        _op(fp8)(cache, c.block_ids.cuda(), c.cu_seqlens.cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["num_blocks", "-1", "INT32_MAX"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_rows_that_cannot_be_fetched_are_zeros(fp8, bad):
    c, zero_rows, _, want = _guard_case(16, fp8, bad)
    before, after = _run_in_buffer(c)
    _assert_buffer(before, after, want, c.T)
    rows = after[3: 3 + c.T, :gr.WIDTH]
    is_zero = ~rows.any(1)
    assert sorted(is_zero.nonzero().flatten().tolist()) == zero_rows  # exactly those rows


@pytest.mark.gpu
def test_cu_seqlens_that_do_not_ascend_write_only_rows_of_their_own_request():
    c, _, _ = _case(16, "plain", False)
    cu = torch.tensor([2, 40, 30, 30, 90, 60, 100], dtype=torch.int32)  # negative counts: empty requests
    st = c.seq_starts.clone()
    T = 110
    before = torch.full((T, gr.WIDTH), gr.SENTINEL, dtype=torch.int16)
    buf = before.cuda()
    _, cache = _cache_on_gpu(c)
    _op(False)(cache, c.block_ids.cuda(), cu.cuda(), seq_starts=st.cuda(), output=buf.view(BF16))
    got = buf.cpu()
    # whichever request the search lands on, a written row is that request's row under the statement, or untouched
    cul = cu.tolist()
    for r in range(T):
        if bool((got[r] == gr.SENTINEL).all()):
            continue
        owners = [b for b in range(6) if cul[b] <= r < cul[b + 1]]
        assert owners, r
        wants = []
        for b in owners:
            one_cu = torch.tensor([cul[b] if i <= b else cul[b + 1] for i in range(7)], dtype=torch.int32)
            wants.append(gr.gather_statement(c.cache, c.block_ids, one_cu, st, out_bits=before)[r])
        assert any(torch.equal(got[r], w) for w in wants), r


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_round_trip_with_the_writer(fp8):
    import hpc

    P, lens = 32, [70, 1, 0, 33]
    rows = sum(lens)
    g = torch.Generator().manual_seed(17)
    kv_a = torch.randn(rows, 576, generator=g).to(BF16).cuda()
    w = (1 + 0.1 * torch.randn(512, generator=g)).cuda()
    table = ms.cos_sin_table(128).cuda()
    nb = sum(-(-n // P) for n in lens) + 1
    bid = torch.full((len(lens), 4), -1, dtype=torch.int32)
    perm, o = torch.randperm(nb, generator=g).tolist(), 0
    for b, n in enumerate(lens):
        k = -(-n // P)
        bid[b, :k] = torch.tensor(perm[o: o + k], dtype=torch.int32)
        o += k
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32).cuda()
    seqlen = torch.tensor(lens, dtype=torch.int32).cuda()
    cache = torch.zeros(nb, P, 656 if fp8 else 576, dtype=torch.uint8 if fp8 else BF16, device="cuda")
    out_ckv = torch.empty(rows, 576, dtype=BF16, device="cuda")
    store = hpc.mla_rope_norm_store_kv_fp8 if fp8 else hpc.mla_rope_norm_store_kv
    store(cache, kv_a, table, w, seqlen, cu, bid.cuda(), out_ckv=out_ckv)
    got = _op(fp8)(cache, bid.cuda(), cu, num_rows=rows)
    want = f8.dequantise(f8.quantise(out_ckv.cpu())) if fp8 else out_ckv.cpu()
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_hipgraph_replay_follows_the_device_lengths(fp8):
    c, _, _ = _case(16, "pool", fp8)
    _, cache = _cache_on_gpu(c)
    bid, cu, st = c.block_ids.cuda(), c.cu_seqlens.cuda(), c.seq_starts.cuda()
    buf = torch.full((c.T, 640), gr.SENTINEL, dtype=torch.int16, device="cuda")
    out = buf.view(BF16)[:, :gr.WIDTH]
    op = _op(fp8)
    op(cache, bid, cu, seq_starts=st, output=out)  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        op(cache, bid, cu, seq_starts=st, output=out)
    # other lengths and starts within the pages each request holds
    new = [(0, 1), (0, 0), (2, 20), (1, 30), (7, 250), (0, 35)]
    ncu = [1]
    for _, n in new:
        ncu.append(ncu[-1] + n)
    new_cu, new_st = torch.tensor(ncu, dtype=torch.int32), torch.tensor([s for s, _ in new], dtype=torch.int32)
    assert ncu[-1] <= c.T
    cu.copy_(new_cu.cuda())
    st.copy_(new_st.cuda())
    buf.fill_(gr.SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    before = torch.full((c.T, gr.WIDTH), gr.SENTINEL, dtype=torch.int16)
    want = gr.gather_statement(c.cache, c.block_ids, new_cu, new_st, out_bits=before)
    assert not bool((want[ncu[0]: ncu[-1]] == gr.SENTINEL).all(1).any())
    assert torch.equal(buf.cpu()[:, :gr.WIDTH], want) and bool((buf.cpu()[:, gr.WIDTH:] == gr.SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_far_pool_offsets_are_64_bit(fp8):
    """page 2 of the view lies more than 4 GiB behind the base: a 32-bit page offset would read page 0's neighbourhood"""
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip("needs 16 GiB of free device memory")
    P, row, elem = 16, (656 if fp8 else 576), (1 if fp8 else 2)
    block_bytes = 2 ** 31 + 2 ** 28  # 2.25 GiB: page 2 starts at 4.5 GiB
    pool = torch.empty(3 * block_bytes // elem, dtype=torch.uint8 if fp8 else torch.int16, device="cuda")
    cache = pool.as_strided((3, P, row), (block_bytes // elem, row, 1))
    g = torch.Generator().manual_seed(23)
    if fp8:
        pages = f8.quantise(torch.randn(3, P, 576, generator=g).to(BF16), vary_seed=5)
    else:
        pages = torch.randint(-2 ** 15, 2 ** 15, (3, P, row), generator=g, dtype=torch.int32).to(torch.int16)
    for p in range(3):
        cache[p].copy_(pages[p].cuda())
    bid = torch.tensor([[2], [0], [1]], dtype=torch.int32)
    cu, st = torch.tensor([0, 1, 2, 3], dtype=torch.int32), torch.tensor([7, 0, 15], dtype=torch.int32)
    got = _op(fp8)(cache if fp8 else cache.view(BF16), bid.cuda(), cu.cuda(), seq_starts=st.cuda(), num_rows=3)
    want = gr.gather_statement(pages if fp8 else pages.view(BF16), bid, cu, st, out_bits=torch.zeros(3, 576, dtype=torch.int16))
    assert torch.equal(got.cpu().view(torch.int16), want)
    del pool, cache
