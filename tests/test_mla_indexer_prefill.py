"""hpc.mla_indexer_logits_prefill_fp8 / mla_indexer_topk_prefill / mla_indexer_topk_prefill_fp8: the DSA indexer over a ragged
prefill chunk.

The statement is the decode statement on the expanded form (tests/mla_indexer_prefill_ref.py).  One small case throughout: nine
requests with 1 .. 70 new rows over 0 .. 2100 cached tokens, a request shorter than its rows, one without rows, three pad rows -
161 rows by about 2,200 columns, across the 512-token chunk edge and on both sides of topk.
CPU: the expanded statement against a brute-force loop; the mutants of the row rule unequal to it on the exact inputs; surface
and fakes; the plan against the route restated; refusals through the C-ABI with never-dereferenced pointers; empty chunks.
GPU: logits EQUAL to the statement on exact inputs, bit-identical to hpc.mla_indexer_logits_fp8 on the expanded form on random
ones (hence within that op's C_BAR), repeatable, row windows, guard bands; top-k equal to the statement and to hpc.mla_indexer_topk
on the expanded form; the fused call bit-identical to its parts for any slab; end to end and graph replay are in
tests/test_attention_prefill_mla_sparse.py."""
import ctypes
import functools
from ctypes import c_int, c_int64, c_void_p
from pathlib import Path

import pytest
import torch

import mla_indexer_prefill_ref as pr
import mla_indexer_ref as ir

UNSUPPORTED, INVALID = -1, -2
MAX_TOPK = 65536
C_BAR = 1024  # the logits bar of tests/test_mla_indexer.py (derived there): |op - statement| <= C_BAR * 2^-24 * A
TILE = 16
SCRATCH_BUDGET = 256 << 20


@functools.lru_cache(maxsize=None)
def _case(i, exact):
    """(inputs, the statement float64 with NaN where nothing is written) of one configuration - computed once"""
    Hi, P = pr.CONFIGS[i]
    inp = pr.inputs(Hi, P, exact=exact)
    return inp, pr.logits_statement(inp)


# ---- CPU 1: the statement --------------------------------------------------------------------------------------------------------
def test_the_case_reaches_every_edge():
    inp, want = _case(0, True)
    assert inp["T"] == 161 and want.shape == (161, 134 * 16) and _case(2, True)[1].shape == (161, 35 * 64)
    rows = [pr.row_rule(inp["lens_total"], inp["q_index"], r) for r in range(inp["T"])]
    assert [r for r, (_, _, live) in enumerate(rows) if not live] == [154, 155, 158, 159, 160]  # pos < 0 twice, three pad rows
    assert rows[0] == (0, 0, True) and rows[1] == (1, 5, True) and rows[3][0] == 2 and rows[156] == (8, 0, True)
    assert 7 not in {b for b, _, _ in rows}  # the request without rows owns none
    vis = [pos + 1 if live else 0 for _, pos, live in rows]
    assert min(v for v in vis if v) == 1 and max(vis) == 2117 and any(v <= 64 for v in vis) and any(v > 2048 for v in vis)
    assert any(0 < v <= 512 for v in vis) and any(v > 512 for v in vis)  # rows on both sides of the 512-token chunk edge
    assert len(inp["dead"]) == 9 and inp["block_ids"].shape[1] == 134


def test_expanded_statement_against_a_brute_force_loop():
    """every row of the chunk, a sample of its columns: the formula by a loop over heads, the written set from the row rule
    restated with a linear scan"""
    inp, want = _case(0, False)
    codes, scales = ir.unpack(inp["k_cache"])
    P, nb = inp["P"], codes.shape[0]
    qi, L = inp["q_index"].tolist(), inp["lens_total"].tolist()
    g = torch.Generator().manual_seed(1)
    for r in range(inp["T"]):
        owner = [b for b in range(len(L)) if qi[b] <= r < qi[b + 1]]
        vis = max(L[owner[0]] - (qi[owner[0] + 1] - r) + 1, 0) if owner else 0
        assert bool(want[r, vis:].isnan().all()) and not bool(want[r, :vis].isnan().any()), r
        for j in ([0, vis - 1] + torch.randint(0, max(vis, 1), (3,), generator=g).tolist() if vis else []):
            page = int(inp["block_ids"][owner[0], j // P])
            if not 0 <= page < nb:
                assert want[r, j] == float("-inf"), (r, j)
                continue
            tot = 0.0
            for h in range(inp["Hi"]):
                dot = float(inp["q"][r, h].double() @ codes[page, j % P].double())
                tot += float(inp["weights"][r, h]) * max(dot, 0.0)
            ref = float(scales[page, j % P]) * tot
            assert abs(float(want[r, j]) - ref) <= 1e-9 * (1 + abs(ref)), (r, j)


@pytest.mark.parametrize("i", range(len(pr.CONFIGS)))
def test_row_rule_mutants_differ_on_the_exact_inputs(i):
    """each mutant of the row rule, run through the statement, is unequal to the statement on the exact inputs - as logits and as
    top-k lists - on the window the GPU tests use (rows 37 ..): the case has teeth"""
    inp, _ = _case(i, True)
    rb = 37
    want = pr.logits_statement(inp, rb)
    lists = pr.topk_statement(want.float(), inp, 64, rb)
    for name, mutation in pr.ROW_RULE_MUTANTS.items():
        got = pr.logits_statement(inp, rb, **mutation)
        assert not ir.equal_where_written(got.float(), want), (pr.CONFIGS[i], name)
        assert not torch.equal(pr.topk_statement(want.float(), inp, 64, rb, **mutation), lists), (pr.CONFIGS[i], name)
    assert ir.equal_where_written(want.float(), want)


# ---- CPU 2: surface and fakes ------------------------------------------------------------------------------------------------------
NAMES = ("mla_indexer_logits_prefill_fp8", "mla_indexer_topk_prefill", "mla_indexer_topk_prefill_fp8")


def test_surface():
    import hpc

    for name in NAMES:
        assert name in hpc.__all__ and callable(getattr(hpc, name)), name
        assert hasattr(torch.ops.hpc_mla, name), name
    doc = hpc.mla_indexer_logits_prefill_fp8.__doc__
    for word in ("tests/mla_indexer_prefill_ref.py", "q_index[b] <= r", "num_seqlen_per_req[b] - (q_index[b + 1] - r)", "row_begin",
                 "row of no request", "NOT written", "-inf", "{16, 32, 64}", "once per 16 rows", "hipGraph", "bit-identical",
                 "No float", "expanded form"):
        assert word in doc, word
    doc = hpc.mla_indexer_topk_prefill.__doc__
    for word in ("ASCENDING", "smaller position", "identity list", "all -1", "1..65536", "never read", "hipGraph"):
        assert word in doc, word
    doc = hpc.mla_indexer_topk_prefill_fp8.__doc__
    for word in ("release_decode_workspaces", "bit-identical", "hipGraph", "scratch_rows", "256 MiB", "does not grow with T"):
        assert word in doc, word


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        q = torch.empty(50, 32, 128, dtype=ir.F8, device="cuda")
        w = torch.empty(50, 32, dtype=torch.float32, device="cuda")
        cache = torch.empty(9, 64 * 132, dtype=torch.uint8, device="cuda")
        bid = torch.empty(3, 5, dtype=torch.int32, device="cuda")
        lens = torch.empty(3, dtype=torch.int32, device="cuda")
        qi = torch.empty(4, dtype=torch.int32, device="cuda")
        y = hpc.mla_indexer_logits_prefill_fp8(q, w, cache, bid, lens, qi, row_begin=16)
        assert (y.shape, y.dtype, y.device.type) == ((50, 5 * 64), torch.float32, "cuda")
        o = torch.empty(50, 320, dtype=torch.float32, device="cuda")
        assert hpc.mla_indexer_logits_prefill_fp8(q, w, cache, bid, lens, qi, output=o) is o
        t = hpc.mla_indexer_topk_prefill(y, lens, qi, 100, row_begin=16)
        assert (t.shape, t.dtype, t.device.type) == ((50, 100), torch.int32, "cuda")
        oi = torch.empty(50, 100, dtype=torch.int32, device="cuda")
        assert hpc.mla_indexer_topk_prefill(y, lens, qi, 100, output=oi) is oi
        t = hpc.mla_indexer_topk_prefill_fp8(q, w, cache, bid, lens, qi, 2048, scratch_rows=16)
        assert (t.shape, t.dtype) == ((50, 2048), torch.int32)
        assert hpc.mla_indexer_topk_prefill_fp8(q, w, cache, bid, lens, qi, 100, output=oi) is oi


# ---- CPU 3: the route and the C-ABI ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def plan(lib, R, req, Hi, P, max_blocks, topk, scratch_rows, cus):
    tile, grid, chunk, slab, slabs, rs, ws = (c_int(-7), c_int(-7), c_int(-7), c_int(-7), c_int(-7), c_int64(-7), c_int64(-7))
    rc = lib.hpc_mla_indexer_prefill_plan(R, req, Hi, P, max_blocks, topk, scratch_rows, cus, *(ctypes.byref(v) for v in
                                                                                                  (tile, grid, chunk, slab, slabs, rs, ws)))
    return rc, tile.value, grid.value, chunk.value, slab.value, slabs.value, rs.value, ws.value


def _route(R, req, P, max_blocks, topk, scratch_rows, cus):
    """the arithmetic of csrc/mla_indexer_route.h::mla_indexer_prefill_route, restated: (tile, logits grid, chunk, slab rows,
    slabs, scratch row stride, scratch bytes)"""
    cols = max_blocks * P
    if topk == 0:  # a logits call: one launch over all rows, no scratch
        slab = R
    else:
        slab = scratch_rows if scratch_rows > 0 else max(SCRATCH_BUDGET // 4 // max(cols, 1) // TILE * TILE, TILE)
        slab = min(slab, R)
    call_tiles, chunk = -(-slab // TILE), 512
    while chunk < 8192 and call_tiles * -(-cols // chunk) > 16 * cus:
        chunk *= 2
    grid = -(-R // TILE) * -(-cols // chunk) if req > 0 else 0
    return TILE, grid, chunk, slab, (-(-R // slab) if slab else 0), cols, (slab * cols * 4 if topk else 0)


@pytest.mark.parametrize("R,req,Hi,P,max_blocks,cus", [(4096, 1, 64, 64, 64, 256), (16384, 4, 64, 64, 64, 256), (4096, 1, 64, 64, 512, 256),
                                                       (161, 9, 16, 16, 134, 304), (8000, 64, 32, 128, 260, 80), (1, 1, 64, 32, 1, 64),
                                                       (100000, 7, 64, 64, 2048, 256), (0, 3, 64, 64, 128, 256), (50, 0, 16, 16, 8, 256),
                                                       (33, 2, 16, 16, 0, 256)])
def test_plan_is_the_route(lib, R, req, Hi, P, max_blocks, cus):
    for topk, scratch_rows in ((0, 0), (1, 0), (2048, 0), (MAX_TOPK, 16), (2048, 50), (64, 1 << 20)):
        assert plan(lib, R, req, Hi, P, max_blocks, topk, scratch_rows, cus) == (0,) + _route(R, req, P, max_blocks, topk, scratch_rows, cus), \
            (topk, scratch_rows)


def test_plan_examples(lib):
    # one fresh 4096-token prompt: 256 row tiles by 8 chunks of 512 columns; the whole chunk's logits fit the budget
    assert plan(lib, 4096, 1, 64, 64, 64, 2048, 0, 256)[1:6] == (16, 256 * 8, 512, 4096, 1)
    # a caller's slab whose logits would pass 2^40 bytes is refused, whatever the chunk has
    assert plan(lib, 4096, 1, 64, 64, 1 << 24, 64, 4096, 256)[0] == UNSUPPORTED
    assert plan(lib, 4096, 1, 64, 64, 1 << 24, 64, 256, 256)[0] == 0
    # over a 32k-token table a slab is 2048 rows: the scratch is the budget, whatever the chunk
    assert plan(lib, 4096, 1, 64, 64, 512, 2048, 0, 256)[4:] == (2048, 2, 512 * 64, SCRATCH_BUDGET)
    assert plan(lib, 65536, 1, 64, 64, 512, 2048, 0, 256)[4:] == (2048, 32, 512 * 64, SCRATCH_BUDGET)
    ok = (161, 9, 64, 64, 35, 64, 0, 256)
    assert plan(lib, *ok)[0] == 0
    for i, bad, code in ((0, -1, INVALID), (1, -1, INVALID), (2, 48, UNSUPPORTED), (2, 128, UNSUPPORTED), (3, 48, UNSUPPORTED),
                         (3, 256, UNSUPPORTED), (4, -1, INVALID), (4, 1 << 26, UNSUPPORTED), (5, -1, UNSUPPORTED),
                         (5, MAX_TOPK + 1, UNSUPPORTED), (6, -1, INVALID)):
        args = list(ok)
        args[i] = bad
        assert plan(lib, *args)[0] == code, (i, bad)


def _ip(v):
    return ctypes.cast(c_void_p(v), ctypes.POINTER(c_int)) if v else None


def _vp(v):
    return c_void_p(v) if v else None


def call_logits(lib, *, out=4096, q=4096, w=4096, cache=4096, bid=4096, lens=4096, qi=4096, R=40, req=2, rb=0, Hi=64, P=64,
                max_blocks=4, num_blocks=8, block_stride=None, row_stride=None, refusal=False):
    bs = P * 132 if block_stride is None else block_stride
    rs = max_blocks * P if row_stride is None else row_stride
    args = (_vp(out), _vp(q), _vp(w), _vp(cache), _ip(bid), _ip(lens), _ip(qi), R, req, rb, Hi, P, max_blocks, num_blocks, c_int64(bs),
            c_int64(rs))
    if refusal:
        return lib.hpc_mla_indexer_logits_prefill_fp8_refusal(*args)
    return lib.hpc_mla_indexer_logits_prefill_fp8_async(*args, None)


def call_topk(lib, *, out=4096, logits=4096, lens=4096, qi=4096, R=40, req=2, rb=0, cols=256, topk=64, row_stride=None, refusal=False):
    rs = cols if row_stride is None else row_stride
    args = (_vp(out), _vp(logits), _ip(lens), _ip(qi), R, req, rb, c_int64(cols), topk, c_int64(rs))
    if refusal:
        return lib.hpc_mla_indexer_topk_prefill_refusal(*args)
    return lib.hpc_mla_indexer_topk_prefill_async(*args, None)


def call_fused(lib, *, out=4096, q=4096, w=4096, cache=4096, bid=4096, lens=4096, qi=4096, R=40, req=2, Hi=64, P=64, max_blocks=4,
               num_blocks=8, block_stride=None, topk=64, scratch_rows=0, ws=4096, ws_bytes=1 << 30, refusal=False):
    bs = P * 132 if block_stride is None else block_stride
    args = (_vp(out), _vp(q), _vp(w), _vp(cache), _ip(bid), _ip(lens), _ip(qi), R, req, Hi, P, max_blocks, num_blocks, c_int64(bs),
            topk, scratch_rows, _vp(ws), c_int64(ws_bytes))
    if refusal:
        return lib.hpc_mla_indexer_topk_prefill_fp8_refusal(*args)
    return lib.hpc_mla_indexer_topk_prefill_fp8_async(*args, None)


_CACHE_REFUSALS = [(dict(P=48), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=256), UNSUPPORTED), (dict(P=0), UNSUPPORTED),
                   (dict(block_stride=64 * 132 - 16), UNSUPPORTED), (dict(block_stride=64 * 132 + 8), UNSUPPORTED),
                   (dict(block_stride=-64 * 132), INVALID), (dict(cache=4096 + 8), UNSUPPORTED), (dict(cache=0), INVALID),
                   (dict(out=0), INVALID)]
_READER_REFUSALS = [(dict(Hi=8), UNSUPPORTED), (dict(Hi=48), UNSUPPORTED), (dict(Hi=128), UNSUPPORTED), (dict(R=-1), INVALID),
                    (dict(req=-1), INVALID), (dict(max_blocks=-1), INVALID), (dict(max_blocks=0), INVALID),
                    (dict(max_blocks=1 << 26), UNSUPPORTED), (dict(num_blocks=-1), INVALID), (dict(q=0), INVALID), (dict(w=0), INVALID),
                    (dict(bid=0), INVALID), (dict(lens=0), INVALID), (dict(qi=0), INVALID), (dict(q=4096 + 8), UNSUPPORTED),
                    (dict(w=4096 + 4), UNSUPPORTED), (dict(R=0, P=48), UNSUPPORTED), (dict(req=0, Hi=24), UNSUPPORTED)]
_TOPK_REFUSALS = [(dict(topk=0), UNSUPPORTED), (dict(topk=-1), UNSUPPORTED), (dict(topk=MAX_TOPK + 1), UNSUPPORTED)]


def _refusal_agrees(fn, lib, kwargs, code):
    """the launcher's code, and the same call's refusal in words: a message exactly when the call is refused.  The pointers are
    never dereferenced: a refused call reaches no device call"""
    assert fn(lib, **kwargs) == code, kwargs
    why = fn(lib, refusal=True, **kwargs)
    assert (why is None) == (code == 0), (kwargs, why)
    assert why is None or len(why.decode()) > 10


@pytest.mark.parametrize("kwargs,code", _CACHE_REFUSALS + _READER_REFUSALS + [
    (dict(row_stride=255), UNSUPPORTED), (dict(out=4096 + 2), UNSUPPORTED), (dict(rb=-1), INVALID), (dict(rb=2 ** 31 - 41), UNSUPPORTED)])
def test_logits_cabi_refuses_on_the_host(lib, kwargs, code):
    _refusal_agrees(call_logits, lib, kwargs, code)


@pytest.mark.parametrize("kwargs,code", _CACHE_REFUSALS + _READER_REFUSALS + _TOPK_REFUSALS + [
    (dict(ws=0), INVALID), (dict(ws_bytes=40 * 256 * 4 - 1), INVALID), (dict(scratch_rows=16, ws_bytes=16 * 256 * 4 - 1), INVALID),
    (dict(ws=4096 + 2), UNSUPPORTED), (dict(scratch_rows=-1), INVALID)])
def test_fused_cabi_refuses_on_the_host(lib, kwargs, code):
    _refusal_agrees(call_fused, lib, kwargs, code)


@pytest.mark.parametrize("kwargs,code", _TOPK_REFUSALS + [
    (dict(R=-1), INVALID), (dict(req=-1), INVALID), (dict(rb=-1), INVALID), (dict(cols=-1), INVALID), (dict(cols=(1 << 30) + 1), UNSUPPORTED),
    (dict(out=0), INVALID), (dict(logits=0), INVALID), (dict(lens=0), INVALID), (dict(qi=0), INVALID), (dict(row_stride=255), UNSUPPORTED),
    (dict(out=4096 + 2), UNSUPPORTED), (dict(logits=4096 + 1), UNSUPPORTED), (dict(R=0, topk=0), UNSUPPORTED),
    (dict(rb=2 ** 31 - 40), UNSUPPORTED)])
def test_topk_cabi_refuses_on_the_host(lib, kwargs, code):
    _refusal_agrees(call_topk, lib, kwargs, code)


def test_empty_chunks_launch_nothing(lib):
    """accepted up to the device call: no rows, or no requests, returns 0 without one (the pointers point nowhere)"""
    for empty in (dict(R=0), dict(req=0), dict(R=0, req=0)):
        for kw in (dict(), dict(P=16), dict(block_stride=64 * 132 + 16), dict(Hi=16)):
            _refusal_agrees(call_logits, lib, dict(empty, **kw), 0)
            _refusal_agrees(call_fused, lib, dict(empty, ws=0, ws_bytes=0, **kw), 0)
        for kw in (dict(), dict(topk=1), dict(topk=MAX_TOPK), dict(cols=0), dict(rb=5)):
            _refusal_agrees(call_topk, lib, dict(empty, **kw), 0)
        _refusal_agrees(call_logits, lib, dict(empty, out=0, q=0, w=0, cache=0, bid=0, lens=0, qi=0), 0)
    # calls with work that every host check accepts are refused by nothing (no launch is made here: the words only)
    for fn in (call_logits, call_fused, call_topk):
        assert fn(lib, refusal=True) is None
    assert call_fused(lib, refusal=True, scratch_rows=16, ws_bytes=16 * 256 * 4) is None
    assert call_logits(lib, refusal=True, rb=37) is None


def test_both_libraries_export_the_launchers():
    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for name in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        so = ctypes.CDLL(str(pkg / name))
        for op in ("logits_prefill_fp8", "topk_prefill", "topk_prefill_fp8"):
            for kind in ("async", "refusal"):
                assert hasattr(so, f"hpc_mla_indexer_{op}_{kind}"), (name, op, kind)
        assert hasattr(so, "hpc_mla_indexer_prefill_plan"), name
        for kind in ("bf16", "fp8"):
            assert hasattr(so, f"hpc_attention_prefill_mla_sparse_{kind}_async"), (name, kind)


# ---- GPU: the logits ---------------------------------------------------------------------------------------------------------------
def _chunk(inp):
    return (inp["k_cache"].cuda(), inp["block_ids"].cuda(), inp["lens_total"].cuda(), inp["q_index"].cuda())


def _logits(inp, row_begin=0, num_rows=None, **kw):
    import hpc

    R = inp["T"] - row_begin if num_rows is None else num_rows
    return hpc.mla_indexer_logits_prefill_fp8(inp["q"][row_begin: row_begin + R].cuda(), inp["weights"][row_begin: row_begin + R].cuda(),
                                              *_chunk(inp), row_begin=row_begin, **kw)


def _nan_output(inp, rows=None):
    cols = inp["block_ids"].shape[1] * inp["P"]
    return torch.full((inp["T"] if rows is None else rows, cols), float("nan"), dtype=torch.float32, device="cuda")


def _expanded(inp):
    """the expanded form on the GPU: (block_ids [T, max_blocks], lengths [T])"""
    bid, lens, _ = pr.expand(inp["block_ids"], inp["lens_total"], inp["q_index"], inp["T"])
    return bid.cuda(), lens.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(pr.CONFIGS)))
def test_logits_equal_the_statement_on_exact_inputs(i):
    """integer codes, integer weights, power-of-two scales: the result must EQUAL the float64 statement where written; the
    unwritten columns - past vis, and every column of a row of no request - still hold NaN; -inf exactly on the poisoned pages"""
    inp, want = _case(i, True)
    out = _nan_output(inp)
    assert _logits(inp, output=out) is out
    assert ir.equal_where_written(out, want), pr.CONFIGS[i]
    assert bool(out[[154, 155, 158, 159, 160]].isnan().all())
    P = inp["P"]
    bid, lens, req = pr.expand(inp["block_ids"], inp["lens_total"], inp["q_index"], inp["T"])
    dead = dict(inp["dead"])
    got = out.cpu()
    for r in range(inp["T"]):
        n = int(lens[r])
        mark = torch.zeros(n, dtype=torch.bool)
        slot = dead[int(req[r])]
        mark[slot * P: (slot + 1) * P] = True
        assert torch.equal(got[r, :n] == float("-inf"), mark), r
    # a fresh output: the written columns are the same
    fresh = _logits(inp).cpu()
    m = ~want.isnan()
    assert torch.equal(fresh[m], got[m])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(pr.CONFIGS)))
def test_logits_are_the_decode_ops_bits_on_random_inputs(i):
    """random e4m3 codes, scales in [2^-6, 2^-2], signed normal weights: bit-identical to hpc.mla_indexer_logits_fp8 on the
    expanded form with the same written set, hence within that op's bar C_BAR * 2^-24 * A of the statement - both asserted;
    and the same bits on repeated calls"""
    import hpc

    inp, want = _case(i, False)
    out = _nan_output(inp)
    _logits(inp, output=out)
    bid, lens = _expanded(inp)
    ref = _nan_output(inp)
    hpc.mla_indexer_logits_fp8(inp["q"].cuda(), inp["weights"].cuda(), inp["k_cache"].cuda(), bid, lens, mtp=0, new_kv_included=True,
                               output=ref)
    assert torch.equal(out.isnan(), ref.isnan())
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), pr.CONFIGS[i]
    ratio = ir.worst_ratio(out, want, pr.absolute_statement(inp))
    print(f"\nmla_indexer_logits_prefill_fp8 {pr.CONFIGS[i]}: worst err / (2^-24 A) = {ratio:.3f} (bar {C_BAR})")
    assert ratio <= C_BAR, (pr.CONFIGS[i], ratio)
    for _ in range(3):
        again = _nan_output(inp)
        _logits(inp, output=again)
        assert torch.equal(again.view(torch.int32), out.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("i", [1, 2])
def test_row_windows_equal_the_rows_of_the_full_call(i):
    """q and weights of rows row_begin .. with row_begin = 0, 16, 37: the matching rows of the full call, bit for bit, unwritten
    columns included; tiles are cut from the window's rows, so 37 moves every tile edge"""
    inp, _ = _case(i, False)
    full = _nan_output(inp)
    _logits(inp, output=full)
    for rb, rows in ((0, 50), (16, 100), (37, inp["T"] - 37), (37, 1), (150, 11)):
        win = _nan_output(inp, rows)
        _logits(inp, rb, rows, output=win)
        assert torch.equal(win.view(torch.int32), full[rb: rb + rows].view(torch.int32)), (rb, rows)


GUARD = 1 << 20


@pytest.mark.gpu
def test_logits_guard_bands_through_the_cabi(lib):
    """a logits buffer of exactly rows x row stride floats between 1 MiB guard bands, the row stride wider than the columns: the
    bands, the gap behind every row and the unwritten columns still hold their NaN afterwards"""
    inp, want = _case(1, True)
    q, w = inp["q"].cuda(), inp["weights"].cuda()
    cache, bid, lens, qi = _chunk(inp)
    rows, cols = want.shape
    rs = cols + 24
    buf = torch.full((2 * GUARD + rows * rs * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = call_logits(lib, out=buf.data_ptr() + GUARD, q=q.data_ptr(), w=w.data_ptr(), cache=cache.data_ptr(), bid=bid.data_ptr(),
                     lens=lens.data_ptr(), qi=qi.data_ptr(), R=rows, req=len(lens), Hi=inp["Hi"], P=inp["P"], max_blocks=bid.shape[1],
                     num_blocks=cache.shape[0], block_stride=cache.stride(0), row_stride=rs)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + rows * rs * 4:] == 0xFF).all())
    body = buf[GUARD: GUARD + rows * rs * 4].view(torch.float32).reshape(rows, rs)
    assert bool((body[:, cols:].contiguous().view(torch.int32) == -1).all())
    assert ir.equal_where_written(body[:, :cols], want)


# ---- GPU: the top-k ----------------------------------------------------------------------------------------------------------------
def _planted(inp, topk, g):
    """logits [T, columns] for the case's rows: rows that see more than topk tokens hold random values with many ties, zeros of
    both signs, -inf runs, NaN and +inf inside, and ties planted on the threshold; the rest of every row, and the whole of a row
    with n_r <= topk, is NaN and +inf that must never be read or chosen"""
    _, lens, _ = pr.expand(inp["block_ids"], inp["lens_total"], inp["q_index"], inp["T"])
    cols = inp["block_ids"].shape[1] * inp["P"]
    x = torch.full((inp["T"], cols), float("nan"))
    x[:, 1::2] = float("inf")
    for r, n in enumerate(lens.tolist()):
        if n <= topk:
            continue
        v = torch.randn(n, generator=g)
        v[torch.rand(n, generator=g) < 0.5] = 0.375  # one value on half of the row: the threshold sits in a run of ties
        v = torch.where(torch.rand(n, generator=g) < 0.3, (v * 4).round() / 4, v)
        v[torch.rand(n, generator=g) < 0.05] = 0.0
        v[torch.rand(n, generator=g) < 0.05] = -0.0
        for start in torch.randint(0, n, (3,), generator=g).tolist():
            v[start: start + 19] = float("-inf")
        v[torch.randint(0, n, (2,), generator=g)] = float("nan")
        v[torch.randint(0, n, (2,), generator=g)] = float("inf")
        x[r, :n] = v
    return x, lens


@pytest.mark.gpu
@pytest.mark.parametrize("topk", [1, 64, 65, 1000, 2048])
def test_topk_is_the_statement_and_the_decode_op_on_the_expanded_form(topk):
    import hpc

    inp, _ = _case(2, True)
    logits, lens = _planted(inp, topk, torch.Generator().manual_seed(topk))
    assert int((lens > topk).sum()) > 0 and int((lens <= topk).sum()) > 5
    want = pr.topk_statement(logits, inp, topk)
    assert bool((want[[154, 155, 158, 159, 160]] == -1).all())
    out = torch.full((inp["T"], topk), -7, dtype=torch.int32, device="cuda")
    dev = logits.cuda()
    assert hpc.mla_indexer_topk_prefill(dev, inp["lens_total"].cuda(), inp["q_index"].cuda(), topk, output=out) is out
    assert torch.equal(out.cpu(), want), [r for r in range(inp["T"]) if not torch.equal(out[r].cpu(), want[r])]
    assert torch.equal(out, hpc.mla_indexer_topk(dev, lens.cuda(), topk, mtp=0, new_kv_included=True))
    # a window of rows, a strided logits view and a fresh output
    wide = torch.full((inp["T"], logits.shape[1] + 8), float("inf"), device="cuda")
    wide[:, : logits.shape[1]] = dev
    got = hpc.mla_indexer_topk_prefill(wide[37:150, : logits.shape[1]], inp["lens_total"].cuda(), inp["q_index"].cuda(), topk, row_begin=37)
    assert torch.equal(got.cpu(), want[37:150])


# ---- GPU: the fused call -----------------------------------------------------------------------------------------------------------
def _fill_scratch_with_nan():
    for ws in torch.ops.hpc_mla._mla_indexer_prefill_workspaces():
        ws.fill_(0xFF)  # every float of it a NaN


def _fused(inp, topk, **kw):
    import hpc

    return hpc.mla_indexer_topk_prefill_fp8(inp["q"].cuda(), inp["weights"].cuda(), *_chunk(inp), topk, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("i,exact,topk", [(0, False, 64), (1, True, 65), (2, False, 1000), (3, True, 2048)])
def test_fused_is_its_two_parts_bit_for_bit_for_any_slab(i, exact, topk):
    import hpc

    inp, want = _case(i, exact)
    parts = hpc.mla_indexer_topk_prefill(_logits(inp, output=_nan_output(inp)), inp["lens_total"].cuda(), inp["q_index"].cuda(), topk)
    cols = want.shape[1]
    for scratch_rows in (0, 16, 50):  # one slab; eleven; four with a partial last one
        hpc.release_decode_workspaces()
        _fused(inp, topk, scratch_rows=scratch_rows)  # the scratch exists
        ws = torch.ops.hpc_mla._mla_indexer_prefill_workspaces()
        assert len(ws) == 1 and ws[0].numel() == (scratch_rows or inp["T"]) * cols * 4
        for _ in range(3):
            _fill_scratch_with_nan()
            assert torch.equal(_fused(inp, topk, scratch_rows=scratch_rows), parts), scratch_rows
    if exact:  # and the statement's list, through the statement's logits
        assert torch.equal(parts.cpu(), pr.topk_statement(want.float(), inp, topk))
    hpc.release_decode_workspaces()
    assert len(torch.ops.hpc_mla._mla_indexer_prefill_workspaces()) == 0


@pytest.mark.gpu
def test_empty_chunks_and_refusals():
    import hpc

    cache = torch.zeros(2, 64 * 132, dtype=torch.uint8, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    q0, w0 = torch.empty(0, 64, 128, device="cuda").to(ir.F8), torch.empty(0, 64, device="cuda")
    one = (torch.zeros(1, 1, **i32), torch.ones(1, **i32), torch.tensor([0, 1], **i32))
    none = (torch.empty(0, 3, **i32), torch.empty(0, **i32), torch.zeros(1, **i32))
    assert hpc.mla_indexer_logits_prefill_fp8(q0, w0, cache, *one).shape == (0, 64)
    assert hpc.mla_indexer_topk_prefill_fp8(q0, w0, cache, *one, 64).shape == (0, 64)
    q, w = torch.zeros(5, 64, 128, device="cuda").to(ir.F8), torch.zeros(5, 64, device="cuda")
    out = torch.full((5, 192), float("nan"), device="cuda")
    assert bool(hpc.mla_indexer_logits_prefill_fp8(q, w, cache, *none, output=out).isnan().all())  # no request: nothing written
    assert bool((hpc.mla_indexer_topk_prefill_fp8(q, w, cache, *none, 8) == -1).all())
    assert bool((hpc.mla_indexer_topk_prefill(out, none[1], none[2], 8) == -1).all())
    with pytest.raises(RuntimeError, match="q dtype must be float8_e4m3fn"):
        hpc.mla_indexer_logits_prefill_fp8(q.view(torch.uint8), w, cache, *one)
    with pytest.raises(RuntimeError, match="index head count"):
        hpc.mla_indexer_logits_prefill_fp8(q[:, :24].contiguous(), w[:, :24].contiguous(), cache, *one)
    with pytest.raises(RuntimeError, match="block_size"):
        hpc.mla_indexer_logits_prefill_fp8(q, w, cache[:, : 48 * 132], *one)
    with pytest.raises(RuntimeError, match="q_index must be"):
        hpc.mla_indexer_logits_prefill_fp8(q, w, cache, one[0], one[1], one[2][:1])
    with pytest.raises(RuntimeError, match="row_begin"):
        hpc.mla_indexer_logits_prefill_fp8(q, w, cache, *one, row_begin=-1)
    with pytest.raises(RuntimeError, match="scratch_rows"):
        hpc.mla_indexer_topk_prefill_fp8(q, w, cache, *one, 8, scratch_rows=-1)
    for bad in (0, MAX_TOPK + 1):
        with pytest.raises(RuntimeError, match="topk"):
            hpc.mla_indexer_topk_prefill_fp8(q, w, cache, *one, bad)
        with pytest.raises(RuntimeError, match="topk"):
            hpc.mla_indexer_topk_prefill(torch.zeros(1, 64, device="cuda"), one[1], one[2], bad)
