"""hpc.mla_indexer_store_k_fp8 / mla_indexer_logits_fp8 / mla_indexer_topk / mla_indexer_topk_fp8: the DSA lightning indexer.

CPU: the float64 statement (tests/mla_indexer_ref.py) against a brute-force loop; the public surface and fakes; the plan against
the route's arithmetic restated here; host refusals through the C-ABI with never-dereferenced pointers; mutants of plausible bugs
rejected by the logits bar and by the top-k statement on the GPU tests' own inputs.
GPU: the store bit-identical to tests/blockwise_quant_ref.py with every other byte untouched; logits EQUAL to the statement on
exact inputs and within c * 2^-24 * A on random ones; unwritten columns; top-k torch.equal to the statement for planted ties,
zeros of both signs, -inf runs and rows that must not be read; the fused call bit-identical to its parts, repeatable, replayed in
a hipGraph; end to end into the token-sparse attention."""
import ctypes
import functools
from ctypes import c_int, c_int64, c_void_p
from pathlib import Path

import pytest
import torch

import blockwise_quant_ref as bq
import mla_indexer_ref as ir
import mla_needles as mn
import mla_sparse_ref as sr
from utils import attn_close, attn_rel_err

UNSUPPORTED, INVALID = -1, -2
MAX_TOPK = 65536
# the logits bar: |op - statement| <= C_BAR * 2^-24 * A, A the statement with absolute values everywhere and no ReLU.  The
# standard rounding model (128 + 64 accumulations and a few multiplies) gives 256; v_mfma_f32_16x16x128_f8f6f4 does not keep to it.
# Measured on MI355X over this file's four configurations (profiles/mla_indexer.txt): 224.5, 489.2, 315.8 and 257.9, while the
# kernel's own fp32 arithmetic behind an exactly rounded dot product stays below 1 (modelled on the CPU) and integer inputs come
# out exact - the excess is the instruction's internal accumulation of random e4m3 products.  So the bar is twice the measured
# maximum rounded up to a power of two, 2 x 489.2 -> 1024 (2^-14 of A); every mutant of test_logits_bar_rejects_mutants is beyond
# 2.5e6.
C_BAR = 1024


# ---- CPU 1: the statement ------------------------------------------------------------------------------------------------------
def test_statement_against_a_brute_force_loop():
    g = torch.Generator().manual_seed(0)
    P, sq, Hi, B = 16, 2, 3, 3
    codes = torch.randn(7, P, 128, generator=g).to(ir.F8)
    scales = torch.rand(7, P, generator=g) + 0.1
    cache = ir.pack(codes, scales)
    c2, s2 = ir.unpack(cache)
    assert torch.equal(c2.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(s2, scales)
    # the layout, byte for byte: token t's codes at 128 t, its scale at 128 P + 4 t
    assert torch.equal(cache[3, 128 * 5: 128 * 6], codes[3, 5].view(torch.uint8))
    assert torch.equal(cache[3, 128 * P + 4 * 5: 128 * P + 4 * 6].view(torch.float32), scales[3, 5:6])
    q = torch.randn(B * sq, Hi, 128, generator=g).to(ir.F8)
    w = torch.randn(B * sq, Hi, generator=g)
    block_ids = torch.tensor([[3, 1, -1], [0, 99, 2], [6, 5, 4]], dtype=torch.int32)  # 99: a page id outside the pool
    lens_total = torch.tensor([20, 40, 60])                                          # 60: beyond the table's 48 columns
    got = ir.logits_statement(q, w, cache, block_ids, lens_total, sq)
    assert got.shape == (B * sq, 3 * P)
    for r in range(B * sq):
        b, s = divmod(r, sq)
        n = min(int(lens_total[b]) - sq + s + 1, 3 * P)
        assert bool(got[r, n:].isnan().all()) and not bool(got[r, :n].isnan().any())
        for j in range(n):
            page = int(block_ids[b, j // P])
            if not 0 <= page < 7:
                assert got[r, j] == float("-inf")
                continue
            tot = 0.0
            for h in range(Hi):
                dot = sum(float(q[r, h, d]) * float(codes[page, j % P, d]) for d in range(128))
                tot += float(w[r, h]) * max(dot, 0.0)
            assert abs(float(got[r, j]) - float(scales[page, j % P]) * tot) <= 1e-9 * (1 + abs(tot)), (r, j)
    assert bool((got[2, 16:32] == float("-inf")).all()) and bool(torch.isfinite(got[2, :16]).all())
    # the top-k statement on a row with ties, zeros of both signs, a NaN and -inf
    x = torch.tensor([[1.0, 3.0, -0.0, 3.0, float("nan"), 0.0, float("-inf"), 3.0, 2.0, float("inf")]])
    assert ir.topk_statement(x, [10], 1, 4).tolist() == [[1, 3, 4, 9]]        # NaN, inf, then the first two 3.0
    assert ir.topk_statement(x, [10], 1, 7).tolist() == [[0, 1, 3, 4, 7, 8, 9]]
    assert ir.topk_statement(x, [10], 1, 8).tolist() == [[0, 1, 2, 3, 4, 7, 8, 9]]  # -0.0 at 2 before +0.0 at 5
    assert ir.topk_statement(x, [4], 1, 6).tolist() == [[0, 1, 2, 3, -1, -1]]      # n <= topk: the identity list
    assert ir.topk_statement(x, [0], 1, 3).tolist() == [[-1, -1, -1]]
    assert ir.topk_statement(x, [7], 1, 2).tolist() == [[1, 4]]                    # columns at or past n are not candidates


# ---- CPU 2: surface and fakes --------------------------------------------------------------------------------------------------
NAMES = ("mla_indexer_store_k_fp8", "mla_indexer_logits_fp8", "mla_indexer_topk", "mla_indexer_topk_fp8")


def test_surface():
    import hpc

    for name in NAMES:
        assert name in hpc.__all__ and callable(getattr(hpc, name)), name
        assert hasattr(torch.ops.hpc_mla, name), name
    doc = hpc.mla_indexer_store_k_fp8.__doc__
    for word in ("[num_blocks, P * 132]", "torch.uint8", "byte P * 128", "{16, 32, 64, 128}", "multiple of 16 bytes",
                 "scale = amax / 448", "tests/blockwise_quant_ref.py", "mla_rope_norm_store_kv", "hipGraph", "page tails"):
        assert word in doc, word
    doc = hpc.mla_indexer_logits_fp8.__doc__
    for word in ("tests/mla_indexer_ref.py", "vis(b, s) = L_b - Sq + s + 1", "relu(", "{16, 32, 64}", "blockwise_fp8_quant",
                 "Hi ** -0.5", "negative", "-inf", "NOT written", "mtp 0..3", "hipGraph", "bit-identical", "No float atomics"):
        assert word in doc, word
    doc = hpc.mla_indexer_topk.__doc__
    for word in ("ASCENDING", "-0.0 == +0.0", "NaN ranks above +inf", "smaller position", "identity list", "not read at all",
                 "1..65536", "never read", "hipGraph"):
        assert word in doc, word
    doc = hpc.mla_indexer_topk_fp8.__doc__
    for word in ("release_decode_workspaces", "bit-identical", "hipGraph", "scratch"):
        assert word in doc, word


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        q = torch.empty(6, 32, 128, dtype=ir.F8, device="cuda")
        w = torch.empty(6, 32, dtype=torch.float32, device="cuda")
        cache = torch.empty(9, 64 * 132, dtype=torch.uint8, device="cuda")
        bid = torch.empty(3, 5, dtype=torch.int32, device="cuda")
        lens = torch.empty(3, dtype=torch.int32, device="cuda")
        y = hpc.mla_indexer_logits_fp8(q, w, cache, bid, lens, mtp=1)
        assert (y.shape, y.dtype, y.device.type) == ((6, 5 * 64), torch.float32, "cuda")
        o = torch.empty(6, 320, dtype=torch.float32, device="cuda")
        assert hpc.mla_indexer_logits_fp8(q, w, cache, bid, lens, mtp=1, output=o) is o
        t = hpc.mla_indexer_topk(y, lens, 100, mtp=1)
        assert (t.shape, t.dtype, t.device.type) == ((6, 100), torch.int32, "cuda")
        oi = torch.empty(6, 100, dtype=torch.int32, device="cuda")
        assert hpc.mla_indexer_topk(y, lens, 100, mtp=1, output=oi) is oi
        t = hpc.mla_indexer_topk_fp8(q, w, cache, bid, lens, 2048, mtp=1)
        assert (t.shape, t.dtype) == ((6, 2048), torch.int32)
        assert hpc.mla_indexer_topk_fp8(q, w, cache, bid, lens, 100, mtp=1, output=oi) is oi
        k = torch.empty(7, 128, dtype=torch.bfloat16, device="cuda")
        qi = torch.empty(4, dtype=torch.int32, device="cuda")
        assert hpc.mla_indexer_store_k_fp8(cache, k, lens, qi, bid) is None


# ---- CPU 3: the route and the C-ABI ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def plan(lib, B, sq, Hi, P, max_blocks, topk, cus):
    grid, chunk, tgrid, rs, ws = c_int(-7), c_int(-7), c_int(-7), c_int64(-7), c_int64(-7)
    rc = lib.hpc_mla_indexer_plan(B, sq, Hi, P, max_blocks, topk, cus, ctypes.byref(grid), ctypes.byref(chunk), ctypes.byref(tgrid),
                                  ctypes.byref(rs), ctypes.byref(ws))
    return rc, grid.value, chunk.value, tgrid.value, rs.value, ws.value


def _route(B, sq, P, max_blocks, cus):
    """the arithmetic of csrc/mla_indexer_route.h, restated: (logits grid, chunk, top-k grid, scratch row stride, scratch bytes)"""
    cols, chunk = max_blocks * P, 512
    while chunk < 8192 and B * -(-cols // chunk) > 16 * cus:
        chunk *= 2
    return B * -(-cols // chunk), chunk, B * sq, cols, B * sq * cols * 4


@pytest.mark.parametrize("B,sq,Hi,P,max_blocks,cus", [(1, 1, 64, 64, 1024, 256), (64, 1, 64, 64, 128, 256), (64, 1, 64, 64, 512, 256),
                                                      (8, 2, 32, 16, 256, 304), (3, 4, 16, 128, 5, 80), (64, 1, 64, 32, 2048, 64),
                                                      (300, 3, 64, 64, 1, 256), (0, 1, 64, 64, 128, 256), (2, 1, 16, 16, 0, 256)])
def test_plan_is_the_route(lib, B, sq, Hi, P, max_blocks, cus):
    for topk in (0, 1, 2048, MAX_TOPK):
        assert plan(lib, B, sq, Hi, P, max_blocks, topk, cus) == (0,) + _route(B, sq, P, max_blocks, cus), topk


def test_plan_examples(lib):
    # 64 requests over 8k columns: 16 chunks of 512 each; over 64k columns on 256 CUs the chunk doubles until 64 * chunks <= 4096
    assert plan(lib, 64, 1, 64, 64, 128, 2048, 256)[1:3] == (64 * 16, 512)
    assert plan(lib, 64, 1, 64, 64, 1024, 2048, 256)[1:3] == (64 * 64, 1024)
    assert plan(lib, 1, 1, 64, 64, 1024, 2048, 256)[1:3] == (128, 512)
    # the refusals of the plan: what the calls would answer
    ok = (2, 1, 64, 64, 8, 64, 256)
    assert plan(lib, *ok)[0] == 0
    for i, bad, code in ((0, -1, INVALID), (1, 0, INVALID), (1, 5, UNSUPPORTED), (2, 48, UNSUPPORTED), (2, 128, UNSUPPORTED),
                         (3, 48, UNSUPPORTED), (3, 256, UNSUPPORTED), (4, -1, INVALID), (4, 1 << 26, UNSUPPORTED),
                         (5, -1, UNSUPPORTED), (5, MAX_TOPK + 1, UNSUPPORTED)):
        args = list(ok)
        args[i] = bad
        assert plan(lib, *args)[0] == code, (i, bad)


def _ip(v):
    return ctypes.cast(c_void_p(v), ctypes.POINTER(c_int)) if v else None


def _vp(v):
    return c_void_p(v) if v else None


def call_store(lib, *, cache=4096, k=4096, lens=4096, qi=4096, bid=4096, rows=4, req=2, P=64, max_blocks=4, num_blocks=8,
               block_stride=None, k_stride=128, refusal=False):
    bs = P * 132 if block_stride is None else block_stride
    args = (_vp(cache), _vp(k), _ip(lens), _ip(qi), _ip(bid), rows, req, P, max_blocks, num_blocks, c_int64(bs), c_int64(k_stride))
    if refusal:
        return lib.hpc_mla_indexer_store_k_fp8_refusal(*args)
    return lib.hpc_mla_indexer_store_k_fp8_async(*args, None)


def call_logits(lib, *, out=4096, q=4096, w=4096, cache=4096, bid=4096, lens=4096, B=2, sq=1, Hi=64, P=64, max_blocks=4,
                num_blocks=8, block_stride=None, row_stride=None, nki=0, refusal=False):
    bs = P * 132 if block_stride is None else block_stride
    rs = max_blocks * P if row_stride is None else row_stride
    args = (_vp(out), _vp(q), _vp(w), _vp(cache), _ip(bid), _ip(lens), B, sq, Hi, P, max_blocks, num_blocks, c_int64(bs), c_int64(rs))
    if refusal:
        return lib.hpc_mla_indexer_logits_fp8_refusal(*args)
    return lib.hpc_mla_indexer_logits_fp8_async(*args, nki, None)


def call_topk(lib, *, out=4096, logits=4096, lens=4096, B=2, sq=1, cols=256, topk=64, row_stride=None, nki=0, refusal=False):
    rs = cols if row_stride is None else row_stride
    args = (_vp(out), _vp(logits), _ip(lens), B, sq, c_int64(cols), topk, c_int64(rs))
    if refusal:
        return lib.hpc_mla_indexer_topk_refusal(*args)
    return lib.hpc_mla_indexer_topk_async(*args, nki, None)


def call_fused(lib, *, out=4096, q=4096, w=4096, cache=4096, bid=4096, lens=4096, B=2, sq=1, Hi=64, P=64, max_blocks=4,
               num_blocks=8, block_stride=None, topk=64, nki=0, ws=4096, ws_bytes=1 << 30, refusal=False):
    bs = P * 132 if block_stride is None else block_stride
    args = (_vp(out), _vp(q), _vp(w), _vp(cache), _ip(bid), _ip(lens), B, sq, Hi, P, max_blocks, num_blocks, c_int64(bs), topk)
    if refusal:
        return lib.hpc_mla_indexer_topk_fp8_refusal(*args, _vp(ws), c_int64(ws_bytes))
    return lib.hpc_mla_indexer_topk_fp8_async(*args, nki, _vp(ws), c_int64(ws_bytes), None)


_CACHE_REFUSALS = [(dict(P=48), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=256), UNSUPPORTED), (dict(P=0), UNSUPPORTED),
                   (dict(block_stride=64 * 132 - 16), UNSUPPORTED), (dict(block_stride=64 * 132 + 8), UNSUPPORTED),
                   (dict(block_stride=-64 * 132), INVALID), (dict(cache=4096 + 8), UNSUPPORTED), (dict(cache=0), INVALID),
                   (dict(out=0), INVALID)]
_READER_REFUSALS = [(dict(Hi=8), UNSUPPORTED), (dict(Hi=48), UNSUPPORTED), (dict(Hi=128), UNSUPPORTED), (dict(sq=5), UNSUPPORTED),
                    (dict(sq=0), INVALID), (dict(B=-1), INVALID), (dict(max_blocks=-1), INVALID), (dict(max_blocks=0), INVALID),
                    (dict(max_blocks=1 << 26), UNSUPPORTED), (dict(num_blocks=-1), INVALID), (dict(q=0), INVALID), (dict(w=0), INVALID),
                    (dict(bid=0), INVALID), (dict(lens=0), INVALID), (dict(q=4096 + 8), UNSUPPORTED), (dict(w=4096 + 4), UNSUPPORTED),
                    (dict(B=0, P=48), UNSUPPORTED), (dict(B=0, Hi=24), UNSUPPORTED)]
_TOPK_REFUSALS = [(dict(topk=0), UNSUPPORTED), (dict(topk=-1), UNSUPPORTED), (dict(topk=MAX_TOPK + 1), UNSUPPORTED)]


def _refusal_agrees(fn, lib, kwargs, code):
    """the launcher's code, and the same call's refusal in words: a message exactly when the call is refused"""
    assert fn(lib, **kwargs) == code, kwargs
    why = fn(lib, refusal=True, **kwargs)
    assert (why is None) == (code == 0), (kwargs, why)
    assert why is None or len(why.decode()) > 10


@pytest.mark.parametrize("kwargs,code", _CACHE_REFUSALS + _READER_REFUSALS + [(dict(row_stride=255), UNSUPPORTED), (dict(out=4096 + 2), UNSUPPORTED)])
def test_logits_cabi_refuses_on_the_host(lib, kwargs, code):
    _refusal_agrees(call_logits, lib, kwargs, code)


@pytest.mark.parametrize("kwargs,code", _CACHE_REFUSALS + _READER_REFUSALS + _TOPK_REFUSALS + [
    (dict(ws=0), INVALID), (dict(ws_bytes=2 * 256 * 4 - 1), INVALID), (dict(ws=4096 + 2), UNSUPPORTED)])
def test_fused_cabi_refuses_on_the_host(lib, kwargs, code):
    _refusal_agrees(call_fused, lib, kwargs, code)


@pytest.mark.parametrize("kwargs,code", _TOPK_REFUSALS + [
    (dict(sq=5), UNSUPPORTED), (dict(sq=0), INVALID), (dict(B=-1), INVALID), (dict(cols=-1), INVALID), (dict(cols=(1 << 30) + 1), UNSUPPORTED),
    (dict(out=0), INVALID), (dict(logits=0), INVALID), (dict(lens=0), INVALID), (dict(row_stride=255), UNSUPPORTED),
    (dict(out=4096 + 2), UNSUPPORTED), (dict(logits=4096 + 1), UNSUPPORTED), (dict(B=0, topk=0), UNSUPPORTED)])
def test_topk_cabi_refuses_on_the_host(lib, kwargs, code):
    _refusal_agrees(call_topk, lib, kwargs, code)


@pytest.mark.parametrize("kwargs,code", [c for c in _CACHE_REFUSALS if "out" not in c[0]] + [
    (dict(rows=-1), INVALID), (dict(req=-1), INVALID), (dict(max_blocks=-1), INVALID), (dict(num_blocks=-1), INVALID),
    (dict(k=0), INVALID), (dict(lens=0), INVALID), (dict(qi=0), INVALID), (dict(bid=0), INVALID), (dict(k=4096 + 8), UNSUPPORTED),
    (dict(k_stride=132), UNSUPPORTED), (dict(k_stride=120), UNSUPPORTED), (dict(k_stride=-128), UNSUPPORTED),
    (dict(rows=0, P=48), UNSUPPORTED)])
def test_store_cabi_refuses_on_the_host(lib, kwargs, code):
    _refusal_agrees(call_store, lib, kwargs, code)


def test_cabi_accepts_an_empty_batch_without_a_launch(lib):
    """accepted up to the device call: B = 0 (store: no rows, or no requests) returns 0 without one"""
    for kw in (dict(), dict(P=16), dict(block_stride=64 * 132 + 16), dict(Hi=16), dict(sq=4)):
        _refusal_agrees(call_logits, lib, dict(B=0, **kw), 0)
        _refusal_agrees(call_fused, lib, dict(B=0, ws=0, ws_bytes=0, **kw), 0)
    for kw in (dict(), dict(topk=1), dict(topk=MAX_TOPK), dict(cols=0), dict(sq=4)):
        _refusal_agrees(call_topk, lib, dict(B=0, **kw), 0)
    for kw in (dict(rows=0), dict(req=0), dict(rows=0, cache=0, k=0), dict(rows=0, P=128, block_stride=128 * 132 + 32)):
        _refusal_agrees(call_store, lib, kw, 0)
    # calls with work that every host check accepts are refused by nothing (no launch is made here: the words only)
    for fn in (call_logits, call_fused, call_topk, call_store):
        assert fn(lib, refusal=True) is None


def test_both_libraries_export_the_launchers():
    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for name in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        so = ctypes.CDLL(str(pkg / name))
        for op in ("store_k_fp8", "logits_fp8", "topk", "topk_fp8"):
            for kind in ("async", "refusal"):
                assert hasattr(so, f"hpc_mla_indexer_{op}_{kind}"), (name, op, kind)
        assert hasattr(so, "hpc_mla_indexer_plan"), name


# ---- CPU 4: the bars have teeth, on the GPU tests' own inputs ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(i, exact):
    """(inputs, the statement float64 with NaN where nothing is written, A of the bound) of one configuration - computed once"""
    Hi, mtp, P = ir.CONFIGS[i]
    inp = ir.inputs(Hi, mtp, P, exact=exact)
    return inp, ir.statement(inp), (None if exact else ir.statement(inp, absolute=True))


@pytest.mark.parametrize("i", range(len(ir.CONFIGS)))
def test_logits_bar_rejects_mutants(i):
    """each mutant of a plausible bug, run through the statement: unequal to the statement on the exact inputs, and beyond
    C_BAR * 2^-24 * A somewhere (or writing other columns) on the random ones"""
    exact, want_e, _ = _case(i, True)
    rand, want_r, A = _case(i, False)
    for name, mutation in ir.LOGITS_MUTANTS.items():
        assert not ir.equal_where_written(ir.statement(exact, **mutation).float(), want_e), (i, name)
        ratio = ir.worst_ratio(ir.statement(rand, **mutation).float(), want_r, A)
        print(f"  config {ir.CONFIGS[i]} {name:40s} {ratio:12.4g} x 2^-24 A (bar {C_BAR})")
        assert ratio > C_BAR, (i, name, ratio)
    # and the statement itself, rounded to float32, passes both
    assert ir.equal_where_written(want_e.float(), want_e) and ir.worst_ratio(want_r.float(), want_r, A) <= 1.0


def _exact_logits(i):
    """the exact test's integer logits as the top-k's input: float32, the unwritten columns NaN"""
    inp, want, _ = _case(i, True)
    return inp, want.float()


_EXACT_TOPK = [(0, 64), (1, 65), (2, 1000), (3, 2048)]  # (configuration, topk) of the GPU test over the exact test's logits


def test_topk_mutants_differ():
    """each mutant's lists differ from the statement's on the exact inputs of the GPU test (a tie has to sit on the threshold
    for the tie rule to show: not every (configuration, topk) has one, so the cases are taken together)"""
    differs = {name: [] for name in ir.TOPK_MUTANTS}
    for i, topk in _EXACT_TOPK:
        inp, logits = _exact_logits(i)
        sq = inp["num_seq_q"]
        want = ir.topk_statement(logits, inp["lens_total"], sq, topk)
        for name, mutation in ir.TOPK_MUTANTS.items():
            if not torch.equal(ir.topk_statement(logits, inp["lens_total"], sq, topk, **mutation), want):
                differs[name].append((i, topk))
    print(differs)
    assert all(differs.values()), differs


# ---- GPU: the store ------------------------------------------------------------------------------------------------------------
FILL = 0xA5


def _store_case(P, new, lens_total, *, pad_rows=0, seed=0, dead=()):
    """requests with `new` tokens each at the end of lens_total; `dead`: (request, table slot) pairs whose page id is poisoned.
    Returns the op's inputs (CPU) and the expected cache over a pool pre-filled with FILL."""
    g = torch.Generator().manual_seed(seed)
    R = len(new)
    T = sum(new) + pad_rows
    nblocks = [-(-L // P) for L in lens_total]
    pool = sum(nblocks) + 2
    perm = torch.randperm(pool, generator=g).to(torch.int32)
    max_blocks = max(nblocks)
    bid = torch.full((R, max_blocks), -1, dtype=torch.int32)
    off = 0
    for b, nb in enumerate(nblocks):
        bid[b, :nb] = perm[off: off + nb]
        off += nb
    for b, slot in dead:
        bid[b, slot] = pool + 5 if slot % 2 else -1
    k = (torch.randn(T, 128, generator=g) * torch.exp2(torch.randint(-3, 4, (T, 1), generator=g).float())).bfloat16()
    k[T // 2] = 0  # a row of zeros: scale 0
    qi = torch.tensor([0] + list(torch.tensor(new).cumsum(0)), dtype=torch.int32)
    codes, scales = bq.quant(k)
    want = torch.full((pool, P * 132), FILL, dtype=torch.uint8)
    stored = 0
    for b in range(R):
        for i in range(new[b]):
            r = int(qi[b]) + i
            pos = lens_total[b] - new[b] + i
            if pos < 0 or pos // P >= max_blocks or not 0 <= int(bid[b, pos // P]) < pool:
                continue
            page, t = int(bid[b, pos // P]), pos % P
            want[page, 128 * t: 128 * t + 128] = codes[r].view(torch.uint8)
            want[page, 128 * P + 4 * t: 128 * P + 4 * t + 4] = scales[r].view(torch.uint8)
            stored += 1
    return dict(k=k, lens=torch.tensor(lens_total, dtype=torch.int32), qi=qi, bid=bid, pool=pool, want=want, stored=stored)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [16, 64])
def test_store_is_the_quantiser_bit_for_bit_and_touches_nothing_else(P):
    import hpc

    g = torch.Generator().manual_seed(P)
    decode_lens = [int(v) for v in torch.randint(4, 40 * P, (64,), generator=g)]
    decode_lens[0], decode_lens[1], decode_lens[2] = 4, P, P + 1          # the new tokens at the very start / across the first edge
    cases = {
        "T 1": _store_case(P, [1], [5 * P + 3], seed=1),
        "64 requests x mtp 3": _store_case(P, [4] * 64, decode_lens, seed=2, pad_rows=7, dead=[(5, 0), (9, 1), (11, 0)]),
        # a prefill chunk of 300 rows over two requests that crosses page edges; request 2 is longer than its new tokens
        "prefill chunk of 300": _store_case(P, [171, 129], [171, 129 + 3 * P + 5], seed=3),
        # a request whose length is below its row count owns rows of no request (pos < 0), and one with no rows at all
        "rows of no request": _store_case(P, [6, 0, 3], [4, 50, 3], seed=4, pad_rows=2),
    }
    for name, c in cases.items():
        cache = torch.full((c["pool"], P * 132), FILL, dtype=torch.uint8, device="cuda")
        args = (c["lens"].cuda(), c["qi"].cuda(), c["bid"].cuda())
        assert hpc.mla_indexer_store_k_fp8(cache, c["k"].cuda(), *args) is None
        assert c["stored"] > 0 and torch.equal(cache.cpu(), c["want"]), name
        # a strided k view (row stride 136) and a cache with a padded block stride give the same bytes
        wide = torch.zeros(len(c["k"]), 136, dtype=torch.bfloat16, device="cuda")
        wide[:, :128] = c["k"].cuda()
        big = torch.full((c["pool"], P * 132 + 48), FILL, dtype=torch.uint8, device="cuda")
        view = big[:, : P * 132]
        assert not wide[:, :128].is_contiguous() or len(c["k"]) == 1
        hpc.mla_indexer_store_k_fp8(view, wide[:, :128], *args)
        assert torch.equal(view.cpu(), c["want"]) and bool((big[:, P * 132:] == FILL).all()), name
    # positions beyond the table store nothing: the same decode case with its table cut to two columns
    c = cases["64 requests x mtp 3"]
    cache = torch.full((c["pool"], P * 132), FILL, dtype=torch.uint8, device="cuda")
    hpc.mla_indexer_store_k_fp8(cache, c["k"].cuda(), c["lens"].cuda(), c["qi"].cuda(), c["bid"][:, :2].contiguous().cuda())
    keep = torch.zeros(c["pool"], dtype=torch.bool)
    for b in range(64):
        for slot in range(2):
            if 0 <= int(c["bid"][b, slot]) < c["pool"]:
                keep[int(c["bid"][b, slot])] = True
    want = torch.where(keep[:, None], c["want"], torch.full_like(c["want"], FILL))
    assert torch.equal(cache.cpu(), want)


# ---- GPU: the logits -----------------------------------------------------------------------------------------------------------
def _dev(inp):
    return (inp["q"].cuda(), inp["weights"].cuda(), inp["k_cache"].cuda(), inp["block_ids"].cuda())


def _logits(inp, nki=True, **kw):
    import hpc

    lens = inp["lens_total"] if nki else inp["lens_total"] - inp["num_seq_q"]
    return hpc.mla_indexer_logits_fp8(*_dev(inp), lens.cuda(), mtp=inp["num_seq_q"] - 1, new_kv_included=nki, **kw)


def _nan_output(inp):
    cols = inp["block_ids"].shape[1] * inp["P"]
    return torch.full((len(inp["lens_total"]) * inp["num_seq_q"], cols), float("nan"), dtype=torch.float32, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ir.CONFIGS)))
def test_logits_equal_the_statement_on_exact_inputs(i):
    """integer codes, integer weights, power-of-two scales: every partial sum is an integer below 2^24, so the result must EQUAL
    the float64 statement cast to float32 whatever the order of the instruction's sums; -inf exactly on the poisoned pages; the
    columns at or past min(vis, max_blocks * P) still NaN"""
    inp, want, _ = _case(i, True)
    out = _nan_output(inp)
    assert _logits(inp, output=out) is out
    assert ir.equal_where_written(out, want), ir.CONFIGS[i]
    P, sq = inp["P"], inp["num_seq_q"]
    for b, slot in inp["dead"]:
        for s in range(sq):
            n = max(ir.vis_of(inp["lens_total"], sq, b, s), 0)
            row = out[b * sq + s, :n].cpu()
            dead = torch.zeros(n, dtype=torch.bool)
            dead[slot * P: (slot + 1) * P] = True
            assert torch.equal(row == float("-inf"), dead), (b, s)
    # the lengths given the other way (before the step; negative where a request is shorter than its q rows)
    other = _nan_output(inp)
    _logits(inp, nki=False, output=other)
    assert torch.equal(other.view(torch.int32), out.view(torch.int32))
    # a fresh output: the written columns are the same
    fresh = _logits(inp).cpu()
    m = ~want.isnan()
    assert torch.equal(fresh[m], out.cpu()[m])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ir.CONFIGS)))
def test_logits_within_the_rounding_bound_on_random_inputs(i):
    """random e4m3 codes, scales in [2^-6, 2^-2], signed normal weights: |op - statement| <= C_BAR * 2^-24 * A.  The ratio
    err / (2^-24 A) is printed; what was measured, and why the bar is 1024 and not the rounding model's 256, stands at C_BAR."""
    inp, want, A = _case(i, False)
    out = _nan_output(inp)
    _logits(inp, output=out)
    ratio = ir.worst_ratio(out, want, A)
    print(f"\nmla_indexer_logits_fp8 {ir.CONFIGS[i]}: worst err / (2^-24 A) = {ratio:.3f} (bar {C_BAR})")
    assert ratio <= C_BAR, (ir.CONFIGS[i], ratio)
    for _ in range(3):  # the head sum has a fixed order: the same bits on every call
        again = _nan_output(inp)
        _logits(inp, output=again)
        assert torch.equal(again.view(torch.int32), out.view(torch.int32))


GUARD = 1 << 20


@pytest.mark.gpu
def test_logits_guard_bands_through_the_cabi(lib):
    """a logits buffer of exactly rows x row stride floats between 1 MiB guard bands, the row stride wider than the columns: the
    bands, the gap behind every row and the unwritten columns still hold their NaN afterwards"""
    inp, want, _ = _case(1, True)
    q, w, cache, bid = _dev(inp)
    lens = inp["lens_total"].cuda()
    rows, cols = want.shape
    rs = cols + 24
    buf = torch.full((2 * GUARD + rows * rs * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = call_logits(lib, out=buf.data_ptr() + GUARD, q=q.data_ptr(), w=w.data_ptr(), cache=cache.data_ptr(), bid=bid.data_ptr(),
                     lens=lens.data_ptr(), B=len(lens), sq=inp["num_seq_q"], Hi=inp["Hi"], P=inp["P"], max_blocks=bid.shape[1],
                     num_blocks=cache.shape[0], block_stride=cache.stride(0), row_stride=rs, nki=1)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + rows * rs * 4:] == 0xFF).all())
    body = buf[GUARD: GUARD + rows * rs * 4].view(torch.float32).reshape(rows, rs)
    assert bool((body[:, cols:].contiguous().view(torch.int32) == -1).all())
    assert ir.equal_where_written(body[:, :cols], want)


# ---- GPU: the top-k ------------------------------------------------------------------------------------------------------------
def _topk(logits, lens_total, topk, sq=1, **kw):
    import hpc

    return hpc.mla_indexer_topk(logits, torch.as_tensor(lens_total, dtype=torch.int32).cuda(), topk, mtp=sq - 1,
                                new_kv_included=True, **kw)


def _planted_row(n, cols, g, unread):
    """n columns of random logits with many duplicates, zeros of both signs and runs of -inf, then `unread` values to the end"""
    x = torch.randn(n, generator=g)
    x[torch.rand(n, generator=g) < 0.5] = 0.375  # one value, half of the row
    x = torch.where(torch.rand(n, generator=g) < 0.3, (x * 4).round() / 4, x)                    # a coarse grid: many ties
    x[torch.rand(n, generator=g) < 0.05] = 0.0
    x[torch.rand(n, generator=g) < 0.05] = -0.0
    for start in torch.randint(0, max(n, 1), (4,), generator=g).tolist():
        x[start: start + 37] = float("-inf")
    row = torch.empty(cols)
    row[:n] = x
    row[n::2] = unread[0]
    row[n + 1::2] = unread[1]
    return row


@pytest.mark.gpu
@pytest.mark.parametrize("topk", [1, 64, 65, 1000, 2048])
def test_topk_is_the_statement_for_any_input(topk):
    """ids torch.equal the statement: planted duplicates, +0.0 and -0.0, -inf runs; columns at or past n_r hold +inf and NaN and
    must never be chosen; the rows with n_r <= topk come out right while ALL their logits are NaN: they are not read"""
    g = torch.Generator().manual_seed(topk)
    ns = [0, 1, topk - 1, topk, topk + 1, 5000, 40000]
    cols = 40000 + 72
    rows = []
    for n in ns:
        if n <= topk:
            rows.append(torch.full((cols,), float("nan")))
        else:
            rows.append(_planted_row(n, cols, g, (float("inf"), float("nan"))))
    logits = torch.stack(rows)
    want = ir.topk_statement(logits, ns, 1, topk)
    assert all(sorted(set(r.tolist()) - {-1}) == [v for v in r.tolist() if v >= 0] for r in want)  # ascending, no repeats
    out = torch.full((len(ns), topk), -7, dtype=torch.int32, device="cuda")
    assert _topk(logits.cuda(), ns, topk, output=out) is out
    assert torch.equal(out.cpu(), want), [i for i in range(len(ns)) if not torch.equal(out[i].cpu(), want[i])]
    # a strided logits view and a fresh output
    wide = torch.full((len(ns), cols + 8), float("inf"), device="cuda")
    wide[:, :cols] = logits.cuda()
    assert torch.equal(_topk(wide[:, :cols], ns, topk).cpu(), want)
    # NaN and +inf INSIDE the row rank on top, in position order
    if topk < 5000:
        row = _planted_row(5000, cols, g, (float("inf"), float("nan")))
        row[[7, 4000]] = float("nan")
        row[[3, 4999]] = float("inf")
        one = row[None, :].contiguous()
        w1 = ir.topk_statement(one, [5000], 1, topk)
        assert 7 in w1[0].tolist() and (topk < 4 or {3, 7, 4000, 4999} <= set(w1[0].tolist()))
        assert torch.equal(_topk(one.cuda(), [5000], topk).cpu(), w1)


@pytest.mark.gpu
@pytest.mark.parametrize("i,topk", _EXACT_TOPK)
def test_topk_of_the_exact_tests_integer_logits(i, topk):
    """integer logits tie massively, and with mtp > 0 the rows of a request end at different columns"""
    inp, logits = _exact_logits(i)
    sq = inp["num_seq_q"]
    want = ir.topk_statement(logits, inp["lens_total"], sq, topk)
    got = _topk(logits.cuda(), inp["lens_total"], topk, sq=sq)
    assert torch.equal(got.cpu(), want)


# ---- GPU: the fused call -------------------------------------------------------------------------------------------------------
def _fill_scratch_with_nan():
    import hpc  # noqa: F401  (registers the ops)

    for ws in torch.ops.hpc_mla._mla_indexer_workspaces():
        ws.fill_(0xFF)  # every float of it a NaN


def _fused(inp, topk, **kw):
    import hpc

    return hpc.mla_indexer_topk_fp8(*_dev(inp), inp["lens_total"].cuda(), topk, mtp=inp["num_seq_q"] - 1, new_kv_included=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("i,exact,topk", [(0, False, 64), (1, True, 65), (2, False, 1000), (3, True, 2048)])
def test_fused_is_its_two_parts_bit_for_bit(i, exact, topk):
    import hpc

    inp, want, _ = _case(i, exact)
    sq = inp["num_seq_q"]
    parts = _topk(_logits(inp, output=_nan_output(inp)), inp["lens_total"], topk, sq=sq)
    _fused(inp, topk)  # the scratch exists
    assert len(torch.ops.hpc_mla._mla_indexer_workspaces()) == 1
    first = None
    for _ in range(20):
        _fill_scratch_with_nan()
        got = _fused(inp, topk)
        assert torch.equal(got, parts)
        first = got if first is None else first
        assert torch.equal(got, first)
    if exact:  # and the statement's list, through the statement's logits
        assert torch.equal(parts.cpu(), ir.topk_statement(want.float(), inp["lens_total"], sq, topk))
    hpc.release_decode_workspaces()
    assert len(torch.ops.hpc_mla._mla_indexer_workspaces()) == 0


@pytest.mark.gpu
def test_graph_replays_after_lengths_pages_cache_and_q_changed_in_place():
    """capture once with output given; replay; change everything in place; replay: the new result"""
    import hpc

    Hi, mtp, P, topk = 32, 1, 32, 200
    a = ir.inputs(Hi, mtp, P, exact=True, lens_total=[700, 64, 3000, 5], seed=31)
    b = ir.inputs(Hi, mtp, P, exact=True, lens_total=[65, 2000, 2, 900], seed=32)
    pool = max(a["k_cache"].shape[0], b["k_cache"].shape[0])
    cols = max(a["block_ids"].shape[1], b["block_ids"].shape[1])

    def padded(c):  # the case's pool inside the graph's pool, its table inside the graph's table
        cache = torch.full((pool, P * 132), 0x38, dtype=torch.uint8)
        cache[: c["k_cache"].shape[0]] = c["k_cache"]
        bid = torch.full((4, cols), -1, dtype=torch.int32)
        bid[:, : c["block_ids"].shape[1]] = c["block_ids"]
        return dict(c, k_cache=cache, block_ids=bid)

    cases = [padded(a), padded(b)]
    q = torch.zeros(4 * (mtp + 1), Hi, 128, device="cuda").to(ir.F8)
    w = torch.zeros(4 * (mtp + 1), Hi, device="cuda")
    cache = torch.zeros(pool, P * 132, dtype=torch.uint8, device="cuda")
    bid = torch.full((4, cols), -1, dtype=torch.int32, device="cuda")
    lens = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(4 * (mtp + 1), topk, dtype=torch.int32, device="cuda")

    def load(c):
        q.view(torch.uint8).copy_(c["q"].view(torch.uint8))
        w.copy_(c["weights"])
        cache.copy_(c["k_cache"])
        bid.copy_(c["block_ids"])
        lens.copy_(c["lens_total"])

    def step():
        return hpc.mla_indexer_topk_fp8(q, w, cache, bid, lens, topk, mtp=mtp, new_kv_included=True, output=out)

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert step() is out
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()
        step()
        grown = torch.cuda.memory_allocated() - before
    ws_bytes = sum(t.numel() for t in torch.ops.hpc_mla._mla_indexer_workspaces())
    assert grown <= ws_bytes, (grown, ws_bytes)  # nothing allocated in the capture beyond the cached scratch
    for c in (cases[0], cases[1], cases[0]):
        load(c)
        out.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        want = ir.topk_statement(ir.statement(c).float(), c["lens_total"], mtp + 1, topk)
        assert torch.equal(out.cpu(), want)
    del graph
    hpc.release_decode_workspaces()


# ---- GPU: end to end into the token-sparse attention -------------------------------------------------------------------------------
def _end_to_end(contexts, H, P, topk, Hi=16, seed=5):
    """store every token's index key, then the fused indexer; returns (the attention's needle inputs, indices on the GPU, the
    statement's indices).  Exact-input keys: integers in [-7, 7] with a 7 in every row, so the stored scale is 1/64 and the stored
    codes are 64 k exactly; q codes and weights are integers in [-2, 2]: every partial sum is an integer below 2^24."""
    import hpc

    inp = mn.needle_inputs(contexts, 1, P, H, seed=seed)
    g = torch.Generator().manual_seed(seed)
    lens_total = inp["lens_total"]
    B, T = len(lens_total), int(lens_total.sum())
    k = torch.randint(-7, 8, (T, 128), generator=g).float()
    k[:, 0] = 7.0
    k = k.bfloat16()
    pool = inp["ckv"].shape[0]
    k_cache = torch.full((pool, P * 132), FILL, dtype=torch.uint8, device="cuda")
    qi = torch.tensor([0] + lens_total.cumsum(0).tolist(), dtype=torch.int32)
    bid = inp["block_ids"].cuda()
    hpc.mla_indexer_store_k_fp8(k_cache, k.cuda(), lens_total.cuda(), qi.cuda(), bid)
    codes, scales = ir.unpack(k_cache.cpu())
    for b in range(B):  # what was stored is 64 k and 1 / 64, exactly
        for pos in (0, int(lens_total[b]) - 1):
            page, row = int(inp["block_ids"][b, pos // P]), int(qi[b]) + pos
            assert torch.equal(codes[page, pos % P].float(), 64 * k[row].float()) and float(scales[page, pos % P]) == 1 / 64
    q_idx = torch.randint(-2, 3, (B, Hi, 128), generator=g).float().to(ir.F8)
    w = torch.randint(1, 3, (B, Hi), generator=g).float() * (1 - 2 * torch.randint(0, 2, (B, Hi), generator=g)).float()
    idx = hpc.mla_indexer_topk_fp8(q_idx.cuda(), w.cuda(), k_cache, bid, lens_total.cuda(), topk, new_kv_included=True)
    logits = ir.logits_statement(q_idx, w, k_cache.cpu(), inp["block_ids"], lens_total, 1)
    return inp, idx, ir.topk_statement(logits.float(), lens_total, 1, topk)


@pytest.mark.gpu
def test_end_to_end_store_indexer_sparse_attention():
    """store -> fused indexer -> sparse attention: the indices are the statement's, and the attention on them stays within the
    needle bars of tests/test_attention_decode_mla_sparse.py against mla_sparse_ref.sparse_statement"""
    import hpc

    topk = 64
    inp, idx, want = _end_to_end([40, 64, 300], 16, 64, topk)
    assert torch.equal(idx.cpu(), want)
    assert want[0].tolist() == list(range(41)) + [-1] * 23 and int((want[1] >= 0).sum()) == 64 and int((want[2] >= 0).sum()) == 64
    out, lse = hpc.attention_decode_mla_sparse_bf16(inp["q"].cuda(), inp["ckv"].cuda(), inp["block_ids"].cuda(), inp["lens_before"].cuda(),
                                                    idx, inp["scale"], return_lse=True)
    ref, rlse = sr.sparse_statement(inp["q"], inp["ckv"], inp["block_ids"], inp["lens_total"], want, 1, inp["scale"])
    ref = ref.to(torch.bfloat16)
    w_out, w_lse = float(attn_rel_err(ref, out.cpu(), 1).max()), mn.lse_err(rlse, lse)
    print(f"\nend to end: out worst {w_out:.5f} (tau {mn.TAU_NEEDLE}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_NEEDLE})")
    assert attn_close(ref, out.cpu(), mn.TAU_NEEDLE, 1, label="indexer end to end")
    assert w_lse <= mn.LSE_BAR_NEEDLE


@pytest.mark.gpu
def test_end_to_end_identity_lists_give_the_dense_attention_bit_for_bit():
    """every context <= topk, mtp 0, splits 1: the indexer yields 0 .. L_b - 1 then -1, on which the sparse attention is the
    dense one at splits 1, bit for bit"""
    import hpc

    topk = 700
    inp, idx, want = _end_to_end([0, 1, 63, 64, 65, 600, 699], 16, 32, topk, seed=6)
    assert torch.equal(idx.cpu(), want)
    L = inp["lens_total"]
    ident = torch.arange(topk, dtype=torch.int32)[None, :].repeat(len(L), 1)
    ident[ident >= L[:, None]] = -1
    assert torch.equal(want, ident)
    args = (inp["q"].cuda(), inp["ckv"].cuda(), inp["block_ids"].cuda(), inp["lens_before"].cuda())
    out, lse = hpc.attention_decode_mla_sparse_bf16(*args, idx, inp["scale"], return_lse=True, splits=1)
    dout, dlse = hpc.attention_decode_mla_bf16(*args, inp["scale"], return_lse=True, splits=1)
    assert torch.equal(out.view(torch.int16), dout.view(torch.int16)) and torch.equal(lse.view(torch.int32), dlse.view(torch.int32))


@pytest.mark.gpu
def test_empty_batch_and_refusals():
    import hpc

    cache = torch.zeros(2, 64 * 132, dtype=torch.uint8, device="cuda")
    q0 = torch.empty(0, 64, 128, device="cuda").to(ir.F8)
    w0 = torch.empty(0, 64, device="cuda")
    bid0 = torch.empty(0, 3, dtype=torch.int32, device="cuda")
    lens0 = torch.empty(0, dtype=torch.int32, device="cuda")
    assert hpc.mla_indexer_logits_fp8(q0, w0, cache, bid0, lens0).shape == (0, 192)
    assert hpc.mla_indexer_topk_fp8(q0, w0, cache, bid0, lens0, 64).shape == (0, 64)
    assert hpc.mla_indexer_topk(torch.empty(0, 192, device="cuda"), lens0, 64).shape == (0, 64)
    hpc.mla_indexer_store_k_fp8(cache, torch.empty(0, 128, dtype=torch.bfloat16, device="cuda"), lens0, torch.zeros(1, dtype=torch.int32, device="cuda"), bid0)
    q = torch.zeros(1, 64, 128, device="cuda").to(ir.F8)
    w = torch.zeros(1, 64, device="cuda")
    one = (torch.zeros(1, 1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="q dtype must be float8_e4m3fn"):
        hpc.mla_indexer_logits_fp8(q.view(torch.uint8), w, cache, *one)
    with pytest.raises(RuntimeError, match="index head count"):
        hpc.mla_indexer_logits_fp8(q[:, :24], w[:, :24].contiguous(), cache, *one)
    with pytest.raises(RuntimeError, match="block_size"):
        hpc.mla_indexer_logits_fp8(q, w, cache[:, : 48 * 132], *one)
    with pytest.raises(RuntimeError, match="k_cache must be"):
        hpc.mla_indexer_logits_fp8(q, w, cache[:, :100], *one)
    with pytest.raises(RuntimeError, match="mtp"):
        hpc.mla_indexer_logits_fp8(q, w, cache, *one, mtp=4)
    with pytest.raises(RuntimeError, match="weights"):
        hpc.mla_indexer_logits_fp8(q, w[:, :32], cache, *one)
    for bad in (0, MAX_TOPK + 1):
        with pytest.raises(RuntimeError, match="topk"):
            hpc.mla_indexer_topk_fp8(q, w, cache, *one, bad)
        with pytest.raises(RuntimeError, match="topk"):
            hpc.mla_indexer_topk(torch.zeros(1, 64, device="cuda"), one[1], bad)
    with pytest.raises(RuntimeError, match="logits dtype must be float32"):
        hpc.mla_indexer_topk(torch.zeros(1, 64, device="cuda").half(), one[1], 8)
    with pytest.raises(RuntimeError, match="k dtype must be bfloat16"):
        hpc.mla_indexer_store_k_fp8(cache, torch.zeros(1, 128, device="cuda"), one[1], torch.tensor([0, 1], dtype=torch.int32, device="cuda"), one[0])
