"""hpc.attention_decode_mla_sparse_bf16 / _fp8: MLA decode attention over a list of token positions per q row.

CPU: the float64 statement (tests/mla_sparse_ref.py) against a brute-force loop, with the duplicate and empty-row rules; the
bars of tests/mla_needles.py measured again with the split-list model on this file's calibration cases; mutants of plausible
bugs rejected at >= 3 tau; the public surface and fakes; the plan against the route's arithmetic restated here; host refusals
through the C-ABI with never-dereferenced pointers.
GPU: needle parity for both ops at every split count, the FP8 op bit-equal to the bf16 op on the dequantised cache, identity
lists bit-identical to the dense op, permuted lists, exact one-entry / duplicate / all-invalid cases, forced splits over
NaN-filled scratch, strided caches, repeatability, a hipGraph replayed after everything changed in place, guard bands, refusals."""
import ctypes
import functools
import math
from ctypes import c_float, c_int, c_int64, c_void_p
from pathlib import Path

import pytest
import torch

import mla_fp8_ref as f8
import mla_needles as mn
import mla_sparse_needles as sn
import mla_sparse_ref as sr
from utils import attn_close, attn_rel_err

DIM, DIM_V = sr.DIM, sr.DIM_V
MAX_SPLITS, MAX_TOPK = 64, 65536
VARY_SEED = 4321
OPS = ("bf16", "fp8")


# ---- CPU 1: the statement ------------------------------------------------------------------------------------------------------
def _brute(q, ckv, block_ids, lens_total, indices, sq, scale):
    """entry by entry, in Python floats"""
    R, H = q.shape[0], q.shape[1]
    P, nblk = ckv.shape[1], ckv.shape[0]
    out = torch.zeros(R, H, DIM_V, dtype=torch.float64)
    lse = torch.full((R, H), float("-inf"), dtype=torch.float64)
    for r in range(R):
        b, s = divmod(r, sq)
        vis = int(lens_total[b]) - sq + s + 1
        rows = []
        for idx in indices[r].tolist():
            if not 0 <= idx < vis or idx // P >= block_ids.shape[1]:
                continue
            page = int(block_ids[b, idx // P])
            if 0 <= page < nblk:
                rows.append(ckv[page, idx % P].double())
        for h in range(H):
            z = [scale * float(q[r, h].double() @ c) for c in rows]
            if not z:
                continue
            mx = max(z)
            den = sum(math.exp(v - mx) for v in z)
            lse[r, h] = mx + math.log(den)
            for v, c in zip(z, rows):
                out[r, h] += math.exp(v - mx) / den * c[:DIM_V]
    return out, lse


def test_statement_against_a_brute_force_loop():
    g = torch.Generator().manual_seed(0)
    P, sq, H, B = 16, 2, 3, 3
    ckv = torch.randn(7, P, DIM, generator=g).bfloat16()
    q = torch.randn(B * sq, H, DIM, generator=g).bfloat16()
    block_ids = torch.tensor([[3, 1, -999999], [0, 5, 2], [6, 99, 4]], dtype=torch.int32)  # 99: a page id outside the pool
    lens_total = torch.tensor([20, 40, 48])
    indices = torch.tensor([
        [0, 5, 5, 18, 19, -1, 17, 100],      # (0, 0): vis 19 - a duplicate, 19 is row 1's token, -1, beyond the table
        [19, 3, 20, 47, -5, 3, 3, 16],       # (0, 1): vis 20 - a triple, 20 past the length, 47 on the padding page
        [-1, -1, 39, 64, 2 ** 31 - 1, -2 ** 31, 48, 40],  # (1, 0): vis 39 - nothing valid at all
        [39, 0, 17, 33, 15, 16, 31, 32],     # (1, 1): vis 40
        [16, 17, 31, 20, -1, -1, -1, -1],    # (2, 0): every entry on the page with id 99 - nothing valid
        [0, 16, 32, 46, 47, 15, 31, 33],     # (2, 1): vis 48, two entries on the page with id 99
    ], dtype=torch.int32)
    want, wlse = _brute(q, ckv, block_ids, lens_total, indices, sq, 0.11)
    got, glse = sr.sparse_statement(q, ckv, block_ids, lens_total, indices, sq, 0.11)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    finite = torch.isfinite(wlse)
    assert torch.equal(finite, torch.isfinite(glse)) and torch.allclose(glse[finite], wlse[finite], rtol=0, atol=1e-12)
    # the empty-row rule: zeros and -inf
    for r in (2, 4):
        assert bool((got[r] == 0).all()) and bool((glse[r] == float("-inf")).all())
    assert bool(torch.isfinite(glse[[0, 1, 3, 5]]).all())
    # the duplicate rule: listing a position again counts it again - and is not the same as listing it once
    once = indices.clone()
    once[0, 2] = -1
    alt, alse = sr.sparse_statement(q, ckv, block_ids, lens_total, once, sq, 0.11)
    assert float((alt[0] - got[0]).abs().max()) > 1e-3 and bool((glse[0] > alse[0]).all())
    assert torch.equal(alt[1:], got[1:])
    # a list of one position twice: the same row, lse larger by ln 2
    two = torch.full_like(indices, -1)
    two[:, 0] = 1
    a1, l1 = sr.sparse_statement(q, ckv, block_ids, lens_total, two, sq, 0.11)
    two[:, 5] = 1
    a2, l2 = sr.sparse_statement(q, ckv, block_ids, lens_total, two, sq, 0.11)
    assert torch.allclose(a1, a2, rtol=0, atol=1e-12) and torch.allclose(l2 - l1, torch.full_like(l1, math.log(2.0)), atol=1e-12)


# ---- CPU 2: the bars, measured on this file's cases ------------------------------------------------------------------------------
# (lens before the step, Sq, H, P, topk): the issue's calibration cases
_CAL = [([0, 1, 63, 64, 1500, 4000], 2, 16, 64, 128), ([0, 15, 16, 17, 65, 300], 4, 32, 16, 64),
        ([5000, 700, 129], 1, 48, 32, 320), ([5000, 64, 2100], 2, 16, 64, 2048)]


@functools.lru_cache(maxsize=None)
def _cal_case(i):
    lens, sq, H, P, topk = _CAL[i]
    inp = sn.sparse_needle_inputs(lens, sq, P, H, topk, seed=11)
    return inp, sn.statement(inp)


@functools.lru_cache(maxsize=None)
def _cal_case_fp8(i):
    """(inputs over the dequantised cache, the uint8 cache, the original inputs, the statement's result)"""
    orig, _ = _cal_case(i)
    cache = f8.quantise(orig["ckv"], vary_seed=VARY_SEED + i)
    inp = dict(orig, ckv=f8.dequantise(cache))
    return inp, cache, orig, sn.statement(inp)


def test_lists_hold_the_needles_at_the_edges_and_the_traps_inside():
    for i in range(len(_CAL)):
        inp, _ = _cal_case(i)
        sq, P, topk = inp["num_seq_q"], inp["P"], inp["topk"]
        assert inp["indices"].shape == (len(inp["lens_total"]) * sq, topk) and inp["indices"].dtype == torch.int32
        assert len(inp["dead_pages"]) >= 1
        flat = inp["indices"].flatten().tolist()
        assert -1 in flat and -2 ** 31 in flat and 2 ** 31 - 1 in flat and 2 ** 30 + 3 in flat
        for b in range(len(inp["lens_total"])):
            for s in range(sq):
                row = inp["indices"][b * sq + s].tolist()
                vis = sr.vis_of(inp["lens_total"], sq, b, s)
                n = max(k for k, v in enumerate(row) if v != -1) + 1
                cands = sn.candidates(int(inp["lens_before"][b]), s, sq, P)
                # 63, 64 and the last slot in use hold candidate positions, as far as the row has candidates
                for k in sn.edge_slots(topk, n)[: min(3, len(cands))]:
                    assert row[k] in cands and 0 <= row[k] < vis, (i, b, s, k)
                assert all(row.count(c) == 1 for c in cands), (i, b, s)
                assert vis in row and inp["block_ids"].shape[1] * P in row  # the next row's token, a position past the table


def test_split_model_within_bars():
    """the kernel's arithmetic restated on the CPU, over list pieces of 64 .. 2048 slots: within the dense op's bars"""
    w_tau, w_lse = 0.0, 0.0
    for i in range(len(_CAL)):
        for inp, (ref, rlse) in (_cal_case(i), (_cal_case_fp8(i)[0], _cal_case_fp8(i)[3])):
            for R in sn.PIECE_LENS:
                if R > 64 and R >= 2 * inp["topk"]:
                    continue
                out, l = sn.split_model(inp, R)
                w_tau = max(w_tau, float(attn_rel_err(ref, out, 1).max()))
                w_lse = max(w_lse, sn.lse_err(rlse, l))
    print(f"\nsparse needle lists: split model worst out {w_tau:.5f} (tau {mn.TAU_NEEDLE} = {mn.TAU_NEEDLE / w_tau:.2f} x), "
          f"worst lse {w_lse:.3g} (bar {mn.LSE_BAR_NEEDLE} = {mn.LSE_BAR_NEEDLE / w_lse:.2f} x) over piece lengths {sn.PIECE_LENS}")
    assert w_tau <= mn.TAU_NEEDLE, w_tau
    assert w_lse <= mn.LSE_BAR_NEEDLE, w_lse


def _last_valid(valid):
    return [int(valid.nonzero().max())] if bool(valid.any()) else []


@pytest.mark.parametrize("i", range(len(_CAL)))
def test_needle_bar_rejects_mutants(i):
    """each mutant of a plausible bug, run through the statement, is >= 3 tau off the statement"""
    inp, (ref, _) = _cal_case(i)
    sq, B = inp["num_seq_q"], len(inp["lens_total"])
    R = B * sq
    mutants = {
        "the list ignored: dense over everything visible": sn.statement(inp, ignore_list=True)[0],
        "slot 63 dropped": sn.statement(inp, drop_slots=lambda v: [63])[0],
        "slot 64 dropped": sn.statement(inp, drop_slots=lambda v: [64])[0],
        "the last valid slot dropped": sn.statement(inp, drop_slots=_last_valid)[0],
        "entries >= vis not masked": sn.statement(inp, mask_vis=False)[0],
        "request b + 1's list": sn.statement(inp, list_row=lambda b, s: ((b + 1) % B) * sq + s)[0],
        "-1 read as token 0": sn.statement(inp, neg_as_zero=True)[0],
        "page translation skipped": sn.statement(inp, translate=False)[0],
        "RoPE columns ignored": sn.statement(inp, use_rope=False)[0],
    }
    if sq > 1:
        mutants["row s reads row s + 1's list"] = sn.statement(inp, list_row=lambda b, s: min(b * sq + s + 1, R - 1))[0]
    if inp["topk"] <= 64:
        del mutants["slot 64 dropped"]  # the list has no slot 64
    short = []
    for name, y in mutants.items():
        m = float(attn_rel_err(ref, y, 1).max()) / mn.TAU_NEEDLE
        print(f"  case {i} {name:55s} {m:9.1f} tau")
        if not m >= 3:
            short.append((name, m))
    assert not short, short


@pytest.mark.parametrize("i", range(len(_CAL) - 1))
def test_needle_bar_rejects_mutants_of_the_fp8_path(i):
    """the FP8 mutants of tests/test_attention_decode_mla_fp8.py, through the sparse statement"""
    inp, cache, orig, (ref, _) = _cal_case_fp8(i)
    codes, scales, rope = f8.unpack(cache)

    def deq(s):
        return f8.dequantise(f8.pack(codes, s.contiguous(), rope))

    mutants = {
        "scales ignored": sn.statement(dict(inp, ckv=deq(torch.ones_like(scales))))[0],
        "group g read with group g + 1's scale": sn.statement(dict(inp, ckv=deq(scales.roll(-1, -1))))[0],
        "a token read with its page neighbour's scale": sn.statement(dict(inp, ckv=deq(scales.roll(1, 1))))[0],
        "the unquantised bf16 values where the codes should be": sn.statement(orig)[0],
    }
    short = []
    for name, y in mutants.items():
        m = float(attn_rel_err(ref, y, 1).max()) / mn.TAU_NEEDLE
        print(f"  case {i} {name:55s} {m:9.1f} tau")
        if not m >= 3:
            short.append((name, m))
    assert not short, short


# ---- CPU 3: surface and fakes --------------------------------------------------------------------------------------------------
def test_surface():
    import hpc

    for name in ("attention_decode_mla_sparse_bf16", "attention_decode_mla_sparse_fp8"):
        assert name in hpc.__all__ and callable(getattr(hpc, name))
        doc = getattr(hpc, name).__doc__
        for word in ("indices", "int32 [B * Sq, topk]", "65536", "vis(b, s)", "-1 padding", "counts twice", "lse = -inf",
                     "no memory access", "tests/mla_sparse_ref.py", "splits", "release_decode_workspaces", "hipGraph",
                     "bit-identical", "H % 16 == 0", "mtp 0..3", "{16, 32, 64, 128}"):
            assert word in doc, (name, word)
    doc = hpc.attention_decode_mla_sparse_bf16.__doc__
    for word in ("LOGICAL token positions", "merge_attn_states", "plen = ceil(topk / splits)", "not launched", "no float atomics",
                 "attention_decode_mla_bf16 at splits = 1"):
        assert word in doc, word
    doc = hpc.attention_decode_mla_sparse_fp8.__doc__
    for word in ("656", "torch.uint8", "c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] )", "attention_decode_mla_fp8"):
        assert word in doc, word


@pytest.mark.parametrize("kind", OPS)
def test_fakes(kind):
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    fn = getattr(hpc, "attention_decode_mla_sparse_" + kind)
    raw = getattr(torch.ops.hpc_mla, "attention_decode_mla_sparse_" + kind)
    with FakeTensorMode():
        q = torch.empty(6, 32, DIM, dtype=torch.bfloat16, device="cuda")
        ckv = (torch.empty(9, 64, 656, dtype=torch.uint8, device="cuda") if kind == "fp8"
               else torch.empty(9, 64, DIM, dtype=torch.bfloat16, device="cuda"))
        bid = torch.empty(3, 4, dtype=torch.int32, device="cuda")
        lens = torch.empty(3, dtype=torch.int32, device="cuda")
        idx = torch.empty(6, 100, dtype=torch.int32, device="cuda")
        out, lse = raw(q, ckv, bid, lens, idx, 0.07, 1, False, None, None, True, 0)
        assert (out.shape, out.dtype, lse.shape, lse.dtype) == ((6, 32, DIM_V), torch.bfloat16, (6, 32), torch.float32)
        out, lse = raw(q, ckv, bid, lens, idx, 0.07, 1, False, None, None, False, 0)
        assert out.shape == (6, 32, DIM_V) and lse.numel() == 0
        y = fn(q, ckv, bid, lens, idx, 0.07, mtp=1)
        assert isinstance(y, torch.Tensor) and y.shape == (6, 32, DIM_V) and y.dtype == torch.bfloat16 and y.device.type == "cuda"
        y, l = fn(q, ckv, bid, lens, idx, 0.07, mtp=1, return_lse=True, splits=4)
        assert y.shape == (6, 32, DIM_V) and l.shape == (6, 32)
        o = torch.empty(6, 32, DIM_V, dtype=torch.bfloat16, device="cuda")
        ol = torch.empty(6, 32, dtype=torch.float32, device="cuda")
        assert fn(q, ckv, bid, lens, idx, 0.07, mtp=1, output=o) is o
        y, l = fn(q, ckv, bid, lens, idx, 0.07, mtp=1, output=o, output_lse=ol)
        assert y is o and l is ol
        y, l = fn(q, ckv, bid, lens, idx, 0.07, mtp=1, output_lse=ol)
        assert y.shape == (6, 32, DIM_V) and l is ol
        y, l = fn(q, ckv, bid, lens, idx, 0.07, mtp=1, output=o, return_lse=True)
        assert y is o and l.shape == (6, 32)


# ---- CPU 4: the route and the C-ABI ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def plan(lib, B, sq, H, topk, splits, cus):
    s, mx, ws, grid, narrow = c_int(-7), c_int(-7), c_int64(-7), c_int(-7), c_int(-7)
    rc = lib.hpc_attention_decode_mla_sparse_plan(B, sq, H, topk, splits, cus, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws),
                                                  ctypes.byref(grid), ctypes.byref(narrow))
    return rc, s.value, mx.value, ws.value, grid.value, narrow.value


def _route(B, sq, H, topk, wanted, cus):
    """the arithmetic of mla_route() (csrc/attention_decode_mla_route.h) in its sparse form, restated: (effective pieces, scratch
    bytes, grid, narrow)"""
    head_tiles = -(-H // 64)
    W = B * sq * head_tiles
    tiles = -(-topk // 64)
    cut = wanted if wanted > 0 else (1 if W >= cus else min(MAX_SPLITS, -(-2 * cus // W), tiles))
    plen = sn.list_piece_len(topk, cut)
    assert plen == -(-tiles // cut) * 64
    eff = -(-topk // plen)
    rows = B * sq * H
    return eff, (eff * rows * (DIM_V + 2) * 4 if eff > 1 else 0), W * eff, int(H == 16)


@pytest.mark.parametrize("B,sq,H,topk,cus", [(1, 1, 16, 2048, 256), (64, 1, 128, 2048, 256), (64, 1, 16, 2048, 256),
                                             (8, 2, 128, 2048, 256), (3, 4, 48, 65, 256), (5, 1, 32, 1, 304), (2, 2, 64, 320, 80),
                                             (1, 1, 16, 65536, 256), (7, 3, 80, 1000, 256), (300, 1, 16, 64, 256),
                                             # W one below, at and one above the CU count
                                             (255, 1, 16, 2048, 256), (256, 1, 16, 2048, 256), (257, 1, 16, 2048, 256),
                                             (79, 1, 64, 320, 80), (80, 1, 64, 320, 80), (81, 1, 64, 320, 80),
                                             (101, 3, 48, 1000, 304), (76, 2, 128, 2048, 304), (51, 3, 128, 1000, 305),
                                             # one tile, two tiles, and one slot either side: the effective count is clamped
                                             (3, 1, 16, 63, 256), (3, 1, 16, 64, 256), (3, 1, 16, 65, 256),
                                             (3, 2, 128, 127, 256), (3, 2, 128, 128, 256), (3, 2, 128, 129, 256)])
def test_plan_is_the_route(lib, B, sq, H, topk, cus):
    for wanted in (0, 1, 2, 3, 5, 8, 33, 64):
        rc, s, mx, ws, grid, narrow = plan(lib, B, sq, H, topk, wanted, cus)
        assert (rc, mx) == (0, MAX_SPLITS)
        assert (s, ws, grid, narrow) == _route(B, sq, H, topk, wanted, cus), (wanted, s, ws, grid, narrow)
        assert 1 <= s <= max(1, wanted or MAX_SPLITS) and (s - 1) * sn.list_piece_len(topk, max(wanted, s)) < topk
    # the effective count is a fixed point: asking for it gives the same plan again
    for wanted in (3, 7, 50):
        eff = plan(lib, B, sq, H, topk, wanted, cus)[1]
        assert plan(lib, B, sq, H, topk, eff, cus)[1:] == plan(lib, B, sq, H, topk, wanted, cus)[1:]


def test_plan_examples(lib):
    # topk 65: two tiles, so at most two pieces whatever is asked for
    assert plan(lib, 2, 1, 16, 65, 64, 256)[1] == 2 and plan(lib, 2, 1, 16, 65, 0, 256)[1] == 2
    # topk 2048 at 8 splits: pieces of 256 slots
    assert plan(lib, 2, 1, 16, 2048, 8, 256)[1] == 8
    # a full machine: one piece, no scratch
    assert plan(lib, 128, 1, 128, 2048, 0, 256)[1:4] == (1, MAX_SPLITS, 0)
    # half a machine (64 q rows x 2 head tiles on 256 CUs): four pieces
    assert plan(lib, 64, 1, 128, 2048, 0, 256)[1] == 4
    # the refusals of the plan
    assert plan(lib, 2, 1, 16, 0, 1, 256)[0] == INVALID and plan(lib, 2, 1, 16, -3, 1, 256)[0] == INVALID
    assert plan(lib, 2, 1, 16, MAX_TOPK + 1, 1, 256)[0] == UNSUPPORTED and plan(lib, 2, 1, 16, MAX_TOPK, 1, 256)[0] == 0
    assert plan(lib, 2, 1, 24, 64, 1, 256)[0] == UNSUPPORTED and plan(lib, 2, 5, 16, 64, 1, 256)[0] == UNSUPPORTED
    assert plan(lib, 2, 1, 16, 64, MAX_SPLITS + 1, 256)[0] == INVALID and plan(lib, -1, 1, 16, 64, 1, 256)[0] == INVALID


@pytest.mark.parametrize("B,H", [(1, 16), (3, 64), (5, 128), (64, 16), (300, 128)])
def test_a_list_cut_evenly_plans_as_the_dense_op(lib, B, H):
    """mtp 0 and a list of 65536 slots = 1024 tiles, which every count asked for here divides: the piece length is a whole
    number of tiles, no piece is dropped, and a q row is a request - so the sparse plan is the dense one (one route behind both)"""
    for wanted in (1, 2, 4, 8, 16, 32, 64):
        s, mx, ws = c_int(-7), c_int(-7), c_int64(-7)
        rc = lib.hpc_attention_decode_mla_plan(B, 1, H, wanted, 256, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws))
        assert rc == 0 and s.value == wanted
        assert plan(lib, B, 1, H, MAX_TOPK, wanted, 256)[:4] == (0, s.value, mx.value, ws.value), wanted


def call(lib, kind="bf16", *, out=4096, lse=4096, q=4096, ckv=4096, bid=4096, lens=4096, idx=4096, B=2, sq=1, H=16, topk=128, P=64,
         max_blocks=4, num_blocks=8, block_stride=None, token_stride=None, scale=0.07, nki=0, splits=1, ws=None, ws_bytes=0):
    """hpc_attention_decode_mla_sparse_{bf16,fp8}_async with pointers that are never dereferenced on the host; the cache's
    strides default to the kind's contiguous ones (bf16: elements, fp8: bytes)"""
    row = 656 if kind == "fp8" else DIM
    token_stride = row if token_stride is None else token_stride
    block_stride = P * row if block_stride is None else block_stride
    ip = ctypes.POINTER(c_int)
    fn = getattr(lib, f"hpc_attention_decode_mla_sparse_{kind}_async")
    return fn(c_void_p(out), c_void_p(lse), c_void_p(q), c_void_p(ckv), ctypes.cast(c_void_p(bid), ip),
              ctypes.cast(c_void_p(lens), ip), ctypes.cast(c_void_p(idx), ip), B, sq, H, topk, P, max_blocks, num_blocks,
              c_int64(block_stride), c_int64(token_stride), c_float(scale), nki, splits, c_void_p(ws) if ws else None,
              c_int64(ws_bytes), None)


UNSUPPORTED, INVALID = -1, -2


@pytest.mark.parametrize("kind", OPS)
@pytest.mark.parametrize("kwargs,code", [
    # the dense launchers' table
    (dict(H=8), UNSUPPORTED), (dict(H=24), UNSUPPORTED), (dict(H=144), UNSUPPORTED), (dict(sq=5), UNSUPPORTED),
    (dict(P=48), UNSUPPORTED), (dict(P=8), UNSUPPORTED), (dict(P=256), UNSUPPORTED), (dict(P=0), UNSUPPORTED),
    (dict(ckv=4096 + 8), UNSUPPORTED), (dict(q=4096 + 2), UNSUPPORTED), (dict(out=4096 + 4), UNSUPPORTED),
    (dict(max_blocks=1 << 26), UNSUPPORTED), (dict(B=0, P=48), UNSUPPORTED),
    (dict(splits=MAX_SPLITS + 1), INVALID), (dict(splits=-1), INVALID), (dict(B=-1), INVALID), (dict(sq=0), INVALID),
    (dict(sq=-1), INVALID), (dict(H=-16), INVALID), (dict(max_blocks=-1), INVALID),
    (dict(out=0), INVALID), (dict(q=0), INVALID), (dict(ckv=0), INVALID), (dict(bid=0), INVALID), (dict(lens=0), INVALID),
    (dict(splits=2, ws=None), INVALID), (dict(splits=2, ws=4096 + 4, ws_bytes=1 << 30), UNSUPPORTED),
    # the list's
    (dict(idx=0), INVALID), (dict(topk=0), INVALID), (dict(topk=-1), INVALID), (dict(num_blocks=-1), INVALID),
    (dict(topk=MAX_TOPK + 1), UNSUPPORTED), (dict(idx=4096 + 2), UNSUPPORTED),
    # two faults: the earlier check's code
    (dict(H=8, topk=0), INVALID), (dict(topk=MAX_TOPK + 1, splits=MAX_SPLITS + 1), UNSUPPORTED), (dict(B=0, topk=0), INVALID),
])
def test_cabi_refuses_on_the_host(lib, kind, kwargs, code):
    assert call(lib, kind, **kwargs) == code


@pytest.mark.parametrize("kind,row", [("bf16", DIM), ("fp8", 656)])
def test_cabi_refuses_bad_strides_and_takes_an_empty_batch(lib, kind, row):
    unit = 8 if kind == "bf16" else 16
    assert call(lib, kind, token_stride=row - 1) == UNSUPPORTED and call(lib, kind, token_stride=row + unit // 2) == UNSUPPORTED
    assert call(lib, kind, block_stride=64 * row + unit // 2) == UNSUPPORTED and call(lib, kind, token_stride=-row) == UNSUPPORTED
    assert call(lib, kind, block_stride=-64 * row) == INVALID and call(lib, kind, H=8, block_stride=-64 * row) == INVALID
    # accepted up to the device call: an empty batch returns 0 without one, whatever the list's length
    for kw in (dict(), dict(token_stride=row + unit, block_stride=64 * (row + unit)), dict(topk=1), dict(topk=MAX_TOPK), dict(num_blocks=0)):
        assert call(lib, kind, B=0, **kw) == 0
    rc, s, _, need, _, _ = plan(lib, 2, 1, 16, 128, 2, 256)
    assert (rc, s) == (0, 2) and need > 0
    assert call(lib, kind, splits=2, ws=4096, ws_bytes=need - 1) == INVALID
    assert call(lib, kind, max_blocks=0) == INVALID  # a batch with work and no page table


def test_both_libraries_export_the_launchers():
    pkg = Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc"
    for name in ("libhpc_amd.so", "libhpc_amd_dev.so"):
        so = ctypes.CDLL(str(pkg / name))
        for sym in ("hpc_attention_decode_mla_sparse_plan", "hpc_attention_decode_mla_sparse_bf16_async",
                    "hpc_attention_decode_mla_sparse_fp8_async"):
            assert hasattr(so, sym), (name, sym)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _lens(inp, nki):
    return (inp["lens_total"] if nki else inp["lens_before"]).cuda()


def _run(kind, inp, cache, splits=0, nki=False, indices=None, **kw):
    """the sparse op of `kind` on `cache` (a CUDA tensor of the kind's dtype)"""
    import hpc

    fn = getattr(hpc, "attention_decode_mla_sparse_" + kind)
    idx = inp["indices"] if indices is None else indices
    return fn(inp["q"].cuda(), cache, inp["block_ids"].cuda(), _lens(inp, nki), idx.cuda(), inp["scale"],
              mtp=inp["num_seq_q"] - 1, new_kv_included=nki, return_lse=True, splits=splits, **kw)


def _dense(kind, inp, cache, splits):
    import hpc

    fn = getattr(hpc, "attention_decode_mla_" + kind)
    return fn(inp["q"].cuda(), cache, inp["block_ids"].cuda(), inp["lens_before"].cuda(), inp["scale"],
              mtp=inp["num_seq_q"] - 1, return_lse=True, splits=splits)


def _fill_scratch_with_nan():
    import hpc  # noqa: F401  (registers the ops)

    for ws in torch.ops.hpc_mla._workspaces():
        ws.fill_(0xFF)  # every float of it a NaN


def _caches(orig, seed):
    """{kind: (inputs whose ckv is what the kind's op sees dequantised, the kind's cache on the GPU)}: the bf16 op runs on the
    FP8 cache's dequantisation, so that both kinds have one statement"""
    cache = f8.quantise(orig["ckv"], vary_seed=seed)
    inp = dict(orig, ckv=f8.dequantise(cache))
    return inp, {"bf16": inp["ckv"].cuda(), "fp8": cache.cuda()}


def _check(ref, rlse, out, lse, label, tau=mn.TAU_NEEDLE, bar=mn.LSE_BAR_NEEDLE):
    w_out, w_lse = float(attn_rel_err(ref, out.cpu(), 1).max()), sn.lse_err(rlse, lse)
    print(f"{label}: out worst {w_out:.5f} (tau {tau}), lse worst {w_lse:.3g} (bar {bar})")
    assert attn_close(ref, out.cpu(), tau, 1, label=label)
    assert w_lse <= bar, (label, w_lse, bar)


# (H, mtp, P, topk): narrow, one tile / a partly filled head tile / causal, pages of 16 / two head tiles, the models' topk /
# mtp 3, a list one slot past a tile
_CONFIGS = [(16, 0, 64, 64), (48, 0, 32, 320), (64, 1, 16, 128), (128, 1, 64, 2048), (32, 3, 128, 65)]
_LENS = [0, 1, 63, 64, 65, 300, 2100, 5000]


@functools.lru_cache(maxsize=None)
def _needle_case(H, mtp, P, topk):
    """one configuration (B = 8): inputs over the dequantised cache, both caches, the statement - computed once"""
    inp, caches = _caches(sn.sparse_needle_inputs(_LENS, mtp + 1, P, H, topk, seed=300 + H), VARY_SEED + H)
    return inp, caches, sn.statement(inp)


@pytest.mark.gpu
@pytest.mark.parametrize("H,mtp,P,topk", _CONFIGS)
def test_needle_parity(H, mtp, P, topk):
    """both ops against the float64 statement at every split count; the FP8 op bit-equal to the bf16 op on the dequantised cache"""
    inp, caches, (ref, rlse) = _needle_case(H, mtp, P, topk)
    for splits in (0, 1, 3, 8):
        _fill_scratch_with_nan()
        got = {kind: _run(kind, inp, caches[kind], splits) for kind in OPS}
        for kind in OPS:
            out, lse = got[kind]
            assert out.dtype == torch.bfloat16 and lse.dtype == torch.float32 and out.shape == (8 * (mtp + 1), H, DIM_V)
            _check(ref, rlse, out, lse, f"{kind} H {H} mtp {mtp} P {P} topk {topk} splits {splits}")
        assert torch.equal(got["fp8"][0].view(torch.int16), got["bf16"][0].view(torch.int16)), splits
        assert torch.equal(got["fp8"][1].view(torch.int32), got["bf16"][1].view(torch.int32)), splits
    if (H, mtp, P) == (64, 1, 16):  # the lengths given the other way
        for kind in OPS:
            a, b = _run(kind, inp, caches[kind], 3), _run(kind, inp, caches[kind], 3, nki=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
@pytest.mark.parametrize("H", [16, 48])
def test_identity_lists_are_the_dense_op_bit_for_bit(kind, H):
    """mtp 0, splits 1, indices[b] = 0 .. L_b - 1 then -1: out and lse are the dense op's at splits 1, narrow and wide form"""
    P = 32
    orig = mn.needle_inputs([0, 1, 63, 64, 65, 700, 1500], 1, P, H, seed=5)
    inp, caches = _caches(orig, VARY_SEED + 1)
    L = inp["lens_total"]
    for topk in (int(L.max()), int(L.max()) + 77):
        idx = torch.arange(topk, dtype=torch.int32)[None, :].repeat(len(L), 1)
        idx[idx >= L[:, None]] = -1
        out, lse = _run(kind, inp, caches[kind], 1, indices=idx)
        dout, dlse = _dense(kind, inp, caches[kind], 1)
        assert torch.equal(out.view(torch.int16), dout.view(torch.int16)), (kind, H, topk)
        assert torch.equal(lse.view(torch.int32), dlse.view(torch.int32)), (kind, H, topk)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
def test_a_permuted_list_stays_within_the_bars(kind):
    H, mtp, P, topk = 48, 0, 32, 320
    inp, caches, (ref, rlse) = _needle_case(H, mtp, P, topk)
    g = torch.Generator().manual_seed(3)
    idx = torch.stack([row[torch.randperm(topk, generator=g)] for row in inp["indices"]])
    assert not torch.equal(idx, inp["indices"])
    for splits in (1, 3):
        out, lse = _run(kind, inp, caches[kind], splits, indices=idx)
        _check(ref, rlse, out, lse, f"{kind} permuted splits {splits}")


def _tiny(H, sq, P, B, g):
    """a pool of 2 B + 1 pages, one page per request, every request with its sq new tokens only"""
    cache = f8.quantise(torch.randn(2 * B + 1, P, DIM, generator=g).bfloat16(), vary_seed=7)
    bid = torch.randperm(2 * B + 1, generator=g)[:B].to(torch.int32).reshape(B, 1)
    q = torch.randn(B * sq, H, DIM, generator=g).bfloat16()
    inp = dict(q=q, block_ids=bid, lens_before=torch.full((B,), P - sq, dtype=torch.int32),
               lens_total=torch.full((B,), P, dtype=torch.int32), num_seq_q=sq, scale=mn.SCALE, ckv=f8.dequantise(cache))
    return inp, {"bf16": inp["ckv"].cuda(), "fp8": cache.cuda()}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
@pytest.mark.parametrize("splits", [1, 2, 8])
def test_one_valid_entry_is_the_cached_row_and_twice_adds_ln2(kind, splits):
    g = torch.Generator().manual_seed(splits)
    for H, sq, P, topk in ((16, 1, 64, 200), (64, 2, 16, 515)):
        B = 3
        inp, caches = _tiny(H, sq, P, B, g)
        R = B * sq
        pos = torch.randint(0, P - sq, (R,), generator=g)  # visible to every row
        slot = torch.tensor([0, topk - 1, 64, 63, 130, topk // 2][:R])
        idx = torch.full((R, topk), -1, dtype=torch.int32)
        idx[:, 7::13] = P + 5   # beyond the table
        idx[:, 3::17] = P - 1   # the last new token: at or past vis for every row but the last of a request
        idx[sq - 1::sq, 3::17] = -9
        idx[torch.arange(R), slot] = pos.to(torch.int32)
        _fill_scratch_with_nan()
        out, lse = _run(kind, inp, caches[kind], splits, indices=idx)
        want = inp["ckv"][inp["block_ids"][:, 0].long().repeat_interleave(sq), pos, :DIM_V]
        assert torch.equal(out.cpu(), want[:, None, :].expand(R, H, DIM_V)), (H, sq, P)
        _, rlse = sr.sparse_statement(inp["q"], inp["ckv"], inp["block_ids"], inp["lens_total"], idx, sq, inp["scale"])
        assert sn.lse_err(rlse, lse) <= mn.LSE_BAR_NEEDLE
        # the same entry listed twice, the copy in another tile: the same row, lse larger by ln 2
        idx2 = idx.clone()
        idx2[torch.arange(R), (slot + 70) % topk] = pos.to(torch.int32)
        _fill_scratch_with_nan()
        out2, lse2 = _run(kind, inp, caches[kind], splits, indices=idx2)
        assert torch.equal(out2, out)
        assert float((lse2.double().cpu() - lse.double().cpu() - math.log(2.0)).abs().max()) <= mn.LSE_BAR_NEEDLE


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
@pytest.mark.parametrize("splits", [1, 4])
def test_an_all_invalid_row_is_zeros_and_minus_inf(kind, splits):
    g = torch.Generator().manual_seed(9)
    for H, sq, P, topk in ((16, 1, 64, 300), (80, 2, 32, 257)):
        B = 3
        inp, caches = _tiny(H, sq, P, B, g)
        R = B * sq
        idx = torch.full((R, topk), -1, dtype=torch.int32)
        idx[:, 1::3] = P        # past the length and the table
        idx[:, 2::5] = -2 ** 31
        idx[:, 4::7] = 2 ** 31 - 1
        idx[R - 1, 100] = 3     # the last row sees one token; every other row none
        out = torch.full((R, H, DIM_V), 7.0, dtype=torch.bfloat16, device="cuda")
        lse = torch.full((R, H), 7.0, dtype=torch.float32, device="cuda")
        _fill_scratch_with_nan()
        _run(kind, inp, caches[kind], splits, indices=idx, output=out, output_lse=lse)
        assert not bool(out.float().isnan().any()) and not bool(lse.isnan().any())
        assert bool((out[: R - 1] == 0).all()) and bool((lse[: R - 1] == float("-inf")).all())
        want = inp["ckv"][int(inp["block_ids"][B - 1, 0]), 3, :DIM_V]
        assert torch.equal(out[R - 1].cpu(), want[None, :].expand(H, DIM_V)) and bool(torch.isfinite(lse[R - 1]).all())


@functools.lru_cache(maxsize=None)
def _forced_case(topk):
    inp, caches = _caches(sn.sparse_needle_inputs([5, 64, 65, 700, 5000], 1, 64, 16, topk, seed=9), VARY_SEED + 2)
    return inp, caches, sn.statement(inp)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
@pytest.mark.parametrize("topk,splits", [(1000, 1), (1000, 3), (1000, 64), (65, 64), (65, 3)])
def test_forced_splits_over_nan_scratch(kind, topk, splits):
    """topk 65 has two tiles: whatever is asked for, two pieces run and the rest are not launched; the scratch holds NaN bytes
    before each call, so a read of an unwritten piece shows"""
    inp, caches, (ref, rlse) = _forced_case(topk)
    _run(kind, inp, caches[kind], MAX_SPLITS)  # the scratch exists at its largest
    _fill_scratch_with_nan()
    out, lse = _run(kind, inp, caches[kind], splits)
    _check(ref, rlse, out, lse, f"{kind} topk {topk} forced splits {splits}")


@pytest.mark.gpu
def test_strided_caches_are_bit_equal_to_the_contiguous_one():
    P, H, sq, topk = 32, 48, 2, 200
    inp, caches = _caches(sn.sparse_needle_inputs([0, 31, 33, 700, 1500], sq, P, H, topk, seed=21), VARY_SEED + 3)
    pool = caches["fp8"].shape[0]
    views = {}
    for kind, (row, pad, dt, fill) in {"bf16": (DIM, DIM + 24, torch.bfloat16, -3.0), "fp8": (656, 704, torch.uint8, 0xA5)}.items():
        padded = torch.full((pool, P, pad), fill, dtype=dt, device="cuda")
        big = torch.full((pool + 2, P + 3, pad), fill, dtype=dt, device="cuda")
        views[kind] = {"padded": padded[:, :, :row], "pool": big[1:-1, 2: 2 + P, :row]}
        for v in views[kind].values():
            assert not v.is_contiguous()
            v.copy_(caches[kind])
    for kind in OPS:
        for splits in (1, 3):
            a, la = _run(kind, inp, caches[kind], splits)
            for name, v in views[kind].items():
                b, lb = _run(kind, inp, v, splits)
                assert torch.equal(a, b) and torch.equal(la, lb), (kind, name, splits)
    ref, rlse = sn.statement(inp)
    _check(ref, rlse, b, lb, "strided")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
@pytest.mark.parametrize("splits", [1, 4])
def test_twenty_calls_are_bit_identical(kind, splits):
    inp, caches = _caches(sn.sparse_needle_inputs([3, 700, 2100], 2, 64, 32, 500, seed=4), VARY_SEED + 4)
    first = _run(kind, inp, caches[kind], splits)
    for _ in range(19):
        _fill_scratch_with_nan()
        again = _run(kind, inp, caches[kind], splits)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
def test_graph_replays_after_lengths_pages_cache_and_indices_changed_in_place(kind):
    """capture on one stream with every output given; replay; change everything in place; replay: the new result"""
    import hpc

    fn = getattr(hpc, "attention_decode_mla_sparse_" + kind)
    H, sq, P, topk = 16, 1, 64, 256
    a = sn.sparse_needle_inputs([700, 64, 3000, 5], sq, P, H, topk, seed=31)
    b = sn.sparse_needle_inputs([65, 2000, 1, 900], sq, P, H, topk, seed=32)
    pool, cols = max(a["ckv"].shape[0], b["ckv"].shape[0]), max(a["block_ids"].shape[1], b["block_ids"].shape[1])

    def padded(orig, seed):  # the case's pool inside the graph's pool, the rest poison
        full = torch.full((pool, P, DIM), mn.POISON, dtype=torch.bfloat16)
        full[: orig["ckv"].shape[0]] = orig["ckv"]
        bid = torch.full((4, cols), sn.PAD_PAGE, dtype=torch.int32)
        bid[:, : orig["block_ids"].shape[1]] = orig["block_ids"]
        cache = f8.quantise(full, vary_seed=seed)
        inp = dict(orig, ckv=f8.dequantise(cache), block_ids=bid)
        return inp, (cache if kind == "fp8" else inp["ckv"])

    cases = [padded(a, VARY_SEED + 5), padded(b, VARY_SEED + 6)]
    ckv = torch.zeros_like(cases[0][1], device="cuda")
    bid = torch.full((4, cols), sn.PAD_PAGE, dtype=torch.int32, device="cuda")
    q = torch.zeros(4 * sq, H, DIM, dtype=torch.bfloat16, device="cuda")
    lens = torch.zeros(4, dtype=torch.int32, device="cuda")
    idx = torch.full((4 * sq, topk), -1, dtype=torch.int32, device="cuda")
    out = torch.zeros(4 * sq, H, DIM_V, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(4 * sq, H, dtype=torch.float32, device="cuda")

    def load(case):
        inp, cache = case
        ckv.copy_(cache)
        bid.copy_(inp["block_ids"])
        q.copy_(inp["q"])
        lens.copy_(inp["lens_before"])
        idx.copy_(inp["indices"])

    def step():
        return fn(q, ckv, bid, lens, idx, mn.SCALE, output=out, output_lse=lse, splits=4)

    load(cases[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y, l = step()
        assert y is out and l is lse
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_allocated()
        step()
        grown = torch.cuda.memory_allocated() - before
    ws_bytes = sum(w.numel() for w in torch.ops.hpc_mla._workspaces())
    assert grown <= ws_bytes, (grown, ws_bytes)  # nothing allocated in the capture beyond the cached scratch
    for case in (cases[0], cases[1], cases[0]):
        load(case)
        out.zero_()
        lse.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref, rlse = sn.statement(case[0])
        _check(ref, rlse, out, lse, f"{kind} graph")
    del graph
    hpc.release_decode_workspaces()
    assert len(torch.ops.hpc_mla._workspaces()) == 0


GUARD, PATTERN = 1 << 20, 0xA5


@pytest.mark.gpu
@pytest.mark.parametrize("kind", OPS)
def test_guard_bands_through_the_cabi(lib, kind):
    """out, lse and a workspace of exactly the planned bytes, each between 1 MiB guard bands: the bands are intact afterwards"""
    H, mtp, splits, topk = 48, 1, 5, 300
    sq, P = mtp + 1, 64
    inp, caches = _caches(sn.sparse_needle_inputs([5, 64, 700, 1500], sq, P, H, topk, seed=17), VARY_SEED + 7)
    B, rows = 4, 4 * sq * H
    rc, s, _, ws_bytes, grid, narrow = plan(lib, B, sq, H, topk, splits, 0)
    assert (rc, s, narrow) == (0, 5, 0) and ws_bytes == s * rows * (DIM_V + 2) * 4 and grid == B * sq * s
    sizes = [rows * DIM_V * 2, rows * 4, ws_bytes]
    bufs = [torch.full((2 * GUARD + n,), PATTERN, dtype=torch.uint8, device="cuda") for n in sizes]
    bufs[2][GUARD: GUARD + ws_bytes] = 0xFF
    q, ckv, bid, lens, idx = (inp["q"].cuda(), caches[kind], inp["block_ids"].cuda(), inp["lens_before"].cuda(),
                              inp["indices"].cuda())
    torch.cuda.synchronize()
    rc = call(lib, kind, out=bufs[0].data_ptr() + GUARD, lse=bufs[1].data_ptr() + GUARD, q=q.data_ptr(), ckv=ckv.data_ptr(),
              bid=bid.data_ptr(), lens=lens.data_ptr(), idx=idx.data_ptr(), B=B, sq=sq, H=H, topk=topk, P=P,
              max_blocks=bid.shape[1], num_blocks=ckv.shape[0], block_stride=ckv.stride(0), token_stride=ckv.stride(1),
              scale=mn.SCALE, splits=splits, ws=bufs[2].data_ptr() + GUARD, ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in zip(bufs, sizes):
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all())
    out = bufs[0][GUARD: GUARD + sizes[0]].view(torch.bfloat16).reshape(B * sq, H, DIM_V)
    lse = bufs[1][GUARD: GUARD + sizes[1]].view(torch.float32).reshape(B * sq, H)
    ref, rlse = sn.statement(inp)
    _check(ref, rlse, out, lse, f"{kind} guards")


@pytest.mark.gpu
def test_empty_batch_and_refusals():
    import hpc

    ckv8 = torch.zeros(2, 64, 656, dtype=torch.uint8, device="cuda")
    ckv16 = torch.zeros(2, 64, DIM, dtype=torch.bfloat16, device="cuda")
    for fn, ckv, other in ((hpc.attention_decode_mla_sparse_bf16, ckv16, ckv8), (hpc.attention_decode_mla_sparse_fp8, ckv8, ckv16)):
        q = torch.empty(0, 16, DIM, dtype=torch.bfloat16, device="cuda")
        bid = torch.empty(0, 1, dtype=torch.int32, device="cuda")
        lens = torch.empty(0, dtype=torch.int32, device="cuda")
        out, lse = fn(q, ckv, bid, lens, torch.empty(0, 64, dtype=torch.int32, device="cuda"), mn.SCALE, return_lse=True)
        assert out.shape == (0, 16, DIM_V) and out.dtype == torch.bfloat16 and lse.shape == (0, 16)
        q1 = torch.zeros(1, 16, DIM, dtype=torch.bfloat16, device="cuda")
        one = (torch.zeros(1, 1, dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda"))
        idx = torch.zeros(1, 64, dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError, match="ckv_cache dtype must be"):
            fn(q1, other, *one, idx, mn.SCALE)
        with pytest.raises(RuntimeError, match="indices dtype must be int32"):
            fn(q1, ckv, *one, idx.long(), mn.SCALE)
        with pytest.raises(RuntimeError, match="indices must be a contiguous tensor of shape"):
            fn(q1, ckv, *one, idx.repeat(2, 1), mn.SCALE)
        with pytest.raises(RuntimeError, match="indices must be a contiguous tensor of shape"):
            fn(q1, ckv, *one, idx[0], mn.SCALE)
        with pytest.raises(RuntimeError, match="indices must be a contiguous tensor of shape"):
            fn(q1, ckv, *one, idx.repeat(1, 2)[:, ::2], mn.SCALE)
        with pytest.raises(RuntimeError, match="topk"):
            fn(q1, ckv, *one, idx[:, :0], mn.SCALE)
        with pytest.raises(RuntimeError, match="topk"):
            fn(q1, ckv, *one, torch.zeros(1, MAX_TOPK + 1, dtype=torch.int32, device="cuda"), mn.SCALE)
        with pytest.raises(RuntimeError, match="indices must be a cuda tensor"):
            fn(q1, ckv, *one, idx.cpu(), mn.SCALE)
        with pytest.raises(RuntimeError, match="splits"):
            fn(q1, ckv, *one, idx, mn.SCALE, splits=MAX_SPLITS + 1)
        with pytest.raises(RuntimeError, match="num_head"):
            fn(q1[:, :8], ckv, *one, idx, mn.SCALE)
        with pytest.raises(RuntimeError, match="block_size"):
            fn(q1, ckv[:, :48], *one, idx, mn.SCALE)
        with pytest.raises(RuntimeError, match="mtp"):
            fn(q1, ckv, *one, idx, mn.SCALE, mtp=4)
