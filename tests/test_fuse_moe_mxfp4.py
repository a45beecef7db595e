"""hpc.fuse_moe_mxfp4 - the fused MoE on MXFP4 expert weights - held to its own stages: count/slot, gate-up GEMM, activation +
128-block quantisation, down GEMM and reduce called one by one through the C ABI with the arguments csrc/fuse_moe.hip::fuse_moe
passes give the fused op's output BIT FOR BIT, and on exact GEMM inputs (tests/mxfp4_ref.py::moe_inputs) the chain's gate-up
matrix is the CPU statement's, bit for bit.  A hipGraph of the op with `output` given replays onto new routing.  CPU: the statement
of the fused op rejects swapped gate / up halves."""
import ctypes

import pytest
import torch

import mxfp4_ref as mr

F8 = torch.float8_e4m3fn
GUARD_ROWS, SENTINEL = 16, -7.0
# (T, E total, topk, rank_ep, size_ep, H, inter, shared)
MOE_CASES = [(T, 8, 2, rank, size, H, I, shared)
             for T in (1, 7, 33) for (H, I) in ((256, 128), (384, 256)) for (rank, size, shared) in ((0, 1, False), (1, 2, True))]
MOE_CASES += [(7, 8, 2, 0, 2, 256, 128, True), (33, 8, 2, 0, 1, 384, 256, True)]  # rank 0 of 2; shared output on every expert local


def _id(c):
    return "T%d-E%d-top%d-rank%dof%d-H%d-I%d%s" % (c[:7] + ("-shared" if c[7] else "",))


def _gate_up_statement(a, rank_ep):
    sl, cu, row_index, _ = mr.slots(a.ids, rank_ep, a.el)
    _, _, parts = mr.gemm_ref(a.x, a.xs, a.guw, a.gus, sl.tolist(), cu, rows=row_index)
    tot, flagged, _ = mr.chain(parts, a.xs[row_index.long()])
    assert flagged == 0
    return sl, row_index, tot.float().bfloat16()


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_slots_are_stable_arrival_order():
    ids = torch.tensor([[0, 3], [3, 5], [1, 3], [4, 7]], dtype=torch.int32)
    sl, cu, row_index, pos = mr.slots(ids, 1, 4)  # local experts 4 ... 7
    assert sl.tolist() == [1, 1, 0, 1] and cu.tolist() == [0, 1, 2, 2, 3]
    assert row_index.tolist() == [3, 1, 3] and pos.tolist() == [[-1, -1], [-1, 1], [-1, -1], [0, 2]]


def test_statement_rejects_swapped_halves():
    """the gate-up matrix is held to the statement bit for bit: one with its halves swapped differs nearly everywhere, and so
    does the fused statement's output"""
    a = mr.moe_inputs(7, 8, 2, 0, 1, 256, 128, False)
    y, gate_up = mr.fuse_moe_ref(a.x, a.xs, a.guw, a.gus, a.dw, a.ds, a.ids, a.sc, 0)
    bad_y, _ = mr.fuse_moe_ref(a.x, a.xs, a.guw, a.gus, a.dw, a.ds, a.ids, a.sc, 0, swap_halves=True)
    assert torch.equal(_gate_up_statement(a, 0)[2].view(torch.int16), gate_up.view(torch.int16))
    swapped = torch.cat([gate_up[:, 128:], gate_up[:, :128]], dim=1)
    assert float((swapped.view(torch.int16) != gate_up.view(torch.int16)).double().mean()) > 0.9
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert float(((bad_y - y).abs() > 0.01 * y.abs().max()).double().mean()) > 0.5


def test_workspace_and_refusals():
    from hpc import _C

    lib = _C.lib
    for args in ((7, 2, 256, 256, 8), (33, 8, 4096, 22016, 64)):
        assert lib.hpc_fuse_moe_mxfp4_workspace_bytes(*args) == lib.hpc_fuse_moe_blockwise_workspace_bytes(*args) > 0
    p = ctypes.c_void_p(4096)
    ok = [p] * 10 + [None, 7, 256, 256, 2, 8, 0, None]
    fn = lib.hpc_fuse_moe_mxfp4_async
    for i in range(10):
        args = list(ok)
        args[i] = None
        assert fn(*args) == -2, i
    for i, v in ((12, 192), (13, 128), (14, 129)):  # hidden % 128, intermediate_size2 % 256, num_topk > 128
        args = list(ok)
        args[i] = v
        assert fn(*args) == -1, i
    args = list(ok)
    args[11] = 0
    assert fn(*args) == 0  # no tokens: nothing to launch


# ---------------------------------------------------------------------------------------------------------------------- GPU
def _dev(a):
    return [t.cuda() if t is not None else None for t in (a.x, a.xs, a.guw, a.gus, a.dw, a.ds, a.ids, a.sc, a.so)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MOE_CASES, ids=_id)
def test_fuse_moe_mxfp4_equals_its_stages(case):
    import hpc
    from hpc import _C

    lib, p = _C.lib, _C.ptr
    T, E, topk, rank_ep, size_ep, H, inter, shared = case
    a = mr.moe_inputs(*case)
    el, m = a.el, T * topk
    xd, xsd, guwd, gusd, dwd, dsd, idsd, scd, sod = _dev(a)
    fused = hpc.fuse_moe_mxfp4(xd, xsd, guwd, gusd, dwd, dsd, idsd, scd, rank_ep, E, shared_output=sod)
    torch.cuda.synchronize()

    i32, st = dict(dtype=torch.int32, device="cuda"), _C.stream_of(xd)
    seqlens, cu, tiles, cu_tiles = torch.empty(el, **i32), torch.empty(el + 1, **i32), torch.empty(el, **i32), torch.empty(el + 1, **i32)
    pos, row_index = torch.empty(T, topk, **i32), torch.zeros(m, **i32)
    gate_up = torch.full((m + GUARD_ROWS, 2 * inter), SENTINEL, dtype=torch.bfloat16, device="cuda")
    down_in = torch.zeros((m, inter), dtype=torch.uint8, device="cuda")
    down_in_scale = torch.zeros((m, inter // 128), dtype=torch.float32, device="cuda")
    down_out = torch.full((m + GUARD_ROWS, H), SENTINEL, dtype=torch.bfloat16, device="cuda")
    y = torch.empty((T, H), dtype=torch.bfloat16, device="cuda")
    assert lib.hpc_moe_count_and_slot_async(p(idsd), T, topk, el, rank_ep, 128, p(seqlens), p(cu), p(tiles), p(cu_tiles), p(pos),
                                            p(row_index), st) == 0
    assert lib.hpc_group_gemm_mxfp4_async(p(gate_up), p(xd), p(xsd), p(guwd), p(gusd), p(seqlens), p(cu), p(row_index), el, m, T, 2 * inter,
                                          H, st) == 0
    num_rows = ctypes.c_void_p(cu.data_ptr() + 4 * el)
    assert lib.hpc_act_mul_and_blockwise_quant_async(p(down_in), p(down_in_scale), p(gate_up), num_rows, m, inter, inter // 128, 1, None,
                                                     st) == 0
    assert lib.hpc_group_gemm_mxfp4_async(p(down_out), p(down_in), p(down_in_scale), p(dwd), p(dsd), p(seqlens), p(cu), None, el, m, m, H,
                                          inter, st) == 0
    assert lib.hpc_moe_reduce_async(p(y), p(down_out), p(pos), p(scd), p(sod), T, topk, H, st) == 0
    torch.cuda.synchronize()

    sl, rows, want_gate_up = _gate_up_statement(a, rank_ep)
    total = int(sl.sum())
    assert torch.equal(seqlens.cpu(), sl) and torch.equal(row_index.cpu()[:total], rows)
    got = gate_up.cpu()
    differ = int((got[:total].view(torch.int16) != want_gate_up.view(torch.int16)).sum())
    fused_differ = int((fused.view(torch.int16) != y.view(torch.int16)).sum())
    print(f"fused MoE {_id(case)}: {total} routed rows of {m}; gate-up matrix: {differ}/{total * 2 * inter} outputs differ from the "
          f"statement; fused op against its stages: {fused_differ}/{y.numel()} outputs differ")
    assert bool((got[m:] == SENTINEL).all()) and bool((down_out[m:] == SENTINEL).all()), "rows behind m were written"
    assert differ == 0
    assert bool(torch.isfinite(y.float()).all()) and (total == 0 or shared or float(y.float().abs().max()) > 0)
    assert fused_differ == 0
    # and the fused statement: the device's activation differs from the model's by its hardware exponential, so the output is held
    # to it only loosely here (the bits are the stages') - a percent of the largest output
    ref = mr.fuse_moe_ref(a.x, a.xs, a.guw, a.gus, a.dw, a.ds, a.ids, a.sc, rank_ep, a.so)[0]
    assert float((fused.cpu().double() - ref).abs().max()) <= 0.02 * max(float(ref.abs().max()), 1.0)


@pytest.mark.gpu
def test_fuse_moe_mxfp4_graph_replay_with_new_routing():
    """captured with `output` given, replayed after the routing (ids and weights of the top-k) changed in place: every replay
    equals an eager call on the same inputs"""
    import hpc

    case = (33, 8, 2, 0, 1, 256, 128, True)
    a, b = mr.moe_inputs(*case), mr.moe_inputs(*case, seed=7)
    xd, xsd, guwd, gusd, dwd, dsd, idsd, scd, sod = _dev(a)
    out = torch.full((33, 256), SENTINEL, dtype=torch.bfloat16, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture, as torch asks
        hpc.fuse_moe_mxfp4(xd, xsd, guwd, gusd, dwd, dsd, idsd, scd, 0, 8, shared_output=sod, output=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hpc.fuse_moe_mxfp4(xd, xsd, guwd, gusd, dwd, dsd, idsd, scd, 0, 8, shared_output=sod, output=out)
    for inputs in (a, b, a):
        idsd.copy_(inputs.ids)
        scd.copy_(inputs.sc)
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        eager = hpc.fuse_moe_mxfp4(xd, xsd, guwd, gusd, dwd, dsd, idsd, scd, 0, 8, shared_output=sod)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
    assert not torch.equal(a.ids, b.ids)
