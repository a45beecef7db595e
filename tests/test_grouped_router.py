"""Group-limited top-k router (hpc.grouped_topk_router, DeepSeek-V3 style routing) against its PyTorch statement
(tests/grouped_router_ref.py): exact indices wherever the inputs decide them, weights at the bar of tests/test_router.py,
refusals of the C entry, the fake, and the chain router GEMM -> router -> fused MoE."""
import ctypes
import functools
from pathlib import Path

import pytest
import torch

import grouped_router_ref as gref
from utils import allclose

ROOT = Path(__file__).resolve().parent.parent
F8 = torch.float8_e4m3fn


# ---- CPU: the definition ------------------------------------------------------------------------------------------------
def test_helper_without_groups_is_the_plain_router_oracle():
    from oracle import router as orouter

    g = torch.Generator().manual_seed(11)
    lg = torch.randn(64, 256, generator=g) * 2
    for renorm in (True, False):
        ids, w = gref.ref_grouped_topk_router(lg, None, 8, 1, 1, "softmax", renorm, 1.0)
        rid, rw = orouter.ref_topk_router(lg, 8, renorm)
        assert torch.equal(ids, rid) and torch.allclose(w, rw)


def test_helper_rules_on_a_hand_written_case():
    """8 experts in 4 groups of 2, keep 2 groups, top 3.  sigmoid(3, 2, 1, -1, -2) = .9526, .8808, .7311, .2689, .1192."""
    bias = torch.tensor([0, 0, 0, 0, 0, 0.3, 0, 0])
    lg = torch.tensor([[3., -2, 2, 2, 1, 1, -2, -2],
                       [2., 2, 1, -1, -2, -2, 1, -1]])
    ids, w = gref.ref_grouped_topk_router(lg, bias, 3, 4, 2, "sigmoid", False, 1.0)
    s = torch.sigmoid(lg)
    # row 0: c = .9526 .1192 | .8808 .8808 | .7311 1.0311 | .1192 .1192; two-best sums 1.072, 1.762, 1.762 (+6e-4), .238:
    # groups 2 and 1 stay, where the maxima (.9526, .8808, 1.0311, .1192) would keep 2 and 0.  Expert 5 is first through
    # its bias alone (without it 4 and 5 tie below 2 and 3); 2 and 3 tie and go by id.
    assert ids[0].tolist() == [5, 2, 3]
    c = s + bias
    assert sorted(c.view(2, 4, 2).max(-1).values[0].topk(2).indices.tolist()) == [0, 2]
    # the weights are the unbiased scores
    assert torch.equal(w[0], s[0, [5, 2, 3]]) and abs(float(w[0, 0]) - 0.7311) < 1e-4
    # row 1: sums 1.762, 1.0, .538, 1.0: group 0 stays, groups 1 and 3 tie for the second place and 1 has the smaller id;
    # experts 0 and 1 tie and go by id
    assert ids[1].tolist() == [0, 1, 2]
    ids2, w2 = gref.ref_grouped_topk_router(lg, bias, 3, 4, 2, "sigmoid", True, 2.5)
    assert torch.equal(ids2, ids) and torch.allclose(w2.sum(-1), torch.full((2,), 2.5))
    assert torch.allclose(w2, 2.5 * w / w.sum(-1, keepdim=True))


# ---- CPU: the C entry refuses before any device call ----------------------------------------------------------------------
def _entry():
    from ctypes import c_float, c_int, c_int64, c_void_p

    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd.so"))
    fn = lib.hpc_grouped_topk_router_async
    fn.restype = c_int
    fn.argtypes = [c_void_p] * 4 + [c_int, c_int, c_int64] + [c_int] * 5 + [c_float, c_void_p]
    return fn


# ids, scale, logits, bias, num_tokens, num_expert, ld, topk, groups, topk_group, scoring, renormalize, scale, stream.
# The pointers are never dereferenced on the host, and num_tokens is 0 throughout: the checks run before the
# `num_tokens == 0` return, so no case here can reach a launch.
_P, _ODD = 4096, 4100
_OK = dict(ids=_P, sc=_P, lg=_P, bias=None, m=0, n=256, ld=256, k=8, g=8, kg=4, f=1)
_INVALID = [dict(ids=None), dict(sc=None), dict(lg=None), dict(m=-1), dict(k=0), dict(g=0, kg=0), dict(kg=0), dict(g=-1),
            dict(kg=9), dict(n=8, ld=8, g=1, kg=1, k=9), dict(f=2), dict(f=-1), dict(g=3, kg=1)]
_UNSUPPORTED = [dict(n=1028, ld=1028, g=1, kg=1), dict(n=254, g=1, kg=1), dict(n=48, ld=48, g=8, kg=4), dict(g=1, kg=1, k=65),
                dict(kg=1, k=33), dict(ld=258), dict(ld=252), dict(lg=_ODD), dict(bias=_ODD)]


def _call(fn, **kw):
    a = dict(_OK, **kw)
    return fn(a["ids"], a["sc"], a["lg"], a["bias"], a["m"], a["n"], a["ld"], a["k"], a["g"], a["kg"], a["f"], 1, 2.5, None)


def test_c_entry_refusals():
    fn = _entry()
    assert _call(fn) == 0 and _call(fn, bias=_P) == 0 and _call(fn, f=0, g=1, kg=1) == 0  # num_tokens == 0: no launch
    assert _call(fn, kg=1, k=32) == 0 and _call(fn, k=64) == 0 and _call(fn, n=1024, ld=1024) == 0
    for kw in _INVALID:
        assert _call(fn, **kw) == -2, kw
    for kw in _UNSUPPORTED:
        assert _call(fn, **kw) == -1, kw


def test_fake():
    from torch._subclasses import FakeTensorMode

    import hpc  # noqa: F401

    with FakeTensorMode():
        lg = torch.empty(16, 256, dtype=torch.float32, device="cuda")
        bias = torch.empty(256, dtype=torch.float32, device="cuda")
        for b in (bias, None):
            ids, w = torch.ops.hpc_router.grouped_topk_router(lg, b, 8, 8, 4, "sigmoid", True, 2.5, None, None)
            assert (tuple(ids.shape), ids.dtype, ids.device) == ((16, 8), torch.int32, lg.device)
            assert (tuple(w.shape), w.dtype, w.device) == ((16, 8), torch.float32, lg.device)
        ids, w = hpc.grouped_topk_router(lg, 8, 8, 4, bias)
        assert ids.shape == (16, 8) and w.dtype == torch.float32


# ---- GPU 1: the exact grid ------------------------------------------------------------------------------------------------
# (num_expert, n_group, topk_group, topk) -> seed.  Logits on a grid of 1/4, bias on a grid of 1/64: every row is full of
# exact ties that only the id rules resolve, and every other deciding gap is wide (asserted below, in float64: a property
# of the inputs - a seed that misses it is replaced, the kernel has no say in it).
GRID = {(256, 8, 4, 8): 0, (64, 8, 3, 6): 0, (384, 1, 1, 8): 0, (160, 8, 3, 6): 21, (96, 3, 1, 4): 0, (1024, 16, 4, 16): 0,
        (8, 1, 1, 8): 3}
GRID_ROWS = 257
GRID_GAP = 5e-5


@functools.lru_cache(maxsize=None)
def _grid(shape):
    n, n_group, topk_group, topk = shape
    g = torch.Generator().manual_seed(GRID[shape])
    lg = torch.randint(-16, 17, (GRID_ROWS, n), generator=g).float() / 4
    bias = torch.randint(-8, 9, (n,), generator=g).float() / 64
    d = gref.decision(lg, bias, topk, n_group, topk_group, "sigmoid")
    ids, w = gref.ref_grouped_topk_router(lg, bias, topk, n_group, topk_group, "sigmoid", True, 2.5)
    return lg, bias, float(d["strict"].min()), float(d["gaps"].min()), ids, w


def test_grid_inputs_decide_every_row():
    """every deciding gap that is not an exact tie of equal inputs exceeds 5e-5 (float64), and the rows do hold ties"""
    for shape in GRID:
        strict, gaps = _grid(shape)[2:4]
        assert strict > GRID_GAP, (shape, strict)
        assert gaps == 0.0, (shape, gaps)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("shape", list(GRID), ids=lambda s: "e%d_g%d_k%d_top%d" % s)
def test_grid_exact(shape, rows):
    import hpc

    n, n_group, topk_group, topk = shape
    lg, bias, strict, _, rid, rw = _grid(shape)
    assert strict > GRID_GAP
    ids, w = hpc.grouped_topk_router(lg[:rows].cuda(), topk, n_group, topk_group, bias.cuda(), "sigmoid", True, 2.5)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert torch.equal(ids.cpu(), rid[:rows])
    assert allclose(rw[:rows], w.cpu(), rtol=1e-5, atol=1e-7)


@pytest.mark.gpu
def test_grid_strided_rows_never_read_the_padding():
    import hpc

    shape = (256, 8, 4, 8)
    lg, bias, strict, _, rid, rw = _grid(shape)
    assert strict > GRID_GAP
    big = torch.full((GRID_ROWS, 320), 1e9)
    big[:, :256] = lg
    view = big.cuda()[:, :256]  # row stride 320 floats
    ids, w = hpc.grouped_topk_router(view, 8, 8, 4, bias.cuda(), "sigmoid", True, 2.5)
    assert torch.equal(ids.cpu(), rid) and allclose(rw, w.cpu(), rtol=1e-5, atol=1e-7)


@pytest.mark.gpu
def test_grid_one_group_softmax_equals_topk_router():
    import hpc

    lg = _grid((256, 8, 4, 8))[0]
    ids, w = hpc.grouped_topk_router(lg.cuda(), 8, 1, 1, None, "softmax", True, 1.0)
    tid, tw = hpc.topk_router(lg.cuda(), 8, True)
    assert torch.equal(ids, tid) and allclose(tw.cpu(), w.cpu(), rtol=1e-5, atol=1e-7)
    rid, rw = gref.ref_grouped_topk_router(lg, None, 8, 1, 1, "softmax", True, 1.0)
    assert torch.equal(ids.cpu(), rid) and allclose(rw, w.cpu(), rtol=1e-5, atol=1e-7)


# ---- GPU 2: random inputs, with the rows that hang on a few ulp set apart ------------------------------------------------------
CLOSE_GAP, CLOSE_SHARE = 1e-5, 0.04
RANDOM = [((256, 8, 4, 8), "sigmoid", True, True, 2.5), ((256, 8, 4, 8), "sigmoid", False, True, 2.5),
          ((256, 8, 4, 8), "softmax", True, True, 2.5), ((256, 8, 4, 8), "softmax", False, False, 1.0),
          ((160, 8, 3, 6), "softmax", False, True, 1.0), ((512, 4, 2, 8), "sigmoid", True, True, 2.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,scoring,with_bias,renorm,scale", RANDOM,
                         ids=lambda v: "e%d_g%d_k%d_top%d" % v if isinstance(v, tuple) else str(v))
def test_random_rows(shape, scoring, with_bias, renorm, scale):
    """Selection depends on s + bias in fp32 and the device's expf is not torch's, so a row whose deciding gap is a few
    ulp may come out differently.  Close row: a gap below 1e-5 in float64 among its first topk + 1 ordered candidates or
    first topk_group + 1 ordered group scores.  The others must match exactly."""
    import hpc

    n, n_group, topk_group, topk = shape
    g = torch.Generator().manual_seed(n + 7 * topk + (scoring == "softmax") + 2 * with_bias)
    lg = torch.randn(1000, n, generator=g)
    bias = 0.1 * torch.randn(n, generator=g) if with_bias else None
    d = gref.decision(lg, bias, topk, n_group, topk_group, scoring)
    close = d["gaps"] < CLOSE_GAP
    print(f"close rows: {int(close.sum())} of {len(close)}")
    assert float(close.float().mean()) <= CLOSE_SHARE
    rid, rw = gref.ref_grouped_topk_router(lg, bias, topk, n_group, topk_group, scoring, renorm, scale)
    rid64, _ = gref.ref_grouped_topk_router(lg, bias, topk, n_group, topk_group, scoring, renorm, scale, torch.float64)
    assert torch.equal(rid[~close], rid64[~close])
    ids, w = hpc.grouped_topk_router(lg.cuda(), topk, n_group, topk_group, None if bias is None else bias.cuda(), scoring,
                                     renorm, scale)
    ids, w = ids.cpu(), w.cpu()
    assert torch.equal(ids[~close], rid[~close])
    assert allclose(rw[~close], w[~close], rtol=1e-5, atol=1e-7)
    for r in torch.where(close)[0].tolist():
        gref.check_close_row(ids[r], d, r, topk, n_group, topk_group)


# ---- GPU 3: edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_caller_outputs_masked_experts_and_nan():
    import hpc

    g = torch.Generator().manual_seed(4)
    lg = torch.randn(7, 64, generator=g)
    lg[:, 10:50] = float("-inf")  # groups 2 ... 5 of 8 hold nothing else, groups 1 and 6 are partly masked
    oi, ow = torch.empty(7, 4, dtype=torch.int32, device="cuda"), torch.empty(7, 4, device="cuda")
    ids, w = hpc.grouped_topk_router(lg.cuda(), 4, 8, 4, None, "sigmoid", False, 1.0, oi, ow)
    assert ids.data_ptr() == oi.data_ptr() and w.data_ptr() == ow.data_ptr()
    rid, rw = gref.ref_grouped_topk_router(lg, None, 4, 8, 4, "sigmoid", False, 1.0)
    assert not bool((gref.decision(lg, None, 4, 8, 4, "sigmoid")["gaps"] < CLOSE_GAP).any())
    assert torch.equal(ids.cpu(), rid) and allclose(rw, w.cpu(), rtol=1e-5, atol=1e-7)
    assert not bool(((ids >= 10) & (ids < 50)).any())
    bias = (0.1 * torch.randn(64, generator=g)).cuda()
    for scoring in ("sigmoid", "softmax"):
        for pos in (0, 37, 63):
            bad = torch.randn(5, 64, generator=g)
            bad[2, pos] = float("nan")
            ids, w = hpc.grouped_topk_router(bad.cuda(), 6, 8, 3, bias, scoring, True, 2.5)
            assert bool(((ids >= 0) & (ids < 64)).all()), (scoring, pos, ids)
            rid, _ = gref.ref_grouped_topk_router(bad, bias.cpu(), 6, 8, 3, scoring, True, 2.5)
            rest = (gref.decision(bad, bias.cpu(), 6, 8, 3, scoring)["gaps"] >= CLOSE_GAP) & ~torch.isnan(bad).any(1)
            assert int(rest.sum()) >= 3 and torch.equal(ids.cpu()[rest], rid[rest])  # the rows next to it are untouched


@pytest.mark.gpu
def test_error_paths():
    import hpc

    lg = torch.randn(4, 64, device="cuda")
    bias = torch.zeros(64, device="cuda")
    for bad in (lambda: hpc.grouped_topk_router(lg.double(), 4, 8, 4),
                lambda: hpc.grouped_topk_router(lg.cpu(), 4, 8, 4),
                lambda: hpc.grouped_topk_router(lg, 0, 8, 4),
                lambda: hpc.grouped_topk_router(lg, 4, 8, 9),
                lambda: hpc.grouped_topk_router(lg, 4, 3, 1),
                lambda: hpc.grouped_topk_router(torch.randn(4, 48, device="cuda"), 4, 8, 4),  # groups of 6
                lambda: hpc.grouped_topk_router(lg, 9, 8, 1),
                lambda: hpc.grouped_topk_router(lg, 4, 8, 4, bias[:32]),
                lambda: hpc.grouped_topk_router(lg, 4, 8, 4, bias.double()),
                lambda: hpc.grouped_topk_router(lg, 4, 8, 4, bias, "tanh")):
        with pytest.raises(RuntimeError):
            bad()
    ids, _ = hpc.grouped_topk_router(lg, 4, 8, 4, bias)  # the arguments above are one step from a call that works
    assert ids.shape == (4, 4)


# ---- GPU 4: the chain -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("num_tokens", [9, 200])
def test_chain_gemm_grouped_router_fused_moe(num_tokens):
    """x -> gemm_bf16xfp32 (fp32 logits) -> grouped_topk_router -> fuse_moe_blockwise_fp8 on the device, against the
    helper fed with the device logits and the MoE oracle.  x and the router weight are small multiples of powers of two,
    so every partial sum of the GEMM is exact in fp32: the logits, and with them which rows are close, do not depend on the
    GEMM's summation order, and the seed below was chosen for having no close row."""
    import hpc
    from oracle import fuse_moe as omoe
    from oracle import gemm as ogemm

    g = torch.Generator().manual_seed(17)
    E, k, H, I = 64, 6, 512, 256
    xb = torch.randint(-1, 2, (num_tokens, H), generator=g).bfloat16()
    wr = torch.randint(-4, 5, (E, H), generator=g).float() / 16
    bias = 0.1 * torch.randn(E, generator=g)
    wh, wl = ogemm.split_weight(wr)
    logits = hpc.gemm_bf16xfp32(xb.cuda(), wh.cuda(), wl.cuda(), 1 / 256, True)
    assert allclose(ogemm.two_plane(xb, wh, wl, 1 / 256), logits.cpu(), rtol=1e-4, atol=2e-3)
    d = gref.decision(logits.cpu(), bias, k, 8, 4, "sigmoid")
    assert not bool((d["gaps"] < CLOSE_GAP).any()), "a close row: choose another seed"
    ids, sc = hpc.grouped_topk_router(logits, k, 8, 4, bias.cuda(), "sigmoid", True, 2.5)
    rid, rsc = gref.ref_grouped_topk_router(logits.cpu(), bias, k, 8, 4, "sigmoid", True, 2.5)
    assert torch.equal(ids.cpu(), rid) and allclose(rsc, sc.cpu(), rtol=1e-5, atol=1e-7)
    x8, xs = (xb.float() / 100).to(F8), torch.randn(num_tokens, H // 128, generator=g)
    guw, guws = torch.randn(E, 2 * I, H, generator=g).to(F8), torch.randn(E, 2 * I // 128, 4, generator=g)
    dw, dws = torch.randn(E, H, I, generator=g).to(F8), torch.randn(E, H // 128, 4, generator=g)
    my = hpc.fuse_moe_blockwise_fp8(x8.cuda(), xs.cuda(), guw.cuda(), guws.cuda(), dw.cuda(), dws.cuda(), ids, sc, 0, E)
    gt = omoe.fuse_moe_blockwise_fp8(x8, xs, guw, guws, dw, dws, rid, rsc, 0, E)
    torch.cuda.synchronize()
    assert allclose(gt.float(), my.cpu().float(), rtol=0.01, atol=0.01)


# ---- GPU 5: graph ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_replay_is_the_eager_result():
    import hpc

    lg, bias = _grid((256, 8, 4, 8))[:2]
    lgd, bd = lg[:64].cuda(), bias.cuda()
    eid, ew = hpc.grouped_topk_router(lgd, 8, 8, 4, bd, "sigmoid", True, 2.5)
    oi, ow = torch.empty_like(eid), torch.empty_like(ew)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hpc.grouped_topk_router(lgd, 8, 8, 4, bd, "sigmoid", True, 2.5, oi, ow)
    for _ in range(2):
        oi.zero_()
        ow.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(oi, eid) and torch.equal(ow.view(torch.int32), ew.view(torch.int32))
