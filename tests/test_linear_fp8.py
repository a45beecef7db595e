"""hpc.gemm_blockwise_fp8: the dense FP8 linear with 128-block scales for decode batches, against its PyTorch statement
(tests/linear_fp8_ref.py).

CPU: the statement's own properties, the bar against a float32 restatement, fakes, the export, host refusals through the C-ABI
and the plan against the route's arithmetic restated here.  GPU: exact inputs bit for bit over every split count, random inputs
at the derived bar, repeatability / counters / hipGraph capture, the scratch contract between guard bands, the chain behind the
fused RMSNorm quantiser."""
import ctypes
import functools
import itertools
import random

import pytest
import torch

import linear_fp8_ref as lref

F8 = torch.float8_e4m3fn
GUARD = 1 << 20
PATTERN = 0xA5
CUS = 256  # the MI355X; the plan takes the CU count as an argument, so the CPU checks do not need a device


@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def plan(lib, m, n, k, splits_wanted, cus=CUS):
    """(code, splits, max_splits, workspace_bytes, counters)"""
    s, mx, cnt = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    ws = ctypes.c_int64(-7)
    rc = lib.hpc_gemm_blockwise_fp8_plan(m, n, k, splits_wanted, cus, ctypes.byref(s), ctypes.byref(mx), ctypes.byref(ws),
                                         ctypes.byref(cnt))
    return rc, s.value, mx.value, ws.value, cnt.value


# ---- CPU: the statement ---------------------------------------------------------------------------------------------------
def test_statement_is_the_scaled_matmul():
    """With unit scales the statement is the plain product of the codes; a block's activation scale and its weight scale each
    multiply that block's contribution alone, and a row of N that ends inside a 128-row scale block reads the last scale row."""
    xq, xs, wq, ws, _ = lref.exact_inputs(5, 192, 384)
    one_x, one_w = torch.ones_like(xs), torch.ones_like(ws)
    r1, a1 = lref.ref(xq, one_x, wq, one_w)
    assert torch.equal(r1, xq.double() @ wq.double().t())
    assert bool((a1 >= r1.abs()).all())
    # activation scale of (row 3, block 1)
    sx = one_x.clone()
    sx[3, 1] = 4.0
    r2, _ = lref.ref(xq, sx, wq, one_w)
    blk = xq.double()[:, 128:256] @ wq.double()[:, 128:256].t()
    want = r1.clone()
    want[3] += 3.0 * blk[3]
    assert torch.equal(r2, want)
    # weight scale of (row block 1 = rows 128 .. 191, block 2)
    sw = one_w.clone()
    sw[1, 2] = 0.5
    r3, _ = lref.ref(xq, one_x, wq, sw)
    blk = xq.double()[:, 256:384] @ wq.double()[:, 256:384].t()
    want = r1.clone()
    want[:, 128:] -= 0.5 * blk[:, 128:]
    assert torch.equal(r3, want)


def test_exact_inputs_are_exact_for_any_split_count():
    """The exact grid's premise, on the CPU: a float32 evaluation split 1, 2, 3 and 8 ways equals bf16(float64 statement)."""
    xq, xs, wq, ws, want = lref.exact_inputs(5, 256, 1024)
    for s in (1, 2, 3, 8):
        assert torch.equal(lref.fp32_restatement(xq, xs, wq, ws, s), want), s


RANDOM_SHAPES = [(7, 256, 640), (33, 128, 2048), (64, 384, 7168), (16, 512, 16384)]


@pytest.mark.parametrize("m,n,k", RANDOM_SHAPES)
def test_bar_holds_for_a_float32_restatement(m, n, k):
    """Before the GPU test relies on the bar: the kernel's arithmetic restated in float32, with 1, 3 and the largest split
    count, stays inside it with room - the bar is derived from the formats, this only shows it is not too tight."""
    xq, xs, wq, ws, r, a = lref.random_inputs(m, n, k)
    bound = lref.bar(r, a, k)
    worst = 0.0
    for s in (1, 3, min(16, k // 128)):
        y = lref.fp32_restatement(xq, xs, wq, ws, s).double()
        worst = max(worst, float(((y - r).abs() / bound.clamp_min(1e-300)).max()))
    print(f"fp32 restatement ({m}, {n}, {k}): worst |y - r| / bar = {worst:.3f}")
    assert worst <= 1.0


# ---- CPU: surface -----------------------------------------------------------------------------------------------------------
def test_exported_with_a_docstring():
    import hpc

    assert callable(hpc.gemm_blockwise_fp8) and "gemm_blockwise_fp8" in hpc.__all__
    doc = hpc.gemm_blockwise_fp8.__doc__
    for word in ("x_scale[m, kb]", "weight_scale", "splits", "bit-identical", "group_gemm_blockwise_fp8", "256"):
        assert word in doc, word


def test_fakes():
    from torch._subclasses import FakeTensorMode

    import hpc

    with FakeTensorMode():
        x = torch.empty(17, 384, dtype=F8, device="cuda")
        xs = torch.empty(17, 3, dtype=torch.float32, device="cuda")
        w = torch.empty(192, 384, dtype=F8, device="cuda")
        ws = torch.empty(2, 3, dtype=torch.float32, device="cuda")
        y = torch.ops.hpc_linear.gemm_blockwise_fp8(x, xs, w, ws, None, 0)
        assert (tuple(y.shape), y.dtype, y.device) == ((17, 192), torch.bfloat16, x.device)
        y = hpc.gemm_blockwise_fp8(x, xs, w, ws, splits=2)
        assert (tuple(y.shape), y.dtype) == ((17, 192), torch.bfloat16)
        out = torch.empty(17, 192, dtype=torch.bfloat16, device="cuda")
        assert hpc.gemm_blockwise_fp8(x, xs, w, ws, output=out) is out
        y = torch.ops.hpc_linear.gemm_blockwise_fp8(x, xs, w, ws, out, 0)
        assert (tuple(y.shape), y.dtype) == ((17, 192), torch.bfloat16)


# ---- CPU: host refusals through the C-ABI, pointers never dereferenced --------------------------------------------------------
def test_host_refusals(lib):
    p = ctypes.c_void_p(4096)

    def call(m, n, k, splits, ws_stride=None, ws_bytes=1 << 40, y=p, x=p, planes=p):
        return lib.hpc_gemm_blockwise_fp8_async(y, x, p, p, p, m, n, k, k // 128 if ws_stride is None else ws_stride, splits,
                                                planes, ws_bytes, p, None)

    assert call(8, 128, 192, 1) == -1  # K % 128
    assert call(8, 128, 0, 1) == -2  # no K at all
    assert call(8, 96, 256, 1) == -1  # N % 64
    assert call(257, 128, 256, 1) == -1  # M > 256
    assert call(8, 65536, 65536, 1) == -1  # N * K beyond 32-bit offsets
    assert call(8, 128, 256, 3) == -2  # splits > max = K / 128 = 2
    assert call(8, 128, 128 * 40, 17) == -2  # splits > max = 16
    assert call(-1, 128, 256, 1) == -2
    assert call(8, 128, 256, -1) == -2
    assert call(8, 128, 256, 1, ws_stride=1) == -2  # weight-scale rows shorter than K / 128
    assert call(8, 128, 256, 1, y=None) == -2
    assert call(8, 128, 256, 1, x=ctypes.c_void_p(4104)) == -1  # activations not 16-byte aligned
    assert call(8, 128, 256, 2, ws_bytes=2 * 8 * 128 * 4 - 1) == -2  # workspace one byte short of the plan's
    assert call(8, 128, 256, 2, planes=None) == -2
    assert call(0, 128, 256, 1) == 0  # nothing to do, nothing launched
    # the plan refuses the same shapes and says -2 for a missing output pointer
    assert plan(lib, 8, 128, 192, 0)[0] == -1 and plan(lib, 257, 128, 256, 0)[0] == -1 and plan(lib, 8, 96, 256, 0)[0] == -1
    assert plan(lib, 8, 65536, 65536, 0)[0] == -1 and plan(lib, 8, 128, 256, 3)[0] == -2
    one = ctypes.c_int(0)
    assert lib.hpc_gemm_blockwise_fp8_plan(8, 128, 256, 0, CUS, None, ctypes.byref(one), None, ctypes.byref(one)) == -2


# ---- CPU: the plan against the route's arithmetic, restated -------------------------------------------------------------------
def route(m, n, k, splits_wanted, cus):
    """(splits, max_splits, workspace_bytes, counters): the rule of csrc/gemm_blockwise_fp8_route.h."""
    kb = k // 128
    tiles = (m + 63) // 64 * (n // 64)
    if splits_wanted:
        s = splits_wanted
    else:
        s = max(1, min((cus + tiles - 1) // tiles, kb // 4, 16))
    return s, min(16, kb), (s * m * n * 4 if s > 1 else 0), (tiles if s > 1 else 0)


def test_plan_equals_the_route_rule(lib):
    seen_split = seen_one = 0
    for m, n, k, cus in itertools.product((1, 16, 17, 64, 65, 200, 256), (64, 192, 576, 2112, 7168, 24576),
                                          (128, 384, 512, 640, 1536, 2304, 7168, 16384), (80, 104, 256, 304)):
        for want in (0, 1, 2, 3, 16):
            got = plan(lib, m, n, k, want, cus)
            if want > min(16, k // 128):
                assert got[0] == -2, (m, n, k, want)
                continue
            assert got == (0,) + route(m, n, k, want, cus), (m, n, k, want, cus)
            _, s, mx, ws, cnt = got
            assert 1 <= s <= mx <= min(16, k // 128)
            assert (ws >= s * m * n * 4 and cnt == (m + 63) // 64 * (n // 64)) if s > 1 else (ws == 0 and cnt == 0)
            if want == 0:
                assert s == 1 or k // 128 // s >= 4  # the library's splits keep four k-blocks
                tiles = (m + 63) // 64 * (n // 64)
                assert s == 1 or tiles * (s - 1) < cus  # never more splits than reach the CU count
                seen_split += s > 1
                seen_one += s == 1
    assert seen_split and seen_one
    # cu_count <= 0 asks the device; without one the route assumes 256
    if not torch.cuda.is_available():
        assert plan(lib, 16, 2112, 7168, 0, 0) == plan(lib, 16, 2112, 7168, 0, 256)
    assert plan(lib, 16, 2112, 7168, 0, 256)[1] == 8 and plan(lib, 64, 7168, 16384, 0, 256)[1] == 3
    assert plan(lib, 0, 128, 256, 0)[0] == 0


# ---- GPU 1: exact inputs, bit for bit -----------------------------------------------------------------------------------------
def _exact_cases():
    """~60 of the (M, N, K, splits) grid with a fixed seed, splits within the shape's bound."""
    grid = [(m, n, k, s) for m, n, k, s in itertools.product((1, 15, 16, 17, 64, 65, 130, 256), (64, 128, 192, 576),
                                                             (128, 384, 640, 2304), (0, 1, 2, 3, 5)) if s <= k // 128]
    return sorted(random.Random(20240607).sample(grid, 60))


EXACT_CASES = _exact_cases()


def test_exact_cases_cover_every_mechanism(lib):
    """The sample holds an unsplit case, an even and an uneven split, a library-chosen split of more than one slice, both
    sides of the 64-token tile and an N that ends inside a scale block."""
    planned = [(c, plan(lib, *c)) for c in EXACT_CASES]
    assert all(p[0] == 0 for _, p in planned)
    split_of = {c: p[1] for c, p in planned}
    assert any(s == 1 for s in split_of.values())
    assert any(s > 1 and (c[2] // 128) % s == 0 for c, s in split_of.items())
    assert any(s > 1 and (c[2] // 128) % s != 0 for c, s in split_of.items())
    assert any(c[3] == 0 and s > 1 for c, s in split_of.items())
    assert any(c[0] > 64 and s > 1 for c, s in split_of.items()) and any(c[0] <= 16 for c in split_of)
    assert any(c[1] % 128 and s > 1 for c, s in split_of.items())


def _dev(*ts):
    return [t.cuda() for t in ts]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,splits", EXACT_CASES)
def test_exact_inputs_bit_for_bit(m, n, k, splits):
    import hpc

    xq, xs, wq, ws, want = lref.exact_inputs(m, n, k)
    y = hpc.gemm_blockwise_fp8(*_dev(xq, xs, wq, ws), splits=splits)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (m, n)
    assert torch.equal(y.cpu(), want)


@pytest.mark.gpu
def test_padded_weight_scale_rows_and_empty_batch():
    """weight_scale rows padded to a multiple of four floats (stride(0) > K / 128) are read by their stride; M == 0 returns an
    empty [0, N] tensor."""
    import hpc

    xq, xs, wq, ws, want = lref.exact_inputs(17, 192, 640)
    dx, dxs, dw, dws = _dev(xq, xs, wq, ws)
    padded = torch.full((ws.shape[0], 8), float("nan"), device="cuda")
    padded[:, :5] = dws
    view = padded[:, :5]
    assert view.stride() == (8, 1)
    assert torch.equal(hpc.gemm_blockwise_fp8(dx, dxs, dw, view, splits=2).cpu(), want)
    y = hpc.gemm_blockwise_fp8(dx[:0], dxs[:0], dw, dws)
    assert tuple(y.shape) == (0, 192) and y.dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="group_gemm_blockwise_fp8"):
        hpc.gemm_blockwise_fp8(torch.empty(257, 640, dtype=F8, device="cuda"), torch.empty(257, 5, device="cuda"), dw, dws)
    with pytest.raises(RuntimeError, match="splits"):
        hpc.gemm_blockwise_fp8(dx, dxs, dw, dws, splits=6)


# ---- GPU 2: random inputs at the derived bar ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("m,n,k", RANDOM_SHAPES)
def test_random_inputs_at_the_derived_bar(m, n, k, splits):
    """|y - r| <= 2^-8 |r| + (K/128 + 24) 2^-23 A per element: bf16's worst half ulp plus one fp32 rounding per rescale,
    accumulate and plane add on magnitudes bounded by A (derived, not measured).  Scales differ by up to 2^12 between
    neighbouring blocks, so a wrong scale index fails this.

    On the MI355X the worst |y - r| / bar is 0.940 / 0.986 / 0.984 / 0.975 at the four shapes, splits 0 / 1 / 3 alike - the
    figures of the float32 restatement on the CPU.  The bar grants fp32 roundings on the blocks' sums, so it also tells an
    fp32-grade block sum from the fp8 matrix instruction's: that one keeps about 15 bits below the largest product of a lane's
    operand chunk, and a kernel built on it measured 1.440 / 2.583 / 1.129 / 0.975 here, over the bar wherever a block's
    products cancel (|r| << A << sum |products|).  The kernel multiplies in f16 for that reason (csrc/gemm_blockwise_fp8.hip)."""
    import hpc

    xq, xs, wq, ws, r, a = lref.random_inputs(m, n, k)
    y = hpc.gemm_blockwise_fp8(*_dev(xq, xs, wq, ws), splits=splits).cpu().double()
    ratio = (y - r).abs() / lref.bar(r, a, k).clamp_min(1e-300)
    print(f"({m}, {n}, {k}) splits {splits}: worst |y - r| / bar = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0


# ---- GPU 3: repeatability, counters, hipGraph ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_repeatable_and_counters_left_zero():
    """Twenty calls of one split shape give the same bits; two shapes that share the stream's scratch alternate without a fill
    in between and both stay right, so every call leaves its counters zero."""
    import hpc

    xq, xs, wq, ws, r, a = lref.random_inputs(33, 128, 2048)
    dev = _dev(xq, xs, wq, ws)
    first = hpc.gemm_blockwise_fp8(*dev)
    for _ in range(19):
        assert torch.equal(hpc.gemm_blockwise_fp8(*dev), first)
    ea = lref.exact_inputs(130, 576, 2304)
    eb = lref.exact_inputs(17, 192, 640)
    da, db = _dev(*ea[:4]), _dev(*eb[:4])
    outs = []
    for _ in range(3):
        outs.append((hpc.gemm_blockwise_fp8(*da, splits=5), hpc.gemm_blockwise_fp8(*db, splits=3)))
    for ya, yb in outs:
        assert torch.equal(ya.cpu(), ea[4]) and torch.equal(yb.cpu(), eb[4])


@pytest.mark.gpu
def test_captures_into_a_graph_with_output_given():
    import hpc

    xq, xs, wq, ws, want = lref.exact_inputs(65, 192, 2304)
    dev = _dev(xq, xs, wq, ws)
    out = torch.zeros(65, 192, dtype=torch.bfloat16, device="cuda")
    eager = hpc.gemm_blockwise_fp8(*dev)
    assert torch.equal(eager.cpu(), want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert hpc.gemm_blockwise_fp8(*dev, output=out) is out
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hpc.gemm_blockwise_fp8(*dev, output=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    del graph
    hpc.release_decode_workspaces()


# ---- GPU 4: the scratch contract ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scratch_of_exactly_the_planned_size(lib):
    """Through the C-ABI with [planes | counters] of exactly the plan's bytes between two guard bands: planes pre-filled with NaN
    patterns, counters zero.  The result is the exact one, the guards are untouched, the counters zero again."""
    from hpc import _C

    m, n, k, splits = 65, 192, 640, 5
    xq, xs, wq, ws, want = lref.exact_inputs(m, n, k)
    dx, dxs, dw, dws = _dev(xq, xs, wq, ws)
    rc, s, _, ws_bytes, counters = plan(lib, m, n, k, splits, 0)
    assert (rc, s) == (0, splits) and ws_bytes == splits * m * n * 4 and counters == 2 * 3
    nbytes = ws_bytes + counters * 4
    buf = torch.full((2 * GUARD + nbytes,), PATTERN, dtype=torch.uint8, device="cuda")
    planes = buf[GUARD:GUARD + ws_bytes].view(torch.int32)
    cnt = buf[GUARD + ws_bytes:GUARD + nbytes].view(torch.int32)
    planes.fill_(0x7FC00000)
    cnt.zero_()
    y = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
    rc = lib.hpc_gemm_blockwise_fp8_async(_C.ptr(y), _C.ptr(dx), _C.ptr(dxs), _C.ptr(dw), _C.ptr(dws), m, n, k, dws.stride(0), splits,
                                          _C.ptr(planes), ws_bytes, _C.ptr(cnt), _C.stream_of(dx))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want)
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + nbytes:] == PATTERN).all())
    assert bool((cnt == 0).all())


# ---- GPU 5: behind the fused RMSNorm quantiser --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_behind_fused_rmsnorm_blockwise_quant():
    """fused_rmsnorm_blockwise_quant -> gemm_blockwise_fp8 at (M 17, H 384, N 192): the quantiser's outputs go in as they come
    out; compared with the statement applied to those outputs, at the bar of the random test.

    On the MI355X: worst |y - r| / bar = 0.976 (1.700 on the fp8 matrix instruction: test_random_inputs_at_the_derived_bar)."""
    import hpc

    m, h, n = 17, 384, 192
    g = torch.Generator().manual_seed(11)
    a = (torch.randn(m, h, generator=g) * 3).bfloat16().cuda()
    w = (1 + 0.1 * torch.randn(h, generator=g)).bfloat16().cuda()
    wq, ws = lref.random_weight(n, h)
    q, s = hpc.fused_rmsnorm_blockwise_quant(a, w)[:2]
    assert q.dtype == F8 and tuple(s.shape) == (m, h // 128)
    y = hpc.gemm_blockwise_fp8(q, s, wq.cuda(), ws.cuda()).cpu().double()
    r, big_a = lref.ref(q.cpu(), s.cpu(), wq, ws)
    ratio = (y - r).abs() / lref.bar(r, big_a, h).clamp_min(1e-300)
    print(f"chain: worst |y - r| / bar = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0 and float(r.abs().max()) > 0
