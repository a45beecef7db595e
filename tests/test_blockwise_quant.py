"""hpc.blockwise_fp8_quant and hpc.fused_rmsnorm_blockwise_quant - the producers of the (x, x_scale) pair of the blockwise
fused MoE - against their PyTorch statement (tests/blockwise_quant_ref.py): codes and scales bit for bit, the normed row at
the half-ulp bar of the rope tests, preallocated outputs, hipGraph capture, refusals, fakes, and the chain into
fuse_moe_blockwise_fp8."""
import ctypes
import functools
import itertools
from pathlib import Path

import pytest
import torch

import blockwise_quant_ref as bref
from utils import ROPE_SLACK, moe_allclose, rope_excess

ROOT = Path(__file__).resolve().parent.parent
F8 = torch.float8_e4m3fn
BF16 = torch.bfloat16
EPS = 1e-6


def _blocks(t, h, seed, dtype=BF16):
    """[t, h]: every block of 128 columns is randn * 2^k with k drawn per (row, block) from -6 ... 6, and one block of every
    row is exactly zero (with a single block per row, h = 128: the block of every odd row)."""
    g = torch.Generator().manual_seed(seed)
    nb = h // 128
    k = torch.randint(-6, 7, (t, nb, 1), generator=g)
    x = torch.randn(t, nb, 128, generator=g) * torch.exp2(k.float())
    z = torch.randint(0, nb, (t,), generator=g)
    rows = torch.arange(t) if nb > 1 else torch.arange(1, t, 2)
    x[rows, z[rows]] = 0
    return x.view(t, h).to(dtype)


def _bits(q, scale):
    return q.cpu().view(torch.uint8), scale.cpu().view(torch.int32)


def _same(got, want):
    (gq, gs), (wq, ws) = _bits(*got), _bits(*want)
    assert gq.shape == wq.shape and gs.shape == ws.shape, (gq.shape, wq.shape, gs.shape, ws.shape)
    bad_q, bad_s = int((gq != wq).sum()), int((gs != ws).sum())
    if bad_q or bad_s:
        print(f"\n{bad_q}/{gq.numel()} codes and {bad_s}/{gs.numel()} scales differ")
        for r, c in torch.nonzero(gs != ws)[:5].tolist():
            print(f"  scale[{r}, {c}]: got {float(got[1][r, c]):.9g} want {float(want[1][r, c]):.9g}")
        for r, c in torch.nonzero(gq != wq)[:5].tolist():
            print(f"  q[{r}, {c}]: got 0x{int(gq[r, c]):02x} want 0x{int(wq[r, c]):02x}")
    return bad_q == 0 and bad_s == 0


# ---- CPU: the statement, the fakes, the surface ----------------------------------------------------------------------------
def test_statement_properties():
    """No NaN code, the largest code of every non-zero block is +-448, a zero block has a zero scale and zero codes, and
    the scale is the IEEE fp32 quotient amax / 448 (not a product with a rounded reciprocal)."""
    import numpy as np

    for h, seed in ((128, 0), (384, 1), (7168, 2), (16384, 3)):
        x = _blocks(9, h, seed)
        q, s = bref.quant(x)
        assert q.dtype == F8 and q.shape == x.shape and s.dtype == torch.float32 and s.shape == (9, h // 128)
        assert int(((q.view(torch.uint8) & 0x7F) == 0x7F).sum()) == 0
        top = q.float().view(9, h // 128, 128).abs().amax(-1)
        zero = x.float().view(9, h // 128, 128).abs().amax(-1) == 0
        assert zero.any() and not zero.all()
        assert torch.equal(top[~zero], torch.full_like(top[~zero], 448.0))
        assert torch.equal(s[zero], torch.zeros_like(s[zero])) and torch.equal(top[zero], torch.zeros_like(top[zero]))
        amax = x.float().view(9, h // 128, 128).abs().amax(-1).numpy()
        assert np.array_equal(s.numpy(), amax / np.float32(448.0))


def test_exported_from_hpc():
    import hpc

    for name in ("blockwise_fp8_quant", "fused_rmsnorm_blockwise_quant"):
        assert callable(getattr(hpc, name)) and name in hpc.__all__, name
    assert hpc.blockwise_fp8_quant.__doc__ and hpc.fused_rmsnorm_blockwise_quant.__doc__


def test_fakes():
    from torch._subclasses import FakeTensorMode

    import hpc

    t, h = 5, 384
    with FakeTensorMode():
        dev = torch.device("cuda")
        for dt in (BF16, torch.float16, torch.float32):
            x = torch.empty(t, h, dtype=dt, device=dev)
            for with_q, with_s in itertools.product((False, True), repeat=2):
                oq = torch.empty(t, h, dtype=F8, device=dev) if with_q else None
                os_ = torch.empty(t, h // 128, dtype=torch.float32, device=dev) if with_s else None
                q, s = hpc.blockwise_fp8_quant(x, oq, os_)
                assert (tuple(q.shape), q.dtype, q.device.type) == ((t, h), F8, "cuda")
                assert (tuple(s.shape), s.dtype, s.device.type) == ((t, h // 128), torch.float32, "cuda")
                assert (oq is None or q is oq) and (os_ is None or s is os_)
        a = torch.empty(t, h, dtype=BF16, device=dev)
        w = torch.empty(h, dtype=BF16, device=dev)
        for with_r, normed, with_q, with_s, with_y in itertools.product((False, True), repeat=5):
            if with_y and not normed:
                continue
            r = torch.empty(t, h, dtype=BF16, device=dev) if with_r else None
            oq = torch.empty(t, h, dtype=F8, device=dev) if with_q else None
            os_ = torch.empty(t, h // 128, dtype=torch.float32, device=dev) if with_s else None
            oy = torch.empty(t, h, dtype=BF16, device=dev) if with_y else None
            out = hpc.fused_rmsnorm_blockwise_quant(a, w, EPS, r, normed, oq, os_, oy)
            assert len(out) == (3 if normed else 2)
            assert (tuple(out[0].shape), out[0].dtype) == ((t, h), F8)
            assert (tuple(out[1].shape), out[1].dtype) == ((t, h // 128), torch.float32)
            assert (oq is None or out[0] is oq) and (os_ is None or out[1] is os_)
            if normed:
                assert (tuple(out[2].shape), out[2].dtype, out[2].device.type) == ((t, h), BF16, "cuda")
                assert oy is None or out[2] is oy
        q, s = hpc.fused_rmsnorm_blockwise_quant(a, w.view(1, h))
        assert q.shape == (t, h) and s.shape == (t, h // 128)


def _entries():
    from ctypes import c_float, c_int, c_void_p

    lib = ctypes.CDLL(str(ROOT / "hpc-ops_amd" / "hpc" / "libhpc_amd.so"))
    fq, fn = lib.hpc_blockwise_fp8_quant_async, lib.hpc_fused_rmsnorm_blockwise_quant_async
    fq.restype = fn.restype = c_int
    fq.argtypes = [c_void_p] * 3 + [c_int] * 3 + [c_void_p]
    fn.argtypes = [c_void_p] * 6 + [c_float, c_int, c_int, c_void_p]
    return fq, fn


def test_c_entry_refusals():
    """Every check of the C entries is made on the host: no case here reaches a launch (num_tokens is 0 in the accepted
    ones), and the pointers are never dereferenced."""
    fq, fn = _entries()
    p, odd = 4096, 4100
    assert fq(p, p, p, 0, 0, 7168, None) == 0 and fq(None, None, None, 2, 0, 128, None) == 0
    assert fn(p, p, p, p, p, p, EPS, 0, 16384, None) == 0 and fn(p, p, None, p, p, None, EPS, 0, 128, None) == 0
    for h in (0, 64, 320, 16512, -128):
        assert fq(p, p, p, 0, 0, h, None) == -1 and fq(p, p, p, 0, 4, h, None) == -1, h
        assert fn(p, p, p, p, p, p, EPS, 0, h, None) == -1 and fn(p, p, p, p, p, p, EPS, 4, h, None) == -1, h
    assert fq(p, p, p, 3, 4, 512, None) == -2 and fq(p, p, p, -1, 4, 512, None) == -2 and fq(p, p, p, 0, -1, 512, None) == -2
    assert fn(p, p, p, p, p, p, EPS, -1, 512, None) == -2
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert fq(*args, 0, 4, 512, None) == -2, args
    for args in ((None, p, p, p, p, p), (p, None, p, p, p, p), (p, p, p, None, p, p), (p, p, p, p, None, p)):
        assert fn(*args, EPS, 4, 512, None) == -2, args
    assert fq(p, p, odd, 0, 4, 512, None) == -1 and fq(odd, p, p, 0, 4, 512, None) == -1 and fq(p, 4098, p, 0, 4, 512, None) == -1
    for i in range(6):
        args = [p] * 6
        args[i] = 4098 if i == 1 else odd
        assert fn(*args, EPS, 4, 512, None) == -1, i


# ---- GPU 1: quant only, bit for bit --------------------------------------------------------------------------------------
# every nvec tier of the normed kernel, a partial wave (128, 384), block counts that are no power of two (384, 5120, 7168);
# 67 rows leave a partial row block
QUANT_H = [128, 384, 512, 1024, 2048, 4096, 5120, 7168, 8192, 16384]
ROWS = [1, 5, 67]
QUANT_CASES = [(h, t, BF16) for h in QUANT_H for t in ROWS] + \
              [(h, t, dt) for h in (384, 7168) for t in ROWS for dt in (torch.float16, torch.float32)]


@functools.lru_cache(maxsize=None)
def _quant_case(h, t, dtype):
    x = _blocks(t, h, 1000 + h + t, dtype)
    return x, bref.quant(x)


@pytest.mark.gpu
@pytest.mark.parametrize("h,t,dtype", QUANT_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_quant_bitwise(h, t, dtype):
    """Every step is an exact or IEEE-rounded fp32 operation (no fast-math in the build, a correctly rounded division, the
    hardware e4m3 cast pinned by the golden scaled_fp8_quant test): the bar is equality of the bits."""
    import hpc

    x, want = _quant_case(h, t, dtype)
    q, s = hpc.blockwise_fp8_quant(x.cuda())
    assert q.dtype == F8 and s.dtype == torch.float32 and q.is_contiguous() and s.is_contiguous()
    assert _same((q, s), want)


# ---- GPU 2: needles ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_quant_needles():
    """Row r: everything within [-1, 1] except column r of every block, which is -3.  Every scale is fp32(3) / 448 and the
    code there -448: a maximum over the wrong lanes (the whole wave, 8 lanes, a group that straddles two blocks) misses."""
    import hpc

    t, h = 128, 512
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(t, h // 128, 128, generator=g) * 2 - 1)
    x[torch.arange(t), :, torch.arange(t)] = -3.0
    x = x.view(t, h).to(BF16)
    q, s = hpc.blockwise_fp8_quant(x.cuda())
    want_scale = torch.tensor(3.0, dtype=torch.float32) / 448.0
    assert torch.equal(s.cpu().view(torch.int32), want_scale.expand(t, h // 128).contiguous().view(torch.int32))
    needles = q.cpu().float().view(t, h // 128, 128)[torch.arange(t), :, torch.arange(t)]
    assert torch.equal(needles, torch.full((t, h // 128), -448.0))
    assert _same((q, s), bref.quant(x))


# ---- GPU 4: residual add + RMSNorm + quant -------------------------------------------------------------------------------
NORM_H = [128, 384, 2048, 4096, 5120, 7168, 8192, 16384]


@functools.lru_cache(maxsize=None)
def _norm_case(h, t, with_residual):
    a = _blocks(t, h, 2000 + h + t)
    r = _blocks(t, h, 3000 + h + t) if with_residual else None
    g = torch.Generator().manual_seed(h)
    w = (torch.rand(h, generator=g) + 0.5).to(BF16)
    hsum, y64 = bref.norm64(a, w, EPS, r)
    # the fp32 statement, rounded once: what the same bar costs a plain PyTorch implementation on these inputs
    h32 = hsum.float()
    y32 = (h32 * torch.rsqrt(h32.pow(2).mean(-1, keepdim=True) + EPS) * w.float()).to(BF16)
    return a, r, w, hsum, y64, float(rope_excess(y64, y32).max())


def _run_norm(a, r, w, normed, **out):
    import hpc

    ad, wd = a.cuda(), w.cuda()
    rd = r.cuda() if r is not None else None
    res = hpc.fused_rmsnorm_blockwise_quant(ad, wd, EPS, rd, normed, **out)
    return ad, rd, res


@pytest.mark.gpu
@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("t", ROWS)
@pytest.mark.parametrize("h", NORM_H)
def test_fused_rmsnorm_blockwise_quant(h, t, with_residual):
    a, r, w, hsum, y64, cpu_excess = _norm_case(h, t, with_residual)
    ad, rd, (q, s, y) = _run_norm(a, r, w, True)
    assert torch.equal(ad.cpu().view(torch.int16), a.view(torch.int16)), "a was written"
    if with_residual:
        assert torch.equal(rd.cpu().view(torch.int16), hsum.view(torch.int16)), "residual != bf16(a + residual)"
    assert y.dtype == BF16 and y.shape == a.shape and q.dtype == F8 and s.shape == (t, h // 128)
    # the normed row: half a bf16 ulp of the float64 result plus fp32 noise (the sum of squares in another order, the
    # hardware rsqrt), the bar and the slack of the rope tests (tests/utils.py::rope_excess, ROPE_SLACK = 2^-20)
    excess = float(rope_excess(y64, y.cpu()).max())
    print(f"H {h} T {t} residual {with_residual}: excess over half an ulp, of the row maximum: kernel {excess:.3g}, "
          f"fp32 PyTorch statement {cpu_excess:.3g}, bar {ROPE_SLACK:.3g}")
    assert excess <= ROPE_SLACK
    # codes and scales: of the kernel's own bf16-rounded y, bit for bit
    assert _same((q, s), bref.quant(y.cpu()))
    # ... and the same without the normed output
    _, rd2, out2 = _run_norm(a, r, w, False)
    assert len(out2) == 2 and _same(out2, (q, s))
    if with_residual:
        assert torch.equal(rd2, rd)


# ---- GPU 5: the two kernels agree ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("h", [384, 7168])
def test_quant_of_normed_equals_fused(h):
    import hpc

    a, r, w, _, _, _ = _norm_case(h, 67, True)
    _, _, (q, s, y) = _run_norm(a, r, w, True)
    assert _same(hpc.blockwise_fp8_quant(y), (q, s))


# ---- GPU 3: preallocated outputs and row bounds --------------------------------------------------------------------------
def _sentinels(h, dev):
    q = torch.full((8, h), 0x5A, dtype=torch.uint8, device=dev).view(F8)
    s = torch.full((8, h // 128), -7.0, dtype=torch.float32, device=dev)
    y = torch.full((8, h), -9.0, dtype=BF16, device=dev)
    return q, s, y


@pytest.mark.gpu
@pytest.mark.parametrize("h", [384, 7168])
def test_preallocated_outputs_and_row_bounds(h):
    import hpc

    dev = torch.device("cuda")
    t = 5
    x, want = _quant_case(h, t, BF16)
    qb, sb, _ = _sentinels(h, dev)
    q, s = hpc.blockwise_fp8_quant(x.cuda(), qb[:t], sb[:t])
    assert q.data_ptr() == qb.data_ptr() and s.data_ptr() == sb.data_ptr()
    oq, os_ = qb[:t], sb[:t]
    q, s = hpc.blockwise_fp8_quant(x.cuda(), oq, os_)
    assert q is oq and s is os_
    assert _same((qb[:t], sb[:t]), want)
    assert bool((qb[t:].view(torch.uint8) == 0x5A).all()) and bool((sb[t:] == -7.0).all())

    a, r, w, hsum, _, _ = _norm_case(h, t, True)
    qb, sb, yb = _sentinels(h, dev)
    rb = torch.full((8, h), -11.0, dtype=BF16, device=dev)
    rb[:t] = r.cuda()
    oq, os_, oy = qb[:t], sb[:t], yb[:t]
    q, s, y = hpc.fused_rmsnorm_blockwise_quant(a.cuda(), w.cuda(), EPS, rb[:t], True, oq, os_, oy)
    assert q is oq and s is os_ and y is oy
    assert torch.equal(rb[:t].cpu().view(torch.int16), hsum.view(torch.int16))
    assert _same((qb[:t], sb[:t]), bref.quant(yb[:t].cpu()))
    _, _, (q0, s0, y0) = _run_norm(a, r, w, True)
    assert torch.equal(yb[:t], y0) and _same((qb[:t], sb[:t]), (q0, s0))
    assert bool((qb[t:].view(torch.uint8) == 0x5A).all()) and bool((sb[t:] == -7.0).all())
    assert bool((yb[t:] == -9.0).all()) and bool((rb[t:] == -11.0).all())
    oq2, os2 = torch.empty_like(oq), torch.empty_like(os_)
    out = hpc.fused_rmsnorm_blockwise_quant(a.cuda(), w.cuda(), EPS, None, False, oq2, os2)
    assert len(out) == 2 and out[0] is oq2 and out[1] is os2


# ---- GPU 6: it feeds the MoE ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_feeds_fuse_moe_blockwise_fp8():
    """The smallest case of tests/test_fuse_moe_blockwise.py::test_fuse_moe_blockwise_fp8 (1 token, I = 256, rank 0 of 1,
    no shared output; E = 128, top 8, H = 512) with its weights, and the activations from the fused op: layout, dtype and
    contiguity are what the consumer takes, with real positive scales."""
    import hpc
    from oracle import fuse_moe as omoe
    from test_fuse_moe_blockwise import _inputs

    num_tokens, inter, num_expert, num_topk, hidden = 1, 256, 128, 8, 512
    _, _, guw, guws, dw, dws, topk_ids, topk_scale, _ = _inputs(num_tokens, num_topk, hidden, inter, num_expert, 1, False)
    g = torch.Generator().manual_seed(7)
    hs = torch.randn(num_tokens, hidden, generator=g).to(BF16)
    w = (torch.rand(hidden, generator=g) + 0.5).to(BF16)
    q, s = hpc.fused_rmsnorm_blockwise_quant(hs.cuda(), w.cuda(), EPS)
    assert bool((s > 0).all())
    my = hpc.fuse_moe_blockwise_fp8(q, s, guw.cuda(), guws.cuda(), dw.cuda(), dws.cuda(), topk_ids.cuda(), topk_scale.cuda(),
                                    0, num_expert)
    torch.cuda.synchronize()
    gt = omoe.fuse_moe_blockwise_fp8(q.cpu(), s.cpu(), guw, guws, dw, dws, topk_ids, topk_scale, 0, num_expert)
    assert moe_allclose(gt, my.cpu())


# ---- GPU 7: capture ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_capture_with_preallocated_outputs():
    """With every output given nothing is allocated: each op is one kernel in a hipGraph, replayed on new input."""
    import hpc

    t, h = 5, 7168
    dev = torch.device("cuda")
    xs = [_blocks(t, h, 40 + i).cuda() for i in range(3)]
    rs = [_blocks(t, h, 50 + i).cuda() for i in range(3)]
    w = (torch.rand(h) + 0.5).to(BF16).cuda()
    x, r = xs[0].clone(), rs[0].clone()
    q1, s1 = torch.empty(t, h, dtype=F8, device=dev), torch.empty(t, h // 128, dtype=torch.float32, device=dev)
    q2, s2, y2 = torch.empty_like(q1), torch.empty_like(s1), torch.empty(t, h, dtype=BF16, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        hpc.blockwise_fp8_quant(x, q1, s1)
        hpc.fused_rmsnorm_blockwise_quant(x, w, EPS, r, True, q2, s2, y2)
    torch.cuda.current_stream().wait_stream(side)
    g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        hpc.blockwise_fp8_quant(x, q1, s1)
    with torch.cuda.graph(g2):
        hpc.fused_rmsnorm_blockwise_quant(x, w, EPS, r, True, q2, s2, y2)
    for i in (1, 2):
        x.copy_(xs[i])
        r.copy_(rs[i])
        g1.replay()
        g2.replay()
        torch.cuda.synchronize()
        assert _same((q1, s1), hpc.blockwise_fp8_quant(xs[i]))
        re = rs[i].clone()
        qe, se, ye = hpc.fused_rmsnorm_blockwise_quant(xs[i], w, EPS, re, True)
        assert _same((q2, s2), (qe, se)) and torch.equal(y2, ye) and torch.equal(r, re)


# ---- GPU 8: refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    """Each of these raises before anything is launched: the checks are on the host."""
    import hpc

    dev = torch.device("cuda")
    t, h = 4, 512
    x = torch.zeros(t, h, dtype=BF16, device=dev)
    w = torch.ones(h, dtype=BF16, device=dev)
    quant, norm = hpc.blockwise_fp8_quant, hpc.fused_rmsnorm_blockwise_quant
    f8 = lambda *shape: torch.empty(*shape, dtype=F8, device=dev)  # noqa: E731
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    bad = [
        lambda: quant(torch.zeros(t, 320, dtype=BF16, device=dev)),
        lambda: quant(torch.zeros(t, 16512, dtype=BF16, device=dev)),
        lambda: quant(torch.zeros(t, 2 * h, dtype=BF16, device=dev)[:, :h]),
        lambda: quant(torch.zeros(h, t, dtype=BF16, device=dev).t()),
        lambda: quant(torch.zeros(t, h, dtype=torch.int32, device=dev)),
        lambda: quant(torch.zeros(t * h, dtype=BF16, device=dev)),
        lambda: quant(x, f8(t + 1, h)),
        lambda: quant(x, torch.empty(t, h, dtype=torch.uint8, device=dev)),
        lambda: quant(x, f8(t, 2 * h)[:, :h]),
        lambda: quant(x, None, f32(t, h // 128 + 1)),
        lambda: quant(x, None, torch.empty(t, h // 128, dtype=torch.float16, device=dev)),
        lambda: norm(torch.zeros(t, 320, dtype=BF16, device=dev), torch.ones(320, dtype=BF16, device=dev)),
        lambda: norm(torch.zeros(t, 16512, dtype=BF16, device=dev), torch.ones(16512, dtype=BF16, device=dev)),
        lambda: norm(torch.zeros(t, 2 * h, dtype=BF16, device=dev)[:, :h], w),
        lambda: norm(x.float(), w),
        lambda: norm(torch.zeros(t, h, dtype=torch.int32, device=dev), w),
        lambda: norm(x, torch.ones(h - 128, dtype=BF16, device=dev)),
        lambda: norm(x, torch.ones(2, h, dtype=BF16, device=dev)),
        lambda: norm(x, w.float()),
        lambda: norm(x, w, EPS, torch.zeros(t + 1, h, dtype=BF16, device=dev)),
        lambda: norm(x, w, EPS, torch.zeros(t, h, dtype=torch.float16, device=dev)),
        lambda: norm(x, w, EPS, torch.zeros(t, 2 * h, dtype=BF16, device=dev)[:, :h]),
        lambda: norm(x, w, EPS, None, False, f8(t, h // 2)),
        lambda: norm(x, w, EPS, None, False, None, f32(t, h // 128, 1)),
        lambda: norm(x, w, EPS, None, False, None, torch.empty(t, h // 128, dtype=torch.float64, device=dev)),
        lambda: norm(x, w, EPS, None, True, None, None, torch.empty(t, h, dtype=torch.float16, device=dev)),
        lambda: norm(x, w, EPS, None, True, None, None, torch.empty(t + 1, h, dtype=BF16, device=dev)),
        lambda: norm(x, w, EPS, None, False, None, None, torch.empty(t, h, dtype=BF16, device=dev)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"case {i} was accepted")
    torch.cuda.synchronize()
    for dt in (BF16, torch.float16, torch.float32):
        q, s = quant(torch.zeros(0, h, dtype=dt, device=dev))
        assert (tuple(q.shape), q.dtype, tuple(s.shape), s.dtype) == ((0, h), F8, (0, h // 128), torch.float32)
    e = torch.zeros(0, h, dtype=BF16, device=dev)
    q, s, y = norm(e, w, EPS, e.clone(), True)
    assert (tuple(q.shape), q.dtype, tuple(s.shape), s.dtype) == ((0, h), F8, (0, h // 128), torch.float32)
    assert (tuple(y.shape), y.dtype) == ((0, h), BF16)
    q, s = norm(e, w)
    assert q.shape == (0, h) and s.shape == (0, h // 128)
