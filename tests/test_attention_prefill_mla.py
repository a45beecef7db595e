"""hpc.attention_prefill_mla_bf16: MLA prefill attention in the non-absorbed form (192 / 128 heads) with an lse output.

CPU: properties of the float64 statement (tests/mla_prefill_ref.py); the bars of tests/mla_prefill_needles.py measured again -
the online model stays within them, they are at most 3 x its worst case, mutants are rejected at >= 3 tau; the public surface
and fakes; host refusals through the C-ABI with never-dereferenced pointers, in the route's order; the grid restated here.
GPU: needle parity at the measured bars through the strided views a caller has and once through contiguous tensors, the
context form, chunked == whole through merge_attn_states, exact results, repeatability, given outputs, guard bands, a hipGraph
replayed after the lengths changed."""
import ctypes
import functools
import math
from ctypes import c_float, c_int, c_int64, c_void_p

import pytest
import torch

import mla_prefill_needles as mn
import mla_prefill_ref as ref
from utils import attn_close, attn_rel_err

D_QK, D_V = ref.DIM_QK, ref.DIM_V


# ---- CPU 1: the statement ----------------------------------------------------------------------------------------------------
def _tiny(Sq, Lk, H=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Sq, H, D_QK, generator=g).to(torch.bfloat16)
    kn = torch.randn(Lk, H, 128, generator=g).to(torch.bfloat16)
    kp = torch.randn(Lk, 64, generator=g).to(torch.bfloat16)
    v = torch.randn(Lk, H, D_V, generator=g).to(torch.bfloat16)
    return q, kn, kp, v


def test_statement_one_key_is_the_keys_v_row():
    q, kn, kp, v = _tiny(1, 1)
    out, lse = ref.prefill_statement(q, kn, kp, v, [0, 1], None, ref.SCALE)
    assert torch.equal(out.to(torch.bfloat16), v)
    z = ref.SCALE * ((q[0, :, :128].double() * kn[0].double()).sum(-1) + q[0, :, 128:].double() @ kp[0].double())
    assert torch.allclose(lse[0], z, rtol=0, atol=1e-12)


def test_statement_zero_q_is_the_mean():
    q, kn, kp, v = _tiny(5, 40)
    out, lse = ref.prefill_statement(torch.zeros_like(q), kn, kp, v, [0, 5], [0, 40], ref.SCALE, causal=False)
    assert torch.allclose(out[2], v.double().mean(0), rtol=0, atol=1e-12)
    assert torch.allclose(lse, torch.full_like(lse, math.log(40)), rtol=0, atol=1e-12)


def test_statement_causal_row_is_a_one_row_request():
    q, kn, kp, v = _tiny(4, 21)
    out, lse = ref.prefill_statement(q, kn, kp, v, [0, 4], [0, 21], ref.SCALE)
    for s in range(4):  # row s = a one-row request over the first 18 + s keys
        n = 21 - 4 + s + 1
        alone, l1 = ref.prefill_statement(q[s: s + 1], kn[:n], kp[:n], v[:n], [0, 1], [0, n], ref.SCALE)
        assert torch.allclose(out[s], alone[0], rtol=0, atol=1e-12) and torch.allclose(lse[s], l1[0], rtol=0, atol=1e-12)


def test_statement_without_keys_is_zeros_and_minus_inf():
    q, kn, kp, v = _tiny(3, 0)
    out, lse = ref.prefill_statement(q, kn, kp, v, [0, 3], [0, 0], ref.SCALE, causal=False)
    assert not out.any() and bool((lse == float("-inf")).all())
    q, kn, kp, v = _tiny(5, 2)  # causal, more rows than keys: the first three rows see nothing
    out, lse = ref.prefill_statement(q, kn, kp, v, [0, 5], [0, 2], ref.SCALE)
    assert not out[:3].any() and bool((lse[:3] == float("-inf")).all()) and bool(torch.isfinite(lse[3:]).all())
    assert torch.equal(out[3].to(torch.bfloat16), v[0])


# ---- CPU 2: the bars ---------------------------------------------------------------------------------------------------------
EDGE_LENS = [1, 2, 63, 64, 65, 127, 128, 129, 193, 700]
CTX_SQ, CTX_LK = (1, 64, 129), (0, 1, 63, 64, 65, 500)


def _context_batch(H, seed):
    """Sq in {1, 64, 129} against Lk in {0, 1, 63, 64, 65, 500}, one request each"""
    sq = [s for s in CTX_SQ for _ in CTX_LK]
    lk = [l for _ in CTX_SQ for l in CTX_LK]
    return mn.needle_inputs(sq, lk, H, causal=False, seed=seed)


def _causal_context_batch(H, seed):
    """causal with Lk > Sq (a cached prefix) and Lk < Sq (the first rows see no key)"""
    return mn.needle_inputs([5, 64, 129, 70, 129, 3, 200], [70, 64 + 129, 129 + 1, 5, 64, 1, 700], H, causal=True, seed=seed)


@functools.lru_cache(maxsize=None)
def _calibration():
    return [mn.needle_inputs(EDGE_LENS, None, 3, seed=11), mn.needle_inputs([1100], None, 2, seed=12), _context_batch(2, 13),
            _causal_context_batch(2, 14)]


def test_online_model_within_bars():
    """the online model passes both bars on the calibration cases, and each bar is at most 3 x the model's worst case"""
    w_tau, w_lse, min_scale = 0.0, 0.0, float("inf")
    for inp in _calibration():
        r, rl = mn.statement(inp)
        out, l = mn.online_model(inp)
        w_tau = max(w_tau, float(attn_rel_err(r, out).max()))
        w_lse = max(w_lse, ref.lse_err(rl, l))
        live = torch.isfinite(rl)
        min_scale = min(min_scale, float(r.float().abs().amax(-1)[live].min()))
    print(f"\nonline model worst out {w_tau:.5f} (tau {mn.TAU_NEEDLE} = {mn.TAU_NEEDLE / w_tau:.2f} x), worst lse {w_lse:.3g} "
          f"(bar {mn.LSE_BAR_NEEDLE} = {mn.LSE_BAR_NEEDLE / w_lse:.2f} x); smallest live row scale {min_scale:.3g}")
    assert w_tau <= mn.TAU_NEEDLE <= 3 * w_tau, (w_tau, mn.TAU_NEEDLE)
    assert w_lse <= mn.LSE_BAR_NEEDLE <= 3 * w_lse, (w_lse, mn.LSE_BAR_NEEDLE)
    assert min_scale >= 0.1, min_scale  # every live row has |y| of the order of V: the floor of attn_close never comes into play


def test_needle_bar_rejects_mutants():
    """each mutant of a plausible kernel bug, run through the statement, is >= 3 tau off"""
    inp = mn.needle_inputs([1, 37, 128, 300, 5, 64, 1100, 130], None, 4, seed=5)
    r, _ = mn.statement(inp)
    mutants = {
        "k_pe ignored": mn.statement(inp, use_pe=False)[0],
        "k_pe taken per head from the wrong row": mn.statement(inp, pe_row_of_head=True)[0],
        "v read from the k_nope half": mn.statement(inp, v_from_k_nope=True)[0],
        "causal limit + 1": mn.statement(inp, causal_shift=1)[0],
        "causal limit - 1": mn.statement(inp, causal_shift=-1)[0],
        "the last key of a 64-tile lost": mn.statement(inp, drop=lambda L: range(63, L, 64))[0],
        "softmax scale 1/sqrt(128)": mn.statement(inp, scale=1 / math.sqrt(128))[0],
        "zeros": torch.zeros_like(r),
    }
    # the alignment of the causal mask shows only where q and k counts differ
    ctx = _causal_context_batch(4, 6)
    rc, _ = mn.statement(ctx)
    short = []
    for name, (want, y) in dict({k: (r, y) for k, y in mutants.items()},
                                **{"top-left instead of bottom-right alignment": (rc, mn.statement(ctx, top_left=True)[0])}).items():
        m = float(attn_rel_err(want, y).max()) / mn.TAU_NEEDLE
        print(f"  {name:48s} {m:9.1f} tau")
        if not m >= 3:
            short.append((name, m))
    assert not short, short
    assert attn_close(r, mn.online_model(inp)[0], mn.TAU_NEEDLE)


# ---- CPU 3: surface and fakes ------------------------------------------------------------------------------------------------
def test_surface():
    import hpc

    assert "attention_prefill_mla_bf16" in hpc.__all__ and callable(hpc.attention_prefill_mla_bf16)
    doc = hpc.attention_prefill_mla_bf16.__doc__
    for word in ("softmax_scale", "192", "128", "k_pe", "cu_seqlens_k", "max_seqlens_k", "bottom-right", "-inf", "hipGraph",
                 "natural log", "bit-identical", "65535", "tests/mla_prefill_ref.py", "mla_rope_norm_store_kv"):
        assert word in doc, word


def test_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        q = torch.empty(30, 5, D_QK, dtype=torch.bfloat16, device="cuda")
        kv = torch.empty(90, 5, 256, dtype=torch.bfloat16, device="cuda")
        ckv = torch.empty(90, 576, dtype=torch.bfloat16, device="cuda")
        cu = torch.empty(4, dtype=torch.int32, device="cuda")
        kn, v, kp = kv[..., :128], kv[..., 128:], ckv[:, 512:]
        out, lse = torch.ops.hpc_mla.attention_prefill_mla_bf16(q, kn, kp, v, cu, 12, 0.07, cu, 40, False, None, None, True)
        assert (out.shape, out.dtype, lse.shape, lse.dtype) == ((30, 5, D_V), torch.bfloat16, (30, 5), torch.float32)
        out, lse = torch.ops.hpc_mla.attention_prefill_mla_bf16(q, kn, kp, v, cu, 12, 0.07, None, None, True, None, None, False)
        assert out.shape == (30, 5, D_V) and lse.numel() == 0
        y = hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu, 12, 0.07)
        assert isinstance(y, torch.Tensor) and y.shape == (30, 5, D_V) and y.device.type == "cuda"
        y, l = hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu, 12, 0.07, cu_seqlens_k=cu, max_seqlens_k=40, causal=False,
                                              return_lse=True)
        assert y.shape == (30, 5, D_V) and l.shape == (30, 5)
        o = torch.empty(30, 5, D_V, dtype=torch.bfloat16, device="cuda")
        ol = torch.empty(30, 5, dtype=torch.float32, device="cuda")
        assert hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu, 12, 0.07, output=o) is o
        y, l = hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu, 12, 0.07, output=o, output_lse=ol)
        assert y is o and l is ol
        y, l = hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu, 12, 0.07, output_lse=ol)
        assert y.shape == (30, 5, D_V) and l is ol


# ---- CPU 4: the C-ABI refuses on the host -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def call(lib, *, out=4096, lse=4096, q=4096, k_nope=4096, k_pe=4096, v=4096, cu_q=4096, cu_k=None, B=2, H=4, max_q=100,
         max_k=-1, q_row=4 * 192, q_head=192, k_row=4 * 256, k_head=256, pe_row=576, v_row=4 * 256, v_head=256, scale=0.07,
         causal=1):
    """hpc_attention_prefill_mla_bf16_async with pointers that are never dereferenced on the host"""
    ip = lambda p: ctypes.cast(c_void_p(p), ctypes.POINTER(c_int)) if p else None  # noqa: E731
    vp = lambda p: c_void_p(p) if p else None  # noqa: E731
    return lib.hpc_attention_prefill_mla_bf16_async(vp(out), vp(lse), vp(q), vp(k_nope), vp(k_pe), vp(v), ip(cu_q), ip(cu_k), B, H,
                                                    max_q, max_k, c_int64(q_row), c_int64(q_head), c_int64(k_row), c_int64(k_head),
                                                    c_int64(pe_row), c_int64(v_row), c_int64(v_head), c_float(scale), causal, None)


UNSUPPORTED, INVALID = -1, -2


@pytest.mark.parametrize("kwargs,code", [
    (dict(out=0), INVALID), (dict(q=0), INVALID), (dict(k_nope=0), INVALID), (dict(k_pe=0), INVALID), (dict(v=0), INVALID),
    (dict(cu_q=0), INVALID),
    (dict(q=4096 + 8), UNSUPPORTED), (dict(k_pe=4096 + 2), UNSUPPORTED), (dict(out=4096 + 4), UNSUPPORTED),
    (dict(lse=4096 + 2), UNSUPPORTED), (dict(q_row=4 * 192 + 4), UNSUPPORTED), (dict(q_head=196), UNSUPPORTED),
    (dict(k_row=1028), UNSUPPORTED), (dict(k_head=132), UNSUPPORTED), (dict(pe_row=580), UNSUPPORTED),
    (dict(v_row=1028), UNSUPPORTED), (dict(v_head=132), UNSUPPORTED),
    (dict(q_row=184), UNSUPPORTED), (dict(q_head=128), UNSUPPORTED), (dict(k_row=120), UNSUPPORTED), (dict(k_head=64), UNSUPPORTED),
    (dict(pe_row=56), UNSUPPORTED), (dict(v_row=64), UNSUPPORTED), (dict(v_head=120), UNSUPPORTED),
    (dict(cu_k=4096), INVALID), (dict(cu_k=4096, max_k=-5), INVALID),
    (dict(B=-1), INVALID), (dict(max_q=-1), INVALID), (dict(H=0), INVALID), (dict(H=-3), INVALID), (dict(scale=0.0), INVALID),
    (dict(scale=-0.1), INVALID), (dict(scale=float("nan")), INVALID), (dict(scale=float("inf")), INVALID),
    (dict(H=65536), UNSUPPORTED), (dict(B=65536), UNSUPPORTED), (dict(k_row=(1 << 25) + 8), UNSUPPORTED),
    (dict(pe_row=(1 << 25) + 8), UNSUPPORTED),
])
def test_cabi_refuses_on_the_host(lib, kwargs, code):
    assert call(lib, **kwargs) == code


def test_cabi_refusals_come_in_the_routes_order(lib):
    """a call with two faults gets the code of the earlier check: null < alignment < narrow strides < cu_seqlens_k without its
    maximum < negative counts < the grid limits"""
    assert call(lib, q=0, q_row=4) == INVALID            # null before alignment
    assert call(lib, q_row=188, B=-1) == UNSUPPORTED     # alignment before negative counts
    assert call(lib, k_head=64, cu_k=4096) == UNSUPPORTED  # narrow strides before cu_seqlens_k without max_seqlens_k
    assert call(lib, cu_k=4096, H=65536) == INVALID      # ... which comes before the grid limits
    assert call(lib, B=-1, H=65536) == INVALID           # negative counts before the grid limits
    assert call(lib, H=65536, B=0) == UNSUPPORTED        # the limits before the empty call


def test_cabi_takes_an_empty_call(lib):
    assert call(lib, B=0) == 0 and call(lib, max_q=0) == 0  # nothing to launch: no device call either
    assert call(lib, lse=0, B=0) == 0                        # lse may be null
    assert call(lib, cu_k=4096, max_k=0, B=0) == 0


def _grid(B, H, max_q):
    """the arithmetic of csrc/attention_prefill_mla_route.h, restated: (128-position q tiles of the longest request, heads,
    requests) - the kernel's workgroup is 4 waves x 32 positions of one head"""
    return (-(-max_q // 128), H, B)


def test_the_grid_is_the_routes():
    """the grid itself cannot be read back through the C-ABI; what is observable on the host is where it ends: one more head or
    request than the grid's y / z hold is refused, the largest legal ones are not (an empty call: nothing is launched)"""
    assert _grid(3, 5, 129) == (2, 5, 3) and _grid(1, 1, 128) == (1, 1, 1) and _grid(2, 65535, 1) == (1, 65535, 2)
    from hpc import _C

    assert call(_C.lib, H=65535, B=0) == 0 and call(_C.lib, H=65536, B=0) == UNSUPPORTED
    assert call(_C.lib, B=65535, max_q=0) == 0 and call(_C.lib, B=65536, max_q=0) == UNSUPPORTED


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _to_gpu(inp):
    g = dict(inp)
    for k in ("q", "kv", "ckv", "cu_q", "cu_k"):
        g[k] = None if inp[k] is None else inp[k].cuda()
    return mn.with_views(g)


def _run(g, contiguous=False, return_lse=True, **kw):
    import hpc

    kn, kp, v = g["k_nope"], g["k_pe"], g["v"]
    if contiguous:
        kn, kp, v = kn.contiguous(), kp.contiguous(), v.contiguous()
    else:
        assert not kn.is_contiguous() and not v.is_contiguous() and kp.stride(0) == 576
    extra = {} if g["cu_k"] is None else dict(cu_seqlens_k=g["cu_k"], max_seqlens_k=g["max_k"])
    return hpc.attention_prefill_mla_bf16(g["q"], kn, kp, v, g["cu_q"], g["max_q"], g["scale"], causal=g["causal"],
                                          return_lse=return_lse, **extra, **kw)


def _check(want, got, label):
    (r, rl), (out, lse) = want, got
    w_out, w_lse = float(attn_rel_err(r, out.cpu()).max()), ref.lse_err(rl, lse)
    print(f"{label}: out worst {w_out:.5f} (tau {mn.TAU_NEEDLE}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_NEEDLE})")
    assert attn_close(r, out.cpu(), mn.TAU_NEEDLE, label=label)
    assert w_lse <= mn.LSE_BAR_NEEDLE, (label, w_lse, mn.LSE_BAR_NEEDLE)


@functools.lru_cache(maxsize=None)
def _edge_case(H):
    inp = mn.needle_inputs(EDGE_LENS, None, H, seed=100 + H)
    return inp, mn.statement(inp)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 3, 16])
def test_needle_parity_ragged_batch(H):
    inp, want = _edge_case(H)
    g = _to_gpu(inp)
    got = _run(g)
    _check(want, got, f"ragged H {H}")
    if H == 3:  # once through contiguous tensors: the same bits
        again = _run(g, contiguous=True)
        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.gpu
def test_needle_parity_33_tiles():
    inp = mn.needle_inputs([2100], None, 2, seed=7)
    _check(mn.statement(inp), _run(_to_gpu(inp)), "2100 tokens H 2")


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 4])
def test_context_form(H):
    inp = _context_batch(H, 20 + H)
    want = mn.statement(inp)
    out, lse = _run(_to_gpu(inp))
    _check(want, (out, lse), f"context H {H}")
    cu = inp["cu_q"].tolist()
    for i, lk in enumerate(inp["seq_k"]):  # Lk == 0: zeros and -inf, exactly
        if lk == 0:
            assert not out[cu[i]: cu[i + 1]].any() and bool((lse[cu[i]: cu[i + 1]] == float("-inf")).all())
    inp = _causal_context_batch(H, 30 + H)
    want = mn.statement(inp)
    assert bool(torch.isinf(want[1]).any()) and bool(torch.isfinite(want[1]).any())  # rows without a key among the others
    _check(want, _run(_to_gpu(inp)), f"causal context H {H}")


@pytest.mark.gpu
def test_chunked_equals_whole():
    """a request of 300 tokens cut at c: the self pass on [c:] merged with the context pass of q[c:] over [:c] is rows c.. of the
    whole causal call"""
    import hpc

    H, L = 3, 300
    inp = mn.needle_inputs([L], None, H, seed=41)
    g = _to_gpu(inp)
    whole, whole_lse = _run(g)
    _check(mn.statement(inp), (whole, whole_lse), "whole")
    q, kn, kp, v = g["q"], g["k_nope"], g["k_pe"], g["v"]
    for c in (0, 1, 64, 65, 299):
        n = L - c
        cu_self = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        cu_ctx = torch.tensor([0, c], dtype=torch.int32, device="cuda")
        a, la = hpc.attention_prefill_mla_bf16(q[c:], kn[c:], kp[c:], v[c:], cu_self, n, mn.SCALE, return_lse=True)
        b, lb = hpc.attention_prefill_mla_bf16(q[c:], kn[:c], kp[:c], v[:c], cu_self, n, mn.SCALE, cu_seqlens_k=cu_ctx,
                                               max_seqlens_k=c, causal=False, return_lse=True)
        out, lse = hpc.merge_attn_states(a, la, b, lb)
        w_out = float(attn_rel_err(whole[c:].cpu(), out.cpu()).max())
        w_lse = ref.lse_err(whole_lse[c:].double().cpu(), lse)
        print(f"cut {c}: out worst {w_out:.5f} (tau {mn.TAU_NEEDLE}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_NEEDLE})")
        assert attn_close(whole[c:].cpu(), out.cpu(), mn.TAU_NEEDLE, label=f"cut {c}")
        assert w_lse <= mn.LSE_BAR_NEEDLE, (c, w_lse)
        if c == 0:  # no context: the self pass goes through bit for bit, and it is the whole call
            assert not b.any() and bool((lb == float("-inf")).all())
            assert torch.equal(out, a) and torch.equal(lse, la)
            assert torch.equal(a, whole) and torch.equal(la, whole_lse)


@pytest.mark.gpu
def test_uniform_scores_are_exact():
    """zero q over a power-of-two count of identical v rows: every probability is the same power of two, out is the v row
    exactly and lse = log(count) to the lse bar"""
    import hpc

    H = 3
    counts = [1, 2, 64, 128, 512]
    g = torch.Generator().manual_seed(3)
    cu_k = torch.tensor([0] + counts, dtype=torch.int32).cumsum(0).to(torch.int32)
    rows = torch.randn(len(counts), H, D_V, generator=g).to(torch.bfloat16)
    v = torch.cat([rows[i: i + 1].expand(n, H, D_V) for i, n in enumerate(counts)]).contiguous().cuda()
    kn = torch.randn(int(cu_k[-1]), H, 128, generator=g).to(torch.bfloat16).cuda()
    kp = torch.randn(int(cu_k[-1]), 64, generator=g).to(torch.bfloat16).cuda()
    sq = 70
    cu_q = (torch.arange(len(counts) + 1) * sq).to(torch.int32)
    q = torch.zeros(sq * len(counts), H, D_QK, dtype=torch.bfloat16, device="cuda")
    out, lse = hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu_q.cuda(), sq, mn.SCALE, cu_seqlens_k=cu_k.cuda(),
                                              max_seqlens_k=max(counts), causal=False, return_lse=True)
    for i, n in enumerate(counts):
        assert torch.equal(out[i * sq: (i + 1) * sq].cpu(), rows[i][None].expand(sq, H, D_V)), n
        want = torch.full((sq, H), math.log(n), dtype=torch.float64)
        assert ref.lse_err(want, lse[i * sq: (i + 1) * sq]) <= mn.LSE_BAR_NEEDLE, n


@pytest.mark.gpu
def test_two_calls_are_bit_identical_and_given_outputs_are_returned():
    inp, _ = _edge_case(3)
    g = _to_gpu(inp)
    first = _run(g)
    again = _run(g)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    o = torch.zeros_like(first[0])
    ol = torch.zeros_like(first[1])
    y, l = _run(g, output=o, output_lse=ol)
    assert y is o and l is ol and torch.equal(o, first[0]) and torch.equal(ol, first[1])
    y = _run(g, return_lse=False, output=o)
    assert y is o
    y = _run(g, return_lse=False)
    assert isinstance(y, torch.Tensor) and torch.equal(y, first[0])


GUARD, PATTERN = 1 << 20, 0xFF  # NaN bytes


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 5])
def test_guard_bands_stay_untouched(lib, H):
    """out and lse between 1 MiB bands of NaN bytes, through the C-ABI: the bands are intact afterwards, rows of requests shorter
    than max_seqlens_q included"""
    inp = mn.needle_inputs([5, 129, 1, 200], None, H, seed=17)
    g = _to_gpu(inp)
    Tq = g["q"].shape[0]
    sizes = [Tq * H * D_V * 2, Tq * H * 4]
    bufs = [torch.full((2 * GUARD + n,), PATTERN, dtype=torch.uint8, device="cuda") for n in sizes]
    kn, kp, v, q = g["k_nope"], g["k_pe"], g["v"], g["q"]
    torch.cuda.synchronize()
    rc = call(lib, out=bufs[0].data_ptr() + GUARD, lse=bufs[1].data_ptr() + GUARD, q=q.data_ptr(), k_nope=kn.data_ptr(),
              k_pe=kp.data_ptr(), v=v.data_ptr(), cu_q=g["cu_q"].data_ptr(), B=4, H=H, max_q=200, q_row=q.stride(0),
              q_head=q.stride(1), k_row=kn.stride(0), k_head=kn.stride(1), pe_row=kp.stride(0), v_row=v.stride(0),
              v_head=v.stride(1), scale=mn.SCALE)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in zip(bufs, sizes):
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all())
    out = bufs[0][GUARD: GUARD + sizes[0]].view(torch.bfloat16).reshape(Tq, H, D_V)
    lse = bufs[1][GUARD: GUARD + sizes[1]].view(torch.float32).reshape(Tq, H)
    _check(mn.statement(inp), (out, lse), f"guards H {H}")


@pytest.mark.gpu
def test_graph_replays_with_new_lengths():
    """capture with every output given; replay; change cu_seqlens_q / cu_seqlens_k in place (same maxima); replay: the new
    lengths' result"""
    import hpc

    H = 2
    a = mn.needle_inputs([64, 5, 129], [64 + 70, 5, 129 + 200], H, seed=31)
    b = mn.needle_inputs([129, 3, 40], [129 + 200, 20, 41], H, seed=32)
    assert (a["max_q"], a["max_k"]) == (b["max_q"], b["max_k"])
    rows_q = max(a["q"].shape[0], b["q"].shape[0])
    rows_k = max(a["kv"].shape[0], b["kv"].shape[0])
    q = torch.zeros(rows_q, H, D_QK, dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros(rows_k, H, 256, dtype=torch.bfloat16, device="cuda")
    ckv = torch.zeros(rows_k, 576, dtype=torch.bfloat16, device="cuda")
    cu_q = torch.zeros(4, dtype=torch.int32, device="cuda")
    cu_k = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(rows_q, H, D_V, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(rows_q, H, dtype=torch.float32, device="cuda")
    kn, v, kp = kv[mn.PAD:, :, :128], kv[mn.PAD:, :, 128:], ckv[mn.PAD:, 512:]

    def load(inp):
        kv.fill_(mn.POISON)
        ckv.fill_(mn.POISON)
        q.zero_()
        q[: inp["q"].shape[0]].copy_(inp["q"])
        kv[: inp["kv"].shape[0]].copy_(inp["kv"])
        ckv[: inp["ckv"].shape[0]].copy_(inp["ckv"])
        cu_q.copy_(inp["cu_q"])
        cu_k.copy_(inp["cu_k"])

    def step():
        return hpc.attention_prefill_mla_bf16(q, kn, kp, v, cu_q, a["max_q"], mn.SCALE, cu_seqlens_k=cu_k, max_seqlens_k=a["max_k"],
                                              output=out, output_lse=lse)

    load(a)
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
        assert torch.cuda.memory_allocated() == before  # nothing allocated in the capture
    for inp in (a, b, a):
        load(inp)
        out.zero_()
        lse.zero_()
        graph.replay()
        torch.cuda.synchronize()
        n = inp["q"].shape[0]
        _check(mn.statement(inp), (out[:n], lse[:n]), "graph")


@pytest.mark.gpu
def test_empty_calls_and_refusals():
    import hpc

    inp = mn.needle_inputs([5, 3], None, 2, seed=1)
    g = _to_gpu(inp)
    empty_q = g["q"][:0]
    cu0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    out, lse = hpc.attention_prefill_mla_bf16(empty_q, g["k_nope"], g["k_pe"], g["v"], cu0, 0, mn.SCALE, return_lse=True)
    assert out.shape == (0, 2, D_V) and lse.shape == (0, 2)
    with pytest.raises(RuntimeError, match="max_seqlens_k"):
        hpc.attention_prefill_mla_bf16(g["q"], g["k_nope"], g["k_pe"], g["v"], g["cu_q"], 5, mn.SCALE, cu_seqlens_k=g["cu_q"])
    with pytest.raises(RuntimeError, match="launch failed"):
        hpc.attention_prefill_mla_bf16(g["q"], g["k_nope"], g["k_pe"], g["v"], g["cu_q"], 5, 0.0)
    with pytest.raises(RuntimeError, match="k_pe"):
        hpc.attention_prefill_mla_bf16(g["q"], g["k_nope"], g["k_pe"][:, :32], g["v"], g["cu_q"], 5, mn.SCALE)
