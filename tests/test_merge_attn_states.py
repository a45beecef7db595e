"""hpc.merge_attn_states: two attention states merged by their log-sum-exps.

CPU: the fp32 model of the kernel's arithmetic against the float64 statement (tests/mla_prefill_ref.py::merge_statement) - the
bars of tests/mla_prefill_needles.py measured again, model <= bar <= 3 x model; mutants rejected at >= 3 tau; the -inf rules of
the statement; surface, fakes, host refusals through the C-ABI with never-dereferenced pointers (the overlap rule among them).
GPU: random states with lse spread over +-30, one- and two-sided -inf, in place, strided, D in {8, 128, 512}, repeatability,
guard bands."""
import ctypes
from ctypes import c_int64, c_void_p

import pytest
import torch

import mla_prefill_needles as mn
import mla_prefill_ref as ref
from utils import attn_close, attn_rel_err

# (T, H, D): the cases the merge bars are calibrated on and the kernel runs on
CASES = [(37, 3, 8), (300, 5, 128), (65, 2, 512), (1, 1, 24)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_merge_model_within_bars():
    w_tau, w_lse = 0.0, 0.0
    for i, (T, H, D) in enumerate(CASES):
        st = mn.merge_inputs(T, H, D, seed=i)
        r, rl = ref.merge_statement(*st)
        out, l = mn.merge_model(*st)
        w_tau = max(w_tau, float(attn_rel_err(r, out.double()).max()))  # against the unrounded statement
        w_lse = max(w_lse, ref.lse_err(rl, l))
    print(f"\nmerge model worst out {w_tau:.5f} (tau {mn.TAU_MERGE} = {mn.TAU_MERGE / w_tau:.2f} x), worst lse {w_lse:.3g} "
          f"(bar {mn.LSE_BAR_MERGE} = {mn.LSE_BAR_MERGE / w_lse:.2f} x)")
    assert w_tau <= mn.TAU_MERGE <= 3 * w_tau, (w_tau, mn.TAU_MERGE)
    assert w_lse <= mn.LSE_BAR_MERGE <= 3 * w_lse, (w_lse, mn.LSE_BAR_MERGE)


def test_merge_bar_rejects_mutants():
    st = mn.merge_inputs(300, 5, 128, seed=3, dead=False)
    r, rl = ref.merge_statement(*st)
    swapped = ref.merge_statement(*st, swap_weights=True)[0]
    m = float(attn_rel_err(r, swapped).max()) / mn.TAU_MERGE
    print(f"  weights swapped {m:9.1f} tau")
    assert m >= 3
    lse_max = ref.merge_statement(*st, lse_is_max=True)[1]
    worst = ref.lse_err(rl, lse_max)
    print(f"  lse = m only    {worst / mn.LSE_BAR_MERGE:9.1f} lse bars")
    assert worst >= 3 * mn.LSE_BAR_MERGE
    assert attn_close(r, mn.merge_model(*st)[0].double(), mn.TAU_MERGE)


def test_statement_passes_a_side_through():
    a, la, b, lb = mn.merge_inputs(6, 2, 16, seed=1, dead=False)
    dead = torch.full_like(la, float("-inf"))
    out, lse = ref.merge_statement(a, la, b, dead)
    assert torch.equal(out, a.double()) and torch.equal(lse, la.double())
    out, lse = ref.merge_statement(a, dead, b, lb)
    assert torch.equal(out, b.double()) and torch.equal(lse, lb.double())
    out, lse = ref.merge_statement(a, dead, b, dead)
    assert not out.any() and bool((lse == float("-inf")).all())
    out, lse = mn.merge_model(a, dead, b, lb)
    assert torch.equal(out, b) and torch.equal(lse, lb)


def test_merging_two_halves_is_the_whole():
    """the statement of the merge against the statement of the attention: keys 0..39 and 40..99 merged = keys 0..99"""
    g = torch.Generator().manual_seed(2)
    q = torch.randn(7, 2, 192, generator=g).to(torch.bfloat16)
    kn, kp = torch.randn(100, 2, 128, generator=g).to(torch.bfloat16), torch.randn(100, 64, generator=g).to(torch.bfloat16)
    v = torch.randn(100, 2, 128, generator=g).to(torch.bfloat16)
    whole, wl = ref.prefill_statement(q, kn, kp, v, [0, 7], [0, 100], ref.SCALE, causal=False)
    a, la = ref.prefill_statement(q, kn[:40], kp[:40], v[:40], [0, 7], [0, 40], ref.SCALE, causal=False)
    b, lb = ref.prefill_statement(q, kn[40:], kp[40:], v[40:], [0, 7], [0, 60], ref.SCALE, causal=False)
    out, lse = ref.merge_statement(a, la, b, lb)
    assert torch.allclose(out, whole, rtol=0, atol=1e-12) and torch.allclose(lse, wl, rtol=0, atol=1e-12)


def test_surface_and_fakes():
    import hpc
    from torch._subclasses.fake_tensor import FakeTensorMode

    assert "merge_attn_states" in hpc.__all__ and callable(hpc.merge_attn_states)
    doc = hpc.merge_attn_states.__doc__
    for word in ("max(la, lb)", "-inf", "bit for bit", "in place", "D % 8 == 0", "512", "refused", "merge_statement"):
        assert word in doc, word
    with FakeTensorMode():
        a = torch.empty(9, 4, 128, dtype=torch.bfloat16, device="cuda")
        la = torch.empty(9, 4, dtype=torch.float32, device="cuda")
        out, lse = hpc.merge_attn_states(a, la, a, la)
        assert (out.shape, out.dtype, lse.shape, lse.dtype) == ((9, 4, 128), torch.bfloat16, (9, 4), torch.float32)
        o, ol = torch.empty_like(a), torch.empty_like(la)
        y, l = hpc.merge_attn_states(a, la, a, la, output=o, output_lse=ol)
        assert y is o and l is ol
        y, l = hpc.merge_attn_states(a, la, o, ol, output=a, output_lse=la)
        assert y is a and l is la


@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


MB = 1 << 20


def call(lib, *, out=1 * MB, lse=2 * MB, a=3 * MB, la=4 * MB, b=5 * MB, lb=6 * MB, T=10, H=4, D=128, o_row=None, o_head=None,
         a_row=None, a_head=None, b_row=None, b_head=None):
    """hpc_merge_attn_states_async with pointers that are never dereferenced on the host (1 MiB apart: disjoint at these sizes)"""
    fp = lambda p: ctypes.cast(c_void_p(p), ctypes.POINTER(ctypes.c_float)) if p else None  # noqa: E731
    vp = lambda p: c_void_p(p) if p else None  # noqa: E731
    st = lambda row, head: (c_int64(H * D if row is None else row), c_int64(D if head is None else head))  # noqa: E731
    return lib.hpc_merge_attn_states_async(vp(out), fp(lse), vp(a), fp(la), vp(b), fp(lb), c_int64(T), H, D, *st(o_row, o_head),
                                           *st(a_row, a_head), *st(b_row, b_head), None)


UNSUPPORTED, INVALID = -1, -2


@pytest.mark.parametrize("kwargs,code", [
    (dict(out=0), INVALID), (dict(lse=0), INVALID), (dict(a=0), INVALID), (dict(la=0), INVALID), (dict(b=0), INVALID),
    (dict(lb=0), INVALID), (dict(T=-1), INVALID), (dict(H=-1), INVALID),
    (dict(D=0), UNSUPPORTED), (dict(D=12), UNSUPPORTED), (dict(D=520), UNSUPPORTED), (dict(out=MB + 8), UNSUPPORTED),
    (dict(b=5 * MB + 2), UNSUPPORTED), (dict(la=4 * MB + 2), UNSUPPORTED), (dict(a_row=4 * 128 + 4), UNSUPPORTED),
    (dict(o_head=120), UNSUPPORTED), (dict(b_head=132), UNSUPPORTED),
    # overlap: an output on the b side, a shifted a side, in place with other strides, the lse on lse_b
    (dict(out=5 * MB), UNSUPPORTED), (dict(out=3 * MB + 256), UNSUPPORTED), (dict(out=3 * MB, o_row=8 * 128), UNSUPPORTED),
    (dict(lse=6 * MB), UNSUPPORTED), (dict(lse=4 * MB + 16), UNSUPPORTED), (dict(out=4 * MB), UNSUPPORTED),
])
def test_cabi_refuses_on_the_host(lib, kwargs, code):
    assert call(lib, **kwargs) == code


def test_cabi_takes_an_empty_call(lib):
    assert call(lib, T=0) == 0 and call(lib, H=0, o_row=128, a_row=128, b_row=128) == 0  # nothing to launch: no device call either
    assert call(lib, T=0, out=3 * MB, lse=4 * MB) == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _check(st, out, lse, label):
    r, rl = ref.merge_statement(*[t.cpu() for t in st])
    got = out.cpu().double()  # against the unrounded statement: the bar holds the one rounding to bf16
    w_out, w_lse = float(attn_rel_err(r, got).max()), ref.lse_err(rl, lse)
    print(f"{label}: out worst {w_out:.5f} (tau {mn.TAU_MERGE}), lse worst {w_lse:.3g} (bar {mn.LSE_BAR_MERGE})")
    assert attn_close(r, got, mn.TAU_MERGE, label=label)
    assert w_lse <= mn.LSE_BAR_MERGE, (label, w_lse)


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,D", CASES)
def test_random_states(T, H, D):
    import hpc

    st = [t.cuda() for t in mn.merge_inputs(T, H, D, seed=T)]
    out, lse = hpc.merge_attn_states(*st)
    _check(st, out, lse, f"T {T} H {H} D {D}")
    again = hpc.merge_attn_states(*st)
    assert torch.equal(again[0], out) and torch.equal(again[1], lse)
    a, la, b, lb = st
    n = T * H
    if n >= 6:  # the rows merge_inputs killed: one side passes through bit for bit, both give zeros and -inf
        fo, fa, fb = out.view(n, D), a.view(n, D), b.view(n, D)
        assert torch.equal(fo[0], fb[0]) and float(lse.view(-1)[0]) == float(lb.view(-1)[0])
        assert torch.equal(fo[n // 2], fa[n // 2]) and float(lse.view(-1)[n // 2]) == float(la.view(-1)[n // 2])
        assert not fo[n - 1].any() and float(lse.view(-1)[n - 1]) == float("-inf")


@pytest.mark.gpu
def test_one_side_dead_everywhere_is_a_copy():
    import hpc

    a, la, b, lb = [t.cuda() for t in mn.merge_inputs(70, 3, 128, seed=9, dead=False)]
    a[0, 0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=torch.bfloat16)  # signed zeros and tiny values survive
    dead = torch.full_like(la, float("-inf"))
    out, lse = hpc.merge_attn_states(a, la, b, dead)
    assert torch.equal(out.view(torch.int16), a.view(torch.int16)) and torch.equal(lse, la)
    out, lse = hpc.merge_attn_states(b, dead, a, la)
    assert torch.equal(out.view(torch.int16), a.view(torch.int16)) and torch.equal(lse, la)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [8, 24, 128, 512])
def test_in_place_and_strided(D):
    import hpc

    T, H = 130, 3
    st = [t.cuda() for t in mn.merge_inputs(T, H, D, seed=D)]
    want, want_lse = hpc.merge_attn_states(*st)
    # strided inputs and output: views into wider buffers, the gaps holding NaN bytes
    wide = [torch.full((T, H + 1, D + 8), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3)]
    va, vb, vo = (w[:, :H, :D] for w in wide)
    va.copy_(st[0])
    vb.copy_(st[2])
    out, lse = hpc.merge_attn_states(va, st[1], vb, st[3], output=vo)
    assert out is vo and torch.equal(vo, want) and torch.equal(lse, want_lse)
    assert bool(wide[2][:, H].isnan().all()) and bool(wide[2][:, :, D:].isnan().all())  # the gaps of the output are untouched
    # in place on the a side, out and lse
    la = st[1].clone()
    out, lse = hpc.merge_attn_states(va, la, vb, st[3], output=va, output_lse=la)
    assert out is va and lse is la and torch.equal(va, want) and torch.equal(la, want_lse)
    with pytest.raises(RuntimeError, match="launch failed"):
        hpc.merge_attn_states(st[0], st[1], st[2], st[3], output=st[2])  # the b side is no legal destination
    with pytest.raises(RuntimeError, match="launch failed"):
        hpc.merge_attn_states(st[0], st[1], st[2], st[3], output_lse=st[3])


GUARD, PATTERN = 1 << 20, 0xFF  # NaN bytes


@pytest.mark.gpu
def test_guard_bands_stay_untouched(lib):
    T, H, D = 77, 5, 128
    a, la, b, lb = [t.cuda() for t in mn.merge_inputs(T, H, D, seed=4)]
    sizes = [T * H * D * 2, T * H * 4]
    bufs = [torch.full((2 * GUARD + n,), PATTERN, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    rc = call(lib, out=bufs[0].data_ptr() + GUARD, lse=bufs[1].data_ptr() + GUARD, a=a.data_ptr(), la=la.data_ptr(), b=b.data_ptr(),
              lb=lb.data_ptr(), T=T, H=H, D=D)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in zip(bufs, sizes):
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all())
    out = bufs[0][GUARD: GUARD + sizes[0]].view(torch.bfloat16).reshape(T, H, D)
    lse = bufs[1][GUARD: GUARD + sizes[1]].view(torch.float32).reshape(T, H)
    _check((a, la, b, lb), out, lse, "guards")
