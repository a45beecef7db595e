"""hpc.gemm_bf16xfp32 (the router GEMM) against its float64 statement (tests/router_gemm_ref.py).

CPU: the premise of the exact inputs, their bf16 tie shares, the measured slack of the bar for general inputs, the planted errors
each bar must reject, what the sampled cases cover, the launcher's refusals of caller split counts.  GPU: exact inputs bit for bit
through the C ABI with every caller split count - the skinny kernels, the tile kernel's three reduce forms, the development
64 x 64 kernel, scales other than 1 / 256 -, the torch op on exact inputs, real inputs at the derived bar, and the chain into
hpc.topk_router on logits with exact ties between experts."""
import ctypes
import itertools
import math
import random

import pytest
import torch

import router_gemm_ref as rr

GUARD = 1 << 20
PATTERN = 0xA5
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def lib():
    from hpc import _C

    return _C.lib


def plan(lib, m, n, k, use_splitk=1):
    """(the library's split count, counter rows, counter row stride)"""
    s, rows, ld = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.hpc_gemm_bf16xfp32_plan(m, n, k, use_splitk, ctypes.byref(s), ctypes.byref(rows), ctypes.byref(ld)) == 0
    return s.value, rows.value, ld.value


def waves_of(m):
    """accumulator pairs a workgroup deals its 64-k steps to: the skinny kernels' four waves up to 256 tokens, one above"""
    return 4 if m <= 256 else 1


def cut(steps, splits):
    """64-k steps of every split: the kernels' [steps * s / splits, steps * (s + 1) / splits)"""
    return [steps * (s + 1) // splits - steps * s // splits for s in range(splits)]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _skinny_cases(seed=20240611):
    """60 of the (m, n, k, splits, fp32 output) grid with a fixed seed, splits within min(16, k / 64)."""
    grid = [c for c in itertools.product((1, 15, 16, 17, 32, 33, 64, 65, 200, 256), (64, 192), (64, 192, 448, 576, 1024, 2112),
                                         (1, 2, 3, 5, 7, 16), (True, False)) if c[3] <= min(16, c[2] // 64)]
    return sorted(random.Random(seed).sample(grid, 60))


def _tile_cases(seed=20240611):
    """48 of the (m, n, k, splits, fp32 output) grid above 256 tokens with a fixed seed."""
    grid = [c for c in itertools.product((257, 300, 384, 385), (64, 128), (64, 192, 320, 1024), (1, 2, 3, 4, 5, 8, 9, 16),
                                         (True, False)) if c[3] <= min(16, c[2] // 64)]
    return sorted(random.Random(seed).sample(grid, 48))


SKINNY_CASES = _skinny_cases()
TILE_CASES = _tile_cases()
SCALE_CASES = [(17, 64, 576, 3, 1 / 128), (65, 192, 1024, 16, 1 / 512), (33, 64, 448, 7, 1.0), (300, 128, 320, 5, 1 / 128),
               (385, 64, 1024, 9, 1 / 512), (257, 64, 192, 2, 1.0)]
REAL_CASES = [(17, 64, 4096, (1, 3, 16)), (33, 64, 2112, (1, 3, 16)), (64, 128, 7168, (1, 3, 16)), (300, 64, 4096, (1, 5, 16))]
ROUTING_CASES = [(40, 64, 64, 1.0), (300, 256, 192, 0.25)]
TOPK = 8


# ---- CPU: the exact inputs ---------------------------------------------------------------------------------------------------------
def test_exact_inputs_are_exact_in_any_order_and_split():
    """The exact grid's premise: the float32 model of the kernels, with one and with four accumulators and split 1, 2, 3, 7 and
    16 ways, returns float32(statement) bit for bit, and its bf16 rounding is the statement's; so does a plain float32 matmul
    of each plane, whatever order the BLAS takes."""
    for (m, n, k), scale in (((17, 64, 2112), 1 / 256), ((5, 64, 1024), 1 / 512), ((9, 128, 448), 1.0)):
        x, wh, wl, want32, want16, _ = rr.exact_case(m, n, k, scale)
        for waves, splits in itertools.product((1, 4), (1, 2, 3, 7, 16)):
            if splits <= k // 64:
                assert torch.equal(rr.fp32_model(x, wh, wl, scale, waves, splits), want32), (m, n, k, waves, splits)
                assert torch.equal(rr.fp32_model(x, wh, wl, scale, waves, splits, fp32_out=False), want16)
        assert torch.equal(x.float() @ wh.float().t() + (x.float() @ wl.float().t()) * scale, want32)
    with pytest.raises(AssertionError):
        rr.exact_inputs(4, 64, 16384, 1 / 256)  # 16384 * 2 * (2 + 8 / 256) * 256 >= 2^24: the helper refuses what could round
    with pytest.raises(AssertionError):
        rr.exact_inputs(4, 64, 64, 3 / 256)  # no power of two


def test_every_bf16_case_has_its_share_of_ties():
    """At least 1 % of the outputs of every bf16 case are exact bf16 ties (a truncating or round-half-up cast fails on them), and
    the ties round both ways.  Prints the smallest share per k."""
    least = {}
    for m, n, k, _, fp32_out in SKINNY_CASES + TILE_CASES:
        if not fp32_out:
            _, _, _, want32, want16, share = rr.exact_case(m, n, k)
            assert share >= rr.MIN_TIE_SHARE and share == float(rr.is_bf16_tie(want32).float().mean()), (m, n, k, share)
            least[k] = min(least.get(k, 1.0), share)
    for m, n, k, _, scale in SCALE_CASES:
        assert rr.exact_case(m, n, k, scale)[5] >= rr.MIN_TIE_SHARE
    print("smallest bf16 tie share per k:", {k: round(v, 4) for k, v in sorted(least.items())})
    assert len(least) >= 6
    _, _, _, want32, want16, _ = rr.exact_case(64, 192, 576)
    tie = rr.is_bf16_tie(want32)
    up = (want16.float().abs() > want32.abs())[tie]
    assert bool(up.any()) and bool((~up).any())


# ---- CPU: the slack of the bar for general inputs ----------------------------------------------------------------------------------
def test_fp32_model_passes_and_its_excess_holds_the_slack(lib):
    """RGEMM_SLACK is 4 x the worst excess of the float32 model over the float64 statement, rounded up to a power of two, on the
    real-input cases with every (accumulators, splits) they reach: the caller's counts and the library's own."""
    worst32 = worst16 = 0.0
    for m, n, k, caller in REAL_CASES:
        x, wh, wl, r, a = rr.real_inputs(m, n, k)
        for splits in sorted(set(caller) | {plan(lib, m, n, k)[0]}):
            y = rr.fp32_model(x, wh, wl, rr.REAL_SCALE, waves_of(m), splits)
            e32, e16 = float(rr.excess(y, r, a).max()), float(rr.excess(y.bfloat16(), r, a).max())
            print(f"fp32 model ({m}, {n}, {k}) x {waves_of(m)} accumulators, {splits} splits: excess {e32:.3f} x 2^-24 A (fp32), "
                  f"{e16:.3f} beyond half an ulp (bf16)")
            worst32, worst16 = max(worst32, e32), max(worst16, e16)
            assert rr.close(y, r, a, "model") and rr.close(y.bfloat16(), r, a, "model")
    print(f"worst excess of the fp32 model: {worst32:.3f} (fp32 output), {worst16:.3f} (bf16 output)")
    assert worst32 >= worst16 > 0
    assert rr.RGEMM_SLACK == 2.0 ** math.ceil(math.log2(4 * worst32)) and rr.RGEMM_SLACK <= rr.RGEMM_SLACK_CAP


# ---- CPU: planted errors -----------------------------------------------------------------------------------------------------------
def test_planted_errors_are_rejected():
    """Every planted error fails every bar that can see it: bit equality on exact inputs (fp32 and bf16 output) and the derived bar
    on real inputs (both), at k = 512 and 4096.  A cleared last mantissa bit of w_low is invisible on small integers and, at
    7-28 x 2^-24 A, far inside a bf16 output's half ulp: the fp32 real-input bar is the one that sees it.  The truncating cast
    is invisible on an fp32 output.  Everything else is seen by all four."""
    scale = 1 / 256
    for m, n, k in ((17, 64, 512), (33, 64, 4096)):
        ex, ewh, ewl = rr.exact_inputs(m, n, k, scale)
        e32 = rr.ref64(ex, ewh, ewl, scale)[0].float()
        x, wh, wl, r, a = rr.real_inputs(m, n, k)
        assert rr.close(r.float(), r, a, "statement") and rr.close(r.float().bfloat16(), r, a, "statement")
        for kind in rr.PLANTED:
            bad = rr.planted(kind, x, wh, wl, scale).float()
            units = float(rr.excess(bad, r, a).max())
            print(f"k {k} planted '{kind}': worst excess {units:.1f} x 2^-24 A")
            assert not rr.close(bad, r, a, kind), (kind, k)
            bad_exact = rr.planted(kind, ex, ewh, ewl, scale).float()
            if kind == "low plane's last mantissa bit cleared":
                assert torch.equal(bad_exact, e32)
            else:
                assert not rr.close(bad.bfloat16(), r, a, kind), (kind, k)
                assert not torch.equal(bad_exact, e32) and not torch.equal(bad_exact.bfloat16(), e32.bfloat16()), (kind, k)
        # the truncating cast: through the ties (and every other output that rounds up) on exact inputs; on real inputs it is
        # off by up to a whole ulp
        assert not torch.equal(rr.bf16_truncated(e32), e32.bfloat16())
        assert bool((rr.bf16_truncated(e32) != e32.bfloat16())[rr.is_bf16_tie(e32)].any())
        assert not rr.close(rr.bf16_truncated(r.float()), r, a, "truncating cast")


# ---- CPU: what the samples cover ---------------------------------------------------------------------------------------------------
def test_skinny_cases_cover_every_mechanism():
    """The sample holds both sides of every token-tile edge (16 | 17, 32 | 33, 64 | 65, the full 256) in split calls, a split
    whose workgroup has fewer 64-k steps than waves, an uneven cut, 16 splits, one split, and both output types on each."""
    cases = SKINNY_CASES
    assert len(set(cases)) == 60 and all(c[3] <= min(16, c[2] // 64) and c[0] <= 256 for c in cases)
    for m in (16, 17, 32, 33, 64, 65, 256):
        assert any(c[0] == m and c[3] > 1 for c in cases), m
    assert {c[0] for c in cases} >= {1, 15, 200} and {c[1] for c in cases} == {64, 192}
    assert {c[2] for c in cases} == {64, 192, 448, 576, 1024, 2112}
    for fp32_out in (True, False):
        mine = [c for c in cases if c[4] == fp32_out]
        assert any(c[3] == 1 for c in mine) and any(c[3] == 16 for c in mine)
        assert any(c[3] > 1 and min(cut(c[2] // 64, c[3])) < 4 for c in mine)  # a wave without a step
        assert any(c[3] > 1 and len(set(cut(c[2] // 64, c[3]))) > 1 for c in mine)  # an uneven cut
    assert {c[3] for c in cases} == {1, 2, 3, 5, 7, 16}


def test_tile_cases_cover_every_reduce_form():
    """Above 256 tokens: every last-tile size (1, 44, 128 and 1 row), the reduce forms of 4, 8 and 16 planes on both sides of
    4 | 5 and 8 | 9 and at 16, an odd and a single step count per split (the two-stage pipeline's tail), an uneven cut, both
    output types."""
    cases = TILE_CASES
    assert len(set(cases)) == 48 and all(c[3] <= min(16, c[2] // 64) and c[0] > 256 for c in cases)
    assert {c[0] for c in cases} == {257, 300, 384, 385} and {c[1] for c in cases} == {64, 128}
    for fp32_out in (True, False):
        mine = [c for c in cases if c[4] == fp32_out]
        assert {c[3] for c in mine} >= {1, 2, 4, 5, 8, 9, 16}, fp32_out
        steps = [n for c in mine for n in cut(c[2] // 64, c[3])]
        assert 1 in steps and any(n > 1 and n % 2 for n in steps) and any(n > 1 and n % 2 == 0 for n in steps)
        assert any(len(set(cut(c[2] // 64, c[3]))) > 1 for c in mine)
    for m in (257, 300, 384, 385):
        assert any(c[0] == m and c[3] > 8 for c in cases) and any(c[0] == m and 1 < c[3] <= 4 for c in cases), m


def test_caller_split_counts_beyond_the_bound_are_refused(lib):
    """The launcher takes 1 .. min(16, k / 64) and refuses the rest before anything is launched (pointers never dereferenced)."""
    p = ctypes.c_void_p(4096)

    def call(m, n, k, splits, planes=p, flags=p, ld=None):
        return lib.hpc_gemm_bf16xfp32_async(p, planes, flags, p, p, p, m, n, k, 1 / 256, 1, splits, n // 16 if ld is None else ld, None)

    assert call(8, 64, 192, 4) == -2 and call(8, 64, 4096, 17) == -2 and call(300, 64, 320, 6) == -2
    assert call(8, 64, 192, 0) == -2
    assert call(8, 64, 192, 2, planes=None) == -2 and call(8, 64, 192, 2, flags=None) == -2
    assert call(8, 64, 192, 2, ld=3) == -2  # counter rows shorter than the grid
    assert call(8, 96, 192, 1) == -1 and call(8, 64, 96, 1) == -1
    assert call(0, 64, 192, 1) == 0  # nothing to do, nothing launched
    # ... and nothing read: an empty batch's x and y have no storage, their pointers are null
    assert lib.hpc_gemm_bf16xfp32_async(None, None, None, None, p, p, 0, 64, 192, 1 / 256, 1, 1, 4, None) == 0
    assert lib.hpc_gemm_bf16xfp32_async(None, None, None, p, p, p, 8, 64, 192, 1 / 256, 1, 1, 4, None) == -2


# ---- GPU: through the C ABI between guard bands ------------------------------------------------------------------------------------
def run_abi(lib, x, wh, wl, scale, fp32_out, splits):
    """hpc_gemm_bf16xfp32_async with the caller's split count: split_y of exactly splits * m * n * 4 bytes holding NaN patterns,
    counters of exactly the plan's rows x row stride, zeroed, each between two guard bands; the output pre-filled with NaN.
    Checks that the counters are zero again, the guards untouched, no NaN in the output (and, unsplit, split_y unread and
    unwritten) and returns the output on the CPU."""
    from hpc import _C

    (m, k), n = x.shape, wh.shape[0]
    _, rows, ld = plan(lib, m, n, k)
    dx, dh, dl = x.cuda(), wh.cuda(), wl.cuda()
    pbytes, cbytes = splits * m * n * 4, rows * ld * 4
    pbuf = torch.full((2 * GUARD + pbytes,), PATTERN, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((2 * GUARD + cbytes,), PATTERN, dtype=torch.uint8, device="cuda")
    planes, cnt = pbuf[GUARD:GUARD + pbytes].view(torch.int32), cbuf[GUARD:GUARD + cbytes].view(torch.int32)
    planes.fill_(NAN_BITS)
    cnt.zero_()
    y = torch.full((m, n), float("nan"), dtype=torch.float32 if fp32_out else torch.bfloat16, device="cuda")
    rc = lib.hpc_gemm_bf16xfp32_async(_C.ptr(y), _C.ptr(planes), _C.ptr(cnt), _C.ptr(dx), _C.ptr(dh), _C.ptr(dl), m, n, k, scale,
                                      int(fp32_out), splits, ld, _C.stream_of(dx))
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((cnt == 0).all())
    for buf, nbytes in ((pbuf, pbytes), (cbuf, cbytes)):
        assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + nbytes:] == PATTERN).all())
    assert not bool(y.isnan().any())
    if splits == 1:
        assert bool((planes == NAN_BITS).all())
    return y.cpu()


def _assert_exact(lib, m, n, k, splits, fp32_out, scale=1 / 256):
    x, wh, wl, want32, want16, _ = rr.exact_case(m, n, k, scale)
    y = run_abi(lib, x, wh, wl, scale, fp32_out, splits)
    want = want32 if fp32_out else want16
    differ = int((y != want).sum())
    assert differ == 0, f"{differ} of {y.numel()} outputs differ from the statement"


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,splits,fp32_out", SKINNY_CASES)
def test_skinny_exact_inputs_bit_for_bit(lib, m, n, k, splits, fp32_out):
    _assert_exact(lib, m, n, k, splits, fp32_out)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,splits,fp32_out", TILE_CASES)
def test_tile_exact_inputs_bit_for_bit(lib, m, n, k, splits, fp32_out):
    _assert_exact(lib, m, n, k, splits, fp32_out)


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,splits,fp32_out", TILE_CASES)
def test_development_64x64_kernel_exact_inputs_bit_for_bit(lib, m, n, k, splits, fp32_out):
    """Development key 40 = 1: the 64 x 64 kernel that loads operands straight into MFMA layout, on the tile kernel's cases.  Equal
    to the statement bit for bit, and therefore to the tile kernel."""
    from utils import dev_set

    dev_set(40, 1)
    try:
        _assert_exact(lib, m, n, k, splits, fp32_out)
    finally:
        dev_set(40, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("fp32_out", [True, False])
@pytest.mark.parametrize("m,n,k,splits,scale", SCALE_CASES)
def test_scales_other_than_1_256(lib, m, n, k, splits, scale, fp32_out):
    """1 / 128, 1 / 512 and 1.0: a kernel with 1 / 256 written into it passes everything else."""
    _assert_exact(lib, m, n, k, splits, fp32_out, scale)


# ---- GPU: the torch op on exact inputs ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(33, 192, 1024), (300, 128, 1024)])
@pytest.mark.parametrize("use_splitk", [True, False])
@pytest.mark.parametrize("use_split_flag", [True, False])
def test_torch_op_on_exact_inputs(lib, m, n, k, use_splitk, use_split_flag):
    import hpc

    assert plan(lib, m, n, k, 1)[0] > 1 and plan(lib, m, n, k, 0)[0] == 1  # use_splitk decides something at these shapes
    x, wh, wl, want32, want16, _ = rr.exact_case(m, n, k)
    flag = hpc.get_gemm_bf16xfp32_workspace(n, 4096) if use_split_flag else None
    for fp32_out, want in ((True, want32), (False, want16)):
        y = hpc.gemm_bf16xfp32(x.cuda(), wh.cuda(), wl.cuda(), 1 / 256, fp32_out, use_splitk, flag)
        assert y.dtype == want.dtype and torch.equal(y.cpu(), want)
        if flag is not None:
            assert bool((flag == 0).all())


@pytest.mark.gpu
def test_torch_op_refuses_strided_inputs_and_returns_an_empty_batch():
    import hpc

    x, wh, wl, want32, _, _ = rr.exact_case(17, 64, 192)
    dx, dh, dl = x.cuda(), wh.cuda(), wl.cuda()
    wide = torch.zeros(17, 384, dtype=torch.bfloat16, device="cuda")
    wide[:, :192] = dx
    with pytest.raises(RuntimeError, match="contiguous"):
        hpc.gemm_bf16xfp32(wide[:, :192], dh, dl, 1 / 256, True)
    with pytest.raises(RuntimeError, match="contiguous"):
        hpc.gemm_bf16xfp32(dx, dh.t().contiguous().t(), dl, 1 / 256, True)
    assert torch.equal(hpc.gemm_bf16xfp32(wide[:, :192].contiguous(), dh, dl, 1 / 256, True).cpu(), want32)
    for fp32_out in (True, False):
        y = hpc.gemm_bf16xfp32(dx[:0], dh, dl, 1 / 256, fp32_out)
        assert tuple(y.shape) == (0, 64) and y.dtype == (torch.float32 if fp32_out else torch.bfloat16)


# ---- GPU: real inputs at the derived bar -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fp32_out", [True, False])
@pytest.mark.parametrize("m,n,k,caller", REAL_CASES)
def test_real_inputs_at_the_derived_bar(lib, m, n, k, caller, fp32_out):
    """|y - r| <= half_ulp_out(r) + RGEMM_SLACK * 2^-24 * A per element (the half ulp for bf16 output only), with the caller's split
    counts through the C ABI and the library's own through the op.  Prints the worst excess in units of the slack per case.

    On the MI355X, fp32 output, in units of 2^-24 A: the skinny kernels 0.36 / 0.38 / 0.42 unsplit, 0.17 / 0.23 / 0.19 with 3
    splits, 0.21 / 0.33 / 0.18 with 16; the tile kernel 1.36 unsplit, 0.50 with 5 splits, 0.34 with the library's 8, 0.26 with
    16 - a third of the slack at the most, so the 32-term sum inside v_mfma_f32_16x16x32_bf16 is of fp32 grade (the fp8
    instruction's is not: tests/test_linear_fp8.py).  bf16 output: 0.13 beyond the half ulp at the most."""
    import hpc

    x, wh, wl, r, a = rr.real_inputs(m, n, k)
    ok = True
    for splits in caller:
        y = run_abi(lib, x, wh, wl, rr.REAL_SCALE, fp32_out, splits)
        ok &= rr.close(y, r, a, f"({m}, {n}, {k}) {splits} splits")
    y = hpc.gemm_bf16xfp32(x.cuda(), wh.cuda(), wl.cuda(), rr.REAL_SCALE, fp32_out, True, None).cpu()
    ok &= rr.close(y, r, a, f"({m}, {n}, {k}) the library's {plan(lib, m, n, k)[0]} splits")
    assert ok


# ---- GPU: routing end to end on exact logits ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m,experts,k,scale", ROUTING_CASES)
def test_routing_on_exact_logits_with_ties(m, experts, k, scale):
    """gemm_bf16xfp32 -> topk_router on exact inputs at small k, where integer sums give exact ties between experts - with a
    power-of-two scale large enough that the low plane's sums tie together with the high plane's.  The ids must be those of
    the oracle applied to the CPU statement's logits, not the device's: one logit off by a bit on a tied pair moves an id.  At
    least one row ties exactly across the cut between its 8th and 9th logit."""
    import hpc
    from oracle import router as orouter

    x, wh, wl, want32, _, _ = rr.exact_case(m, experts, k, scale)
    ranked = torch.sort(want32, dim=-1, descending=True).values
    cut_ties = int((ranked[:, TOPK - 1] == ranked[:, TOPK]).sum())
    print(f"({m}, {experts}, {k}): {cut_ties} rows tie across the cut, "
          f"{int((ranked[:, 1:] == ranked[:, :-1]).any(-1).sum())} rows hold a tie")
    assert cut_ties >= 1
    logits = hpc.gemm_bf16xfp32(x.cuda(), wh.cuda(), wl.cuda(), scale, True)
    assert torch.equal(logits.cpu(), want32)
    ids, _ = hpc.topk_router(logits, TOPK, True)
    rid, _ = orouter.ref_topk_router(want32, TOPK, True)
    assert torch.equal(ids.cpu(), rid)
