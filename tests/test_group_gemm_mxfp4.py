"""hpc.group_gemm_mxfp4 - the grouped GEMM on MXFP4 weights and e4m3 activations (csrc/group_gemm_mxfp4.hip) - against its
statement tests/mxfp4_ref.py.

* Exact inputs (x integers -3 ... 3, any e2m1 code, e8m0 scales 2^-3 ... 2^1): a 128-block sum is a multiple of 2^-4 below 2^13.
  With xs = 2^-3 ... 2^1 every running sum is exact in fp32 (asserted block by block), so the output equals bf16_rne of the exact
  sum BIT FOR BIT; at least 1 % of every case's outputs are bf16 ties (asserted).  With xs = rand + 0.5 the output equals the bf16
  rounding of the fp32 chain tot = fmaf(P, xs, tot), emulated in float64; no FMA of the committed inputs is undecided (asserted).
* Real inputs (normal data through the 128-block e4m3 quantiser, normal weights through the MXFP4 quantiser):
  |y - statement| <= half a bf16 ulp + C_BAR * 2^-24 * A, A the statement with absolute values everywhere.  C_BAR is twice the
  worst err / (2^-24 A) measured on the MI355X against the float64 statement, rounded up to a power of two - the rule of
  tests/test_mla_indexer.py.
* CPU: the statement against a brute-force loop; every code, both nibbles, scale bytes 0 and 254; the route through the plan
  entry; the fakes; planted errors against the bars.
"""
import ctypes
import functools
import types

import pytest
import torch

import mxfp4_ref as mr
import quant_ref as qr
from utils import ulp_bf16

F8 = torch.float8_e4m3fn
KINDS = ("pow2", "general")
GUARD_ROWS, SENTINEL, SPARE = 32, -7.0, 5
# measured on the MI355X over REAL_CASES: worst (|y - statement| - half a bf16 ulp) / (2^-24 A) = 12.89, 13.54, 15.35, 4.074 (in the
# cases' order); C_BAR = twice the worst, rounded up to a power of two
MEASURED_C = 15.35
C_BAR = 32

L8 = (0, 1, 15, 16, 17, 33, 48, 49)  # 22 rows per group: 32 tokens per pass, two passes for 33 / 48 / 49
L3 = (3, 0, 5)                       # 2 rows per group: 16 tokens per pass
LP = (33, 0, 1, 0)                   # 8 rows per group: 16 tokens per pass, three passes for the group of 33
G1 = (49,)                           # one group (a dense layer): 48 tokens per pass, two passes
# (seqlens, n, k, through a row_index).  k / 128 = 1, 2, 3, 11: one k-block, an odd count, and 6 stages of two; 19 (k = 2432): 10 stages -
# more than the 8 (6 at 48 tokens per pass) a wave keeps in flight, so its prefetch slots are refilled
CASES = [(L8, 64, 128, False), (L8, 192, 384, True), (L8, 256, 1408, False), (L3, 64, 256, True), (L3, 192, 1408, False),
         (G1, 256, 256, False), (G1, 64, 1408, True), (LP, 64, 384, False), (L3, 64, 2432, False), (G1, 64, 2432, True),
         (L8, 64, 2432, True), (G1, 192, 128, True)]
TOKENS_PER_PASS = {L8: 32, L3: 16, LP: 16, G1: 48}


def _id(case):
    seqlens, n, k, ri = case
    return f"{'x'.join(map(str, seqlens))}-n{n}-k{k}" + ("-row_index" if ri else "")


@functools.lru_cache(maxsize=4)
def _case(seqlens, n, k, row_index):
    """inputs and both kinds' expected outputs of one case, computed once and never written; asserts the generator's conditions"""
    total = sum(seqlens)
    spare = SPARE if row_index else 0
    inp = mr.exact_inputs(seqlens, n, k, seed=total * 37 + n + k + spare, spare_rows=spare)
    rows = torch.randperm(total + spare, generator=torch.Generator().manual_seed(k + 1))[:total] if row_index else torch.arange(total)
    sl, cu = mr.cu_of(seqlens)
    c = types.SimpleNamespace(inp=inp, rows=rows.to(torch.int32), sl=sl, cu=cu, n=n, k=k, total=total, G=len(seqlens), kinds={},
                              row_index=row_index, seqlens=seqlens)
    for kind in KINDS:
        exact, big_a, parts = mr.gemm_ref(inp.x, inp.xs[kind], inp.w, inp.s, seqlens, cu, rows=rows)
        assert float(parts.abs().max()) < 2.0 ** 13 and bool((parts * 16 == (parts * 16).round()).all())
        tot, flagged, inexact = mr.chain(parts, inp.xs[kind][rows])
        assert flagged == 0, f"{flagged} FMAs of the float64 emulation are undecided: pick another seed"
        if kind == "pow2":
            assert inexact == 0 and torch.equal(tot, exact), "a running sum is not exact in fp32: k is too large for these inputs"
            want = qr.bf16_rne64(exact)
            assert torch.equal(want, tot.float().bfloat16())
            assert qr.bf16_tie_share(exact) >= 0.01, qr.bf16_tie_share(exact)
        else:
            want = tot.float().bfloat16()
        c.kinds[kind] = types.SimpleNamespace(want=want, exact=exact, big_a=big_a, parts=parts)
    return c


def _equal(c, run, label):
    """run(kind) -> bf16 [total, n] on the CPU.  -> the kinds whose outputs are not all the statement's, bit for bit"""
    missed = []
    for kind in KINDS:
        s, got = c.kinds[kind], run(kind)
        assert got.dtype == torch.bfloat16 and got.shape == s.want.shape, (got.dtype, got.shape)
        same = got.view(torch.int16) == s.want.view(torch.int16)
        print(f"{label} {kind}: {int((~same).sum())}/{same.numel()} outputs differ from the statement; "
              f"{qr.bf16_tie_share(s.exact):.2%} of the exact sums are bf16 ties")
        if not bool(same.all()):
            for r, col in torch.nonzero(~same)[:8].tolist():
                print(f"  ({r}, {col}): got {float(got[r, col]):.9g} want {float(s.want[r, col]):.9g} float64 sum {float(s.exact[r, col]):.12g}")
            missed.append(kind)
    return missed


# ---------------------------------------------------------------------------------------------------------------------- CPU
def test_statement_against_a_brute_force_loop():
    seqlens = (2, 0, 1)
    inp = mr.exact_inputs(seqlens, 3, 256, seed=1)
    sl, cu = mr.cu_of(seqlens)
    got, big_a, _ = mr.gemm_ref(inp.x, inp.xs["general"], inp.w, inp.s, seqlens, cu)
    want = mr.gemm_brute(inp.x, inp.xs["general"], inp.w, inp.s, seqlens, cu)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13) and bool((big_a >= got.abs()).all())
    real = mr.real_inputs(seqlens, 3, 128, seed=2)
    got = mr.gemm_ref(real.x, real.xs, real.w, real.s, seqlens, cu)[0]
    assert torch.allclose(got, mr.gemm_brute(real.x, real.xs, real.w, real.s, seqlens, cu), rtol=1e-12, atol=1e-13)


def test_formats():
    """all 16 codes in both nibbles, the nibble order, scale bytes 0 and 254, and the quantiser's round trip"""
    codes = torch.arange(16, dtype=torch.uint8)
    table = [0, .5, 1, 1.5, 2, 3, 4, 6, -0.0, -.5, -1, -1.5, -2, -3, -4, -6]
    for other in (0, 5):
        lo = mr.unpack_e2m1(codes | (other << 4)).view(16, 2)
        hi = mr.unpack_e2m1((codes << 4) | other).view(16, 2)
        assert lo[:, 0].tolist() == table and hi[:, 1].tolist() == table  # even k: low nibble
        assert bool((lo[:, 1] == table[other]).all()) and bool((hi[:, 0] == table[other]).all())
    assert torch.signbit(mr.unpack_e2m1(torch.tensor([8], dtype=torch.uint8)))[0]
    k = torch.arange(64) % 16
    assert torch.equal(mr.unpack_e2m1(mr.pack_e2m1(k.to(torch.uint8))), mr.E2M1[k])
    sc = mr.e8m0(torch.tensor([0, 126, 127, 128, 254, 255], dtype=torch.uint8))
    assert sc[:5].tolist() == [2.0 ** -127, 0.5, 1.0, 2.0, 2.0 ** 127] and bool(sc[5].isnan())
    # dequant at the extreme scale bytes: 6 * 2^127 and 0.5 * 2^-127 are float64 values, nothing overflows
    w = mr.pack_e2m1(torch.tensor([[7, 1] * 32], dtype=torch.uint8))
    s = torch.tensor([[254, 0]], dtype=torch.uint8)
    d = mr.dequant(w, s)
    assert d[0, 0] == 6 * 2.0 ** 127 and d[0, 33] == 0.5 * 2.0 ** -127
    g = torch.Generator().manual_seed(3)
    wf = torch.randn(4, 5, 256, generator=g)
    wq, sq = mr.quantise_mxfp4(wf)
    back = mr.dequant(wq, sq)
    amax = wf.double().view(4, 5, 8, 32).abs().amax(-1).repeat_interleave(32, dim=-1)
    assert wq.shape == (4, 5, 128) and sq.shape == (4, 5, 8)
    # 2^e <= amax / 4; rounding errs by half the largest step (2) at most, saturation at 6 (values up to 8 * 2^e) by 2
    assert bool(((back - wf.double()).abs() <= amax / 2).all())
    exact = mr.E2M1[torch.randint(0, 16, (2, 64), generator=g)] * 0.25  # representable: comes back as it is
    assert torch.equal(mr.dequant(*mr.quantise_mxfp4(exact)), exact)


def _plan(num_group, m, x_rows, n, k):
    from hpc import _C

    tok, gx, gy = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _C.lib.hpc_group_gemm_mxfp4_plan(num_group, m, x_rows, n, k, ctypes.byref(tok), ctypes.byref(gx), ctypes.byref(gy))
    return rc, tok.value, gx.value, gy.value


def test_route_through_the_plan_entry():
    G = 8
    for avg, tokens in ((1, 16), (10, 16), (11, 32), (22, 32), (23, 48), (200, 48)):
        assert _plan(G, avg * G, avg * G, 256, 384) == (0, tokens, 4, G), avg
        assert _plan(G, avg * G + G - 1, 7, 64, 128) == (0, tokens, 1, G), avg  # the average is m / num_group, rounded down
    assert _plan(1, 49, 49, 11008, 4096) == (0, 48, 172, 1)
    assert _plan(3, 0, 0, 64, 128) == (0, 0, 0, 0)  # nothing to launch
    for seqlens, tokens in TOKENS_PER_PASS.items():
        assert _plan(len(seqlens), sum(seqlens), sum(seqlens), 64, 128)[1] == tokens
    unsupported, invalid = -1, -2
    assert _plan(2, 4, 4, 64, 192)[0] == unsupported       # k % 128
    assert _plan(2, 4, 4, 96, 128)[0] == unsupported       # n % 64
    assert _plan(2, 4, 4, 1 << 20, 1 << 13)[0] == unsupported  # n * k / 2 = 2^32: beyond one buffer descriptor
    assert _plan(2, 4, 1 << 19, 64, 1 << 13)[0] == unsupported  # x_rows * k = 2^32
    assert _plan(65536, 4, 4, 64, 128)[0] == unsupported
    assert _plan(2, 4, 4, 524224, 1 << 14)[0] == 0           # n * k / 2 = 2^32 - 2^19: inside
    for bad in ((0, 4, 4, 64, 128), (2, -1, 4, 64, 128), (2, 4, -1, 64, 128), (2, 4, 4, 0, 128), (2, 4, 4, 64, 0)):
        assert _plan(*bad)[0] == invalid, bad
    from hpc import _C

    assert _C.lib.hpc_group_gemm_mxfp4_plan(2, 4, 4, 64, 128, None, None, None) == 0


def test_async_refuses_on_the_host():
    """null pointers, x_rows < m without a row_index, misaligned pointers: refused before any device call (no GPU here)"""
    from hpc import _C

    fn, p, odd = _C.lib.hpc_group_gemm_mxfp4_async, ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    ok = [p, p, p, p, p, p, p, None, 2, 4, 4, 64, 128, None]
    for i in range(7):
        args = list(ok)
        args[i] = None
        assert fn(*args) == -2, i
    for i in range(5):
        args = list(ok)
        args[i] = odd
        assert fn(*args) == -1, i
    args = list(ok)
    args[10] = 3
    assert fn(*args) == -2            # row r reads row r of x: x_rows >= m
    args[7] = p
    args[9] = 0
    assert fn(*args) == 0             # m == 0: nothing to launch
    args = list(ok)
    args[12] = 192
    assert fn(*args) == -1


def test_surface_and_fakes():
    from torch._subclasses import FakeTensorMode

    import hpc

    for name in ("group_gemm_mxfp4", "fuse_moe_mxfp4"):
        assert name in hpc.__all__ and callable(getattr(hpc, name)), name
    ops = torch.ops.hpc_mxfp4
    assert str(ops.group_gemm.default._schema) == (
        "hpc_mxfp4::group_gemm(Tensor x, Tensor x_scale, Tensor weight, Tensor weight_scale, Tensor seqlens, Tensor cu_seqlens, "
        "Tensor? row_index, Tensor? output) -> Tensor")
    assert str(ops.fuse_moe.default._schema) == (
        "hpc_mxfp4::fuse_moe(Tensor x, Tensor x_scale, Tensor gate_up_weight, Tensor gate_up_weight_scale, Tensor down_weight, "
        "Tensor down_weight_scale, Tensor topk_ids, Tensor topk_scale, Tensor? shared_output, int rank_ep, int num_expert_total, "
        "Tensor? output) -> Tensor")
    U8, I32, F32 = torch.uint8, torch.int32, torch.float32
    with FakeTensorMode():
        def T(*shape, dtype):
            return torch.empty(shape, dtype=dtype, device="cuda")

        G, N, K, M = 3, 192, 256, 11
        x, xs, w, s = T(M, K, dtype=F8), T(M, K // 128, dtype=F32), T(G, N, K // 2, dtype=U8), T(G, N, K // 32, dtype=U8)
        sl, cu = T(G, dtype=I32), T(G + 1, dtype=I32)
        y = ops.group_gemm(x, xs, w, s, sl, cu, None, None)
        assert (tuple(y.shape), y.dtype) == ((M, N), torch.bfloat16)
        y = ops.group_gemm(x, xs, w, s, sl, cu, T(20, dtype=I32), None)
        assert (tuple(y.shape), y.dtype) == ((20, N), torch.bfloat16)
        y = hpc.group_gemm_mxfp4(x, xs, w.view(torch.float4_e2m1fn_x2), s.view(torch.float8_e8m0fnu), sl, cu)
        assert (tuple(y.shape), y.dtype) == ((M, N), torch.bfloat16)
        E, H, I, k = 4, 256, 128, 2
        y = hpc.fuse_moe_mxfp4(T(M, H, dtype=F8), T(M, H // 128, dtype=F32), T(E, 2 * I, H // 2, dtype=U8), T(E, 2 * I, H // 32, dtype=U8),
                               T(E, H, I // 2, dtype=U8), T(E, H, I // 32, dtype=U8), T(M, k, dtype=I32), T(M, k, dtype=F32), 0, E)
        assert (tuple(y.shape), y.dtype) == ((M, H), torch.bfloat16)


MUTANTS = {"nibbles swapped": dict(swapped=True), "scale bias 126": dict(bias=126), "one scale per 16 values": dict(per=16),
           "one scale per 128 values": dict(per=128), "the scale of the neighbouring row": dict(roll_rows=1)}
XS_MUTANT = "xs of the neighbouring row"
CHAIN_MUTANTS = {"k-blocks in descending order": dict(order="descending"), "a rounded product plus a separate add": dict(form="round_product")}
MUTANT_CASE = (L8, 64, 1408, False)
# CPU only: an fp32 rounding moves a bf16 rounding once in some 2^15 outputs, so the chain's mutants need a few hundred thousand
CHAIN_MUTANT_CASE = ((300, 212), 512, 1408, False)


def _model(c, kind, mutant=None):
    """the CPU model of the kernel, with one planted error"""
    inp, xs, form, order = c.inp, c.inp.xs[kind][c.rows.long()], "fma", None
    planted = MUTANTS.get(mutant, {})
    if mutant == XS_MUTANT:
        xs = xs.roll(1, 0)
    if mutant in CHAIN_MUTANTS:
        form = CHAIN_MUTANTS[mutant].get("form", "fma")
        order = range(c.k // 128 - 1, -1, -1) if "order" in CHAIN_MUTANTS[mutant] else None
    parts = mr.gemm_ref(inp.x, inp.xs[kind], inp.w, inp.s, c.seqlens, c.cu, rows=c.rows, **planted)[2]
    return mr.chain(parts.float().double(), xs, form, order)[0].float().bfloat16()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_generator_conditions(case):
    c = _case(*case)  # the assertions are inside
    print(f"{_id(case)}: {qr.bf16_tie_share(c.kinds['pow2'].exact):.2%} ties")


def test_model_meets_both_bars():
    c = _case(*MUTANT_CASE)
    assert _equal(c, lambda kind: _model(c, kind), "model") == []


@pytest.mark.parametrize("mutant", sorted(MUTANTS) + [XS_MUTANT])
def test_equality_bars_reject_mutant(mutant):
    c = _case(*MUTANT_CASE)
    assert _equal(c, lambda kind: _model(c, kind, mutant), mutant) == ["pow2", "general"]


@pytest.mark.parametrize("mutant", sorted(CHAIN_MUTANTS))
def test_general_bar_rejects_another_arithmetic(mutant):
    """another order or another rounding of the same sum is exact on power-of-two scales (that bar cannot see it, by design);
    with general scales at least one output differs"""
    c = _case(*CHAIN_MUTANT_CASE)
    assert torch.equal(_model(c, "pow2", mutant).view(torch.int16), c.kinds["pow2"].want.view(torch.int16))
    differ = int((_model(c, "general", mutant).view(torch.int16) != c.kinds["general"].want.view(torch.int16)).sum())
    print(f"{mutant}: {differ} outputs differ")
    assert differ >= 1


REAL_CASES = [(L8, 192, 1408), (L3, 64, 128), (G1, 256, 384), (LP, 64, 2432)]


@functools.lru_cache(maxsize=None)
def _real(seqlens, n, k):
    inp = mr.real_inputs(seqlens, n, k, seed=sum(seqlens) + n + k)
    sl, cu = mr.cu_of(seqlens)
    y64, big_a, _ = mr.gemm_ref(inp.x, inp.xs, inp.w, inp.s, seqlens, cu)
    return inp, sl, cu, y64, big_a


def _over_real_bar(got64, y64, big_a, c_bar=C_BAR):
    """-> (outputs beyond the bar, the worst (err - half an ulp) / (2^-24 A))"""
    err = (got64 - y64).abs() - 0.5 * ulp_bf16(y64)
    unit = (2.0 ** -24 * big_a).clamp_min(1e-300)
    return int((err > c_bar * unit).sum()), float((err / unit).max())


@pytest.mark.parametrize("mutant", sorted(MUTANTS) + [XS_MUTANT])
def test_real_input_bar_rejects_mutant(mutant):
    """every planted error of the formats and of the addressing is beyond the real-input bar; the statement itself, rounded
    to bf16, is within it with C = 0"""
    seqlens, n, k = REAL_CASES[0]
    inp, sl, cu, y64, big_a = _real(seqlens, n, k)
    assert _over_real_bar(qr.bf16_rne64(y64).double(), y64, big_a, 0)[0] == 0
    xs = inp.xs.roll(1, 0) if mutant == XS_MUTANT else inp.xs
    bad = mr.gemm_ref(inp.x, xs, inp.w, inp.s, seqlens, cu, **MUTANTS.get(mutant, {}))[0]
    over, worst = _over_real_bar(qr.bf16_rne64(bad).double(), y64, big_a)
    print(f"{mutant}: {over}/{y64.numel()} outputs beyond the bar, worst {worst:.3g} x 2^-24 A")
    assert over >= 1


# ---------------------------------------------------------------------------------------------------------------------- GPU
def _guarded(total, n):
    buf = torch.full((total + 2 * GUARD_ROWS, n), SENTINEL, dtype=torch.bfloat16, device="cuda")
    return buf, buf[GUARD_ROWS : GUARD_ROWS + total]


def _run(c, kind, with_output=True):
    import hpc

    inp = c.inp
    xd, xsd, wd, sd, sld, cud = (t.cuda() for t in (inp.x, inp.xs[kind].contiguous(), inp.w, inp.s, c.sl, c.cu))
    buf, out = _guarded(c.total, c.n) if with_output else (None, None)
    if c.row_index:
        y = torch.ops.hpc_mxfp4.group_gemm(xd, xsd, wd, sd, sld, cud, c.rows.cuda(), out)
    else:
        y = hpc.group_gemm_mxfp4(xd, xsd, wd.view(torch.float4_e2m1fn_x2), sd.view(torch.float8_e8m0fnu), sld, cud, output=out)
    torch.cuda.synchronize()
    if with_output:
        assert y.data_ptr() == out.data_ptr()
        b = buf.cpu()
        assert bool((b[:GUARD_ROWS] == SENTINEL).all()) and bool((b[GUARD_ROWS + c.total :] == SENTINEL).all()), "guard rows were written"
    return y.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_group_gemm_mxfp4_exact(case):
    c = _case(*case)
    assert _equal(c, lambda kind: _run(c, kind), _id(case)) == []


@pytest.mark.gpu
def test_group_gemm_mxfp4_exact_fresh_output():
    c = _case(*CASES[0])
    assert _equal(c, lambda kind: _run(c, kind, with_output=False), _id(CASES[0]) + " (no output=)") == []
    # empty call: m == 0 returns at once
    import hpc

    z = lambda *s, dtype: torch.zeros(s, dtype=dtype, device="cuda")  # noqa: E731
    y = hpc.group_gemm_mxfp4(z(0, 128, dtype=torch.uint8).view(F8), z(0, 1, dtype=torch.float32), z(2, 64, 64, dtype=torch.uint8),
                             z(2, 64, 4, dtype=torch.uint8), z(2, dtype=torch.int32), z(3, dtype=torch.int32))
    assert tuple(y.shape) == (0, 64)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        hpc.group_gemm_mxfp4(z(4, 128, dtype=torch.uint8).view(F8), z(4, 1, dtype=torch.float32), z(2, 96, 64, dtype=torch.uint8),
                             z(2, 96, 4, dtype=torch.uint8), z(2, dtype=torch.int32), z(3, dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: _id(c + (False,)))
def test_group_gemm_mxfp4_real_inputs(case):
    import hpc

    seqlens, n, k = case
    inp, sl, cu, y64, big_a = _real(seqlens, n, k)
    y = hpc.group_gemm_mxfp4(inp.x.cuda(), inp.xs.cuda(), inp.w.cuda(), inp.s.cuda(), sl.cuda(), cu.cuda())
    torch.cuda.synchronize()
    over, worst = _over_real_bar(y.cpu().double(), y64, big_a)
    print(f"real inputs {_id(case + (False,))}: worst (err - half a bf16 ulp) / (2^-24 A) = {worst:.4g}; {over} outputs beyond C_BAR = {C_BAR}")
    assert over == 0
