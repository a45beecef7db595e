"""The blockwise-scaled grouped FP8 GEMM (all four kernels, all three addressing forms) and the fused MoE on top of it, on
inputs that determine the bf16 output bit for bit: x in -3 ... 3 and w in -4 ... 4 as e4m3 (tests/quant_ref.py::
gemm_exact_inputs), so a 128-block partial sum is an integer of at most 1536 - exact in fp32 in any order.  The kernels state
one arithmetic: f = xs * ws (one fp32 multiply), tot = fmaf(part, f, tot) per k-block in ascending order, one bf16
rounding.  Two scale kinds, two bars, both EQUALITY - nothing is measured, nothing excluded:

* powers of two (xs = 2^e per (row, block), ws = +-2^e per (group, n-block, k-block), e in -3 ... 1): every running sum is a
  multiple of 2^-6 below 2^18, exact in fp32 in any order (asserted block by block), so the output equals bf16(exact sum),
  rounded to nearest even, whatever a kernel does.  At least 1 % of every case's outputs sit on bf16 ties (asserted).
* general scales (xs = rand + 0.5, ws = +-(rand + 0.5)): the output equals the bf16 rounding of the fp32 chain above, which
  tests/quant_ref.py::blockwise_chain emulates in float64 (the 11 x 24-bit product is exact, TwoSum recovers the sum's
  rounding error); an FMA whose float64 sum was inexact AND an fp32 midpoint could round either way - the committed inputs
  have none (asserted per case).

Scales that belong to no valid row, column or k-block (pad4 columns of ws, tile padding of the transposed layout, pool rows no
output row reads) hold 2^20.  On the CPU thirteen planted errors are rejected (ten by both bars, three - another k-block order,
the eager model's three roundings, a rounded product and a separate add - by the general bar alone).  The fused MoE is held to
its own stages: count/slot, gate-up GEMM, activation, down GEMM and reduce called one by one through the C ABI with the
arguments csrc/fuse_moe.hip::fuse_moe passes give the fused op's output bit for bit, and the chain's gate-up matrix is the CPU
statement's.

Measured on the MI355X: outputs that differ from the statement - default routes 0 (14 + 6 + 5 cases of the three
call forms, both scale kinds), pinned kernel forms 0 (57 cases), fused MoE against its stages 0 and its gate-up matrix against
the statement 0 (6 cases); smallest share of ties 1.76 % (k = 128; 5-16 % from two k-blocks on).  All four kernels meet the
general-scale equality: none is held to the derived fallback (half a bf16 ulp + (k / 128 + 1) 2^-24 A), whose slack the outputs
use 0.39 of at the most.  No finding."""
import functools
import types

import pytest
import torch

import quant_ref as qr
from utils import EPILOGUE_SITE_ROWS, dev_set, topk1_ids_with_rows, ulp_bf16

F8 = torch.float8_e4m3fn
KINDS = ("pow2", "general")
GUARD_ROWS, PAD_ROWS, SENTINEL = 64, 256, -7.0

# ------------------------------------------------------------------------------------------------------------ cases
# group lengths; between them 0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 256, 257 and the 256 x 256 kernel's sites 265 / 296 / 456
L_AVG5 = (8, 9, 10, 0, 1, 7, 3, 5)                       # tile_m 8, streaming 16 tokens per pass
L_AVG7 = (0, 1, 15, 16, 17, 3, 5, 2)                     # tile_m 8, streaming 16 tokens per pass
L_AVG13 = (16, 17, 15, 0, 1, 33, 16, 12)                 # tile_m 16, streaming 32 tokens per pass (with the scan: still streaming)
L_AVG18 = (0, 1, 63, 17, 15, 16, 20, 12)                 # tile_m 32, streaming 32 per pass - with the scan the 256 x 256 kernel
L_AVG30 = (64, 65, 0, 1, 15, 16, 17, 63)                 # tile_m 32, tiled
L_AVG46 = (128, 129, 0, 1, 17, 63, 16, 15)               # tile_m 48
L_AVG52 = (256, 0, 1, 15, 16, 17, 63, 64, 65, 128, 1, 0)  # tile_m 64
L_AVG86 = (257, 129, 0, 1, 64, 65)                       # the 96 -> 48 rung
L_SITES = (265, 296, 456, 0, 1, 128)                     # ride-along tail, 40-row tail body, 200-row last tile; tile_m 64
L_65GROUPS = tuple((0, 1, 15, 16, 17, 63, 64, 4, 8, 33)[i % 10] for i in range(65))  # 21 rows per group on average
L_RAGGED = (300, 0, 129, 5, 128, 1, 257)                 # the lengths of the tiled kernels' tests

# form (a), hpc.group_gemm_blockwise_fp8: (seqlens, n, k); k / 128 in 1, 2, 3, 5, 11, 16 and n in 256, 384, 512 on every route
OP_CASES = [(L_AVG7, 256, 128), (L_AVG13, 384, 256), (L_AVG18, 512, 384), (L_AVG5, 256, 1408), (L_AVG13, 256, 2048),
            (L_AVG30, 256, 640), (L_AVG30, 512, 256), (L_AVG46, 384, 1408), (L_AVG30, 384, 128), (L_AVG52, 512, 2048),
            (L_AVG86, 256, 384), (L_AVG86, 512, 128), (L_SITES, 512, 640), (L_65GROUPS, 256, 256)]
# forms (b) and (c), the C entry with row-major scales: (seqlens, n, k, with the scan of ceil(seqlens / 128))
ROW_INDEX_CASES = [(L_AVG13, 256, 640, True), (L_AVG18, 512, 384, True), (L_SITES, 256, 1408, True), (L_AVG46, 384, 256, True),
                   (L_AVG30, 256, 384, False), (L_AVG46, 384, 128, False)]  # no scan, > 22 rows: streaming, 48 tokens per pass
ROW_MAJOR_CASES = [(L_AVG13, 384, 128, True), (L_AVG18, 256, 2048, True), (L_SITES, 512, 256, True), (L_AVG46, 384, 640, True),
                   (L_65GROUPS, 256, 256, True)]
PINNED_NK = [(512, 640), (256, 2048), (384, 384)]
SPARE = 7  # rows of the pool that no output row reads (form (b))
MUTANT_NK = [(512, 640), (512, 512)]  # k / 128 = 5: pad4 padding exists; 4: none


def _id(case):
    seqlens, n, k = case[:3]
    name = f"{'x'.join(map(str, seqlens)) if len(seqlens) <= 12 else f'{len(seqlens)}groups'}-n{n}-k{k}"
    return name + ("" if len(case) < 4 or case[3] else "-noscan")


@functools.lru_cache(maxsize=4)
def _case(seqlens, n, k, spare_rows=0):
    """Inputs and both bars' expected outputs of one case, computed once.  -> namespace: pool / w (e4m3), rows (the pool row
    every output row reads), sl, cu, group, parts (exact block sums) and per kind: xs_pool, xs (per output row), ws, want (bf16),
    exact and A (float64).  Asserts the generator's conditions."""
    G, total, kb = len(seqlens), sum(seqlens), k // 128
    pool, w = qr.gemm_exact_inputs(seqlens, n, k, seed=total * 37 + n + k + spare_rows, spare_rows=spare_rows)
    rows = torch.randperm(total + spare_rows, generator=torch.Generator().manual_seed(k + 1))[:total] if spare_rows else torch.arange(total)
    sl = torch.tensor(seqlens, dtype=torch.int32)
    cu = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(sl, 0).to(torch.int32)])
    group = torch.repeat_interleave(torch.arange(G), sl.long())
    x = pool.view(torch.uint8)[rows].view(F8)
    parts = qr.blockwise_block_sums(x, w, group)
    assert float(parts.abs().max()) <= 1536 and bool((parts == parts.round()).all())
    unread = torch.ones(total + spare_rows, dtype=torch.bool)
    unread[rows] = False
    c = types.SimpleNamespace(pool=pool, w=w, x=x, rows=rows.to(torch.int32), sl=sl, cu=cu, group=group, parts=parts, n=n, k=k,
                              kb=kb, total=total, G=G, kinds={})
    for kind in KINDS:
        xs_pool, ws = qr.blockwise_scales(total + spare_rows, G, n, k, seed=total + 3 * n + k, kind=kind, loud_rows=unread)
        xs = xs_pool[rows].contiguous()
        tot, flagged, exact, big_a, inexact = qr.blockwise_chain(parts, xs, ws[group][:, :, :kb])
        assert flagged == 0, f"{flagged} FMAs of the float64 emulation are undecided: pick another seed"
        if kind == "pow2":
            assert inexact == 0 and torch.equal(tot, exact) and float(big_a.max()) < 2.0 ** 18  # multiples of 2^-6: 24 bits in any order
            want = qr.bf16_rne64(exact)
            assert torch.equal(want, tot.float().bfloat16())
            ties = qr.bf16_tie_share(exact)
            assert ties >= 0.01, ties
        else:
            want = tot.float().bfloat16()
        c.kinds[kind] = types.SimpleNamespace(xs_pool=xs_pool, xs=xs, ws=ws, want=want, exact=exact, big_a=big_a)
    return c


def _fallback_slack(c, kind):
    """what a kernel with another (legitimate) order would be allowed beyond half a bf16 ulp of the float64 sum: (k / 128 + 1)
    2^-24 A.  No kernel is held to it - the figure is printed next to the equality as the distance from it."""
    return ((c.kb + 1) * 2.0 ** -24 * c.kinds[kind].big_a).clamp_min(1e-300)


def _both_bars(c, run, label):
    """run(kind) -> bf16 [total, n] on the CPU; both bars on it, every output compared.  -> list of the bars missed"""
    missed = []
    for kind in KINDS:
        s = c.kinds[kind]
        got = run(kind)
        assert got.dtype == torch.bfloat16 and got.shape == s.want.shape, (got.dtype, got.shape)
        same = got.view(torch.int16) == s.want.view(torch.int16)
        over = ((got.double() - s.exact).abs() - 0.5 * ulp_bf16(s.exact)).nan_to_num(nan=float("inf")) / _fallback_slack(c, kind)
        print(f"{label} {kind} scales: {int((~same).sum())}/{same.numel()} outputs differ from the statement; "
              f"{qr.bf16_tie_share(s.exact):.2%} of the exact sums are bf16 ties; worst excess over half an ulp = "
              f"{float(over.max()):.3g} x the fallback's slack")
        if not bool(same.all()):
            for r, col in torch.nonzero(~same)[:10].tolist():
                print(f"  ({r}, {col}) group {int(c.group[r])}: got {float(got[r, col]):.9g} want {float(s.want[r, col]):.9g} "
                      f"float64 sum {float(s.exact[r, col]):.12g}")
            missed.append(kind)
    return missed


# ------------------------------------------------------------------------------------------------------------ CPU
def _rne24(fr):
    """a Fraction -> the nearest fp32 value (ties to even), as a float; normal range"""
    from fractions import Fraction

    if fr == 0:
        return 0.0
    sign, a = (-1 if fr < 0 else 1), abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = a / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    fl = q.numerator // q.denominator
    rem = q - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    return sign * float(fl) * 2.0 ** (e - 23)


def test_fma32_is_a_single_rounding():
    """against exact rational arithmetic on random operands of the test's kind (integer x fp32 + fp32), and on constructed
    midpoints: where the float64 sum is inexact and half way, the element is flagged - and only there"""
    from fractions import Fraction

    g = torch.Generator().manual_seed(5)
    a = torch.randint(-1536, 1537, (3000,), generator=g).double()
    b = ((torch.rand(3000, generator=g) + 0.5) * (torch.rand(3000, generator=g) + 0.5)).double()
    c = (torch.randn(3000, generator=g) * 2000).float().double()
    r, flag = qr.fma32(a, b, c)
    assert int(flag.sum()) == 0
    for i in range(3000):
        assert float(r[i]) == _rne24(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))), i
    # 1 + 2^-24 is half way between 1 and 1 + 2^-23; a product of 2^-60 below float64's reach decides: a true FMA rounds up
    one = torch.tensor([1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24], dtype=torch.float64)
    pa, pb = torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64), torch.tensor([2.0 ** -60, -(2.0 ** -60), 1.0], dtype=torch.float64)
    # (c itself is no fp32 value here: the case only exercises the midpoint logic)
    r, flag = qr.fma32(pa, pb, one)
    assert flag.tolist() == [True, True, False] and float(r[2]) == 1.0  # the exact midpoint is decided: ties to even


ALL_CASES = sorted({(c[0], c[1], c[2], 0) for c in OP_CASES + ROW_MAJOR_CASES} | {(c[0], c[1], c[2], SPARE) for c in ROW_INDEX_CASES}
                   | {(L_RAGGED, n, k, s) for n, k in PINNED_NK + MUTANT_NK for s in (0, SPARE)})


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda case: _id(case[:3]) + f"-spare{case[3]}")
def test_generator_conditions(case):
    """every case: block sums are integers <= 1536; power-of-two scales: every running sum exact, >= 1 % bf16 ties; general
    scales: no undecided FMA in the float64 emulation (all asserted inside _case); the two kinds share signs, and no loud scale
    reaches an expected output"""
    c = _case(*case)
    p2, ge = c.kinds["pow2"], c.kinds["general"]
    assert torch.equal(torch.sign(p2.ws), torch.sign(ge.ws))
    assert bool((p2.ws[:, :, c.kb :] == qr.LOUD).all()) and bool((ge.xs < 2).all())
    for s in (p2, ge):
        assert float(s.big_a.max()) < 1536 * 4 * c.kb + 1 and int((s.xs_pool[:, 0] == qr.LOUD).sum()) == case[3]
    print(f"{_id(case[:3])} spare {case[3]}: {qr.bf16_tie_share(p2.exact):.2%} ties (power-of-two scales)")


STREAM16, STREAM32, STREAM48, TILED128, P8 = (1, 1), (1, 2), (1, 3), (2, 0), (4, 0)  # (kernel, streaming form) of csrc/group_gemm_route.h
OP_ROUTES = [STREAM16, STREAM32, STREAM32, STREAM16, STREAM32, P8, P8, TILED128, TILED128, P8, P8, P8, P8, P8]
ROW_INDEX_ROUTES = [STREAM32, P8, P8, TILED128, STREAM48, STREAM48]
ROW_MAJOR_ROUTES = [STREAM32, P8, P8, TILED128, P8]


def test_cases_reach_their_routes():
    """the kernel every default-key case is named for, asked of ggemm_route() through the development build (no GPU): the
    torch op has the scan of ceil(seqlens / 128) above 20 rows per group, the C entry where the case passes it"""
    import ctypes
    from pathlib import Path

    lib = ctypes.CDLL(str(Path(__file__).resolve().parent.parent / "hpc-ops_amd" / "hpc" / "libhpc_amd_dev.so"))
    lib.hpc_dev_ggemm_route.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    got = {}
    for name, cases, routes in (("op", OP_CASES, OP_ROUTES), ("row_index", ROW_INDEX_CASES, ROW_INDEX_ROUTES),
                                ("row-major", ROW_MAJOR_CASES, ROW_MAJOR_ROUTES)):
        assert len(cases) == len(routes)
        for case, want in zip(cases, routes):
            seqlens, n, k = case[:3]
            scan = case[3] if len(case) > 3 else lib.hpc_group_gemm_scan_wanted(len(seqlens), sum(seqlens))
            cin, out = (ctypes.c_int64 * 7)(1, 0, len(seqlens), sum(seqlens), n, k, int(scan)), (ctypes.c_int * 18)()
            assert lib.hpc_dev_ggemm_route(cin, 7, out, 18) == 0 and out[0] == 0
            assert (out[1], out[6] if out[1] == 1 else 0) == want, (name, _id(case), out[1], out[6])
            got.setdefault(want, set()).add(k // 128)
    every_kb = {1, 2, 3, 5, 11, 16}
    assert set().union(*got.values()) == every_kb and got[P8] == every_kb, got
    assert {n for _, n, _ in OP_CASES} == {256, 384, 512}
    lengths = {v for case in OP_CASES + ROW_INDEX_CASES + ROW_MAJOR_CASES for v in case[0]}
    assert {0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 256, 257, 265, 296, 456} <= lengths


MUTANTS = ["the neighbouring k-block's xs", "the neighbouring row's xs", "the neighbouring n-block's ws", "the neighbouring group's ws",
           "ws columns indexed with stride k / 128 instead of pad4", "the last k-block dropped", "the last k-block counted twice",
           "one row taken through the next group's weights", "the transposed layout read with the wrong tile_m",
           "truncating bf16 rounding"]
GENERAL_ONLY_MUTANTS = {"k-blocks summed in descending order": dict(order="descending"),
                        "the eager model's (part * xs) * ws and a separate add": dict(form="eager"),
                        "round(part * f), then an add": dict(form="round_product")}


def _model(c, kind, mutant=None):
    """the CPU model of the kernels' arithmetic, with one planted error"""
    s = c.kinds[kind]
    xs, ws_g, group, parts, order, form = s.xs, s.ws[:, :, : c.kb], c.group, c.parts, None, "fma"
    if mutant == MUTANTS[0]:
        xs = xs.roll(1, 1)
    elif mutant == MUTANTS[1]:
        xs = xs.roll(1, 0)
    elif mutant == MUTANTS[2]:
        ws_g = ws_g.roll(1, 1)
    elif mutant == MUTANTS[3]:
        ws_g = ws_g.roll(1, 0)
    elif mutant == MUTANTS[4]:
        ws_g = s.ws.reshape(c.G, -1)[:, : (c.n // 128) * c.kb].reshape(c.G, c.n // 128, c.kb)
    elif mutant == MUTANTS[5]:
        order = range(c.kb - 1)
    elif mutant == MUTANTS[6]:
        order = list(range(c.kb)) + [c.kb - 1]
    elif mutant == MUTANTS[7]:  # the last row of group 0 through the weights and weight scales of group 2 (group 1 is empty)
        r = int(c.cu[1]) - 1
        group, parts = group.clone(), parts.clone()
        group[r] = 2
        parts[:, r] = qr.blockwise_block_sums(c.x[r : r + 1], c.w, torch.tensor([2]))[:, 0]
    elif mutant == MUTANTS[8]:  # written with tile_m = 32 (117 rows per group), read with 16: group 2 starts at column 304, not 320
        xs = qr.xs_from_transposed(qr.xs_transposed(xs, c.sl, c.cu, 32), c.sl, 16)
    elif mutant in GENERAL_ONLY_MUTANTS:
        form = GENERAL_ONLY_MUTANTS[mutant].get("form", "fma")
        order = range(c.kb - 1, -1, -1) if "order" in GENERAL_ONLY_MUTANTS[mutant] else None
    tot = qr.blockwise_chain(parts, xs, ws_g[group], form, order)[0]
    return qr.bf16_truncate64(tot) if mutant == MUTANTS[9] else tot.float().bfloat16()


@pytest.mark.parametrize("n,k", MUTANT_NK)
def test_model_passes_both_bars(n, k):
    c = _case(L_RAGGED, n, k)
    assert _both_bars(c, lambda kind: _model(c, kind), f"model n{n} k{k}") == []


# (the stride mutant only where pad4(k / 128) != k / 128: at k / 128 = 4 the two strides are one and there is nothing to plant)
@pytest.mark.parametrize("mutant,n,k", [(m, n, k) for n, k in MUTANT_NK for m in MUTANTS if m != MUTANTS[4] or (k // 128) % 4])
def test_bars_reject_mutant(mutant, n, k):
    c = _case(L_RAGGED, n, k)
    assert _both_bars(c, lambda kind: _model(c, kind, mutant), f"{mutant}, n{n} k{k}") == ["pow2", "general"]


@pytest.mark.parametrize("mutant", sorted(GENERAL_ONLY_MUTANTS))
@pytest.mark.parametrize("n,k", MUTANT_NK)
def test_general_bar_rejects_another_arithmetic(mutant, n, k):
    """another order or another rounding of the same sum: exact on power-of-two scales (that bar cannot see it, by design), and
    at least one output of the general-scale case differs"""
    c = _case(L_RAGGED, n, k)
    assert torch.equal(_model(c, "pow2", mutant).view(torch.int16), c.kinds["pow2"].want.view(torch.int16))
    differ = int((_model(c, "general", mutant).view(torch.int16) != c.kinds["general"].want.view(torch.int16)).sum())
    print(f"{mutant}, n{n} k{k}: {differ}/{c.total * n} outputs differ from the statement")
    assert differ >= 1


# ------------------------------------------------------------------------------------------------------------ GPU
def _run_op(c, kind):
    """(a) the torch op: transposed, tile-padded scales, tile_m from the average"""
    import hpc

    s, avg = c.kinds[kind], c.total // c.G
    xs_t = qr.xs_transposed(s.xs, c.sl, c.cu, hpc.aligned_size(avg))
    y = hpc.group_gemm_blockwise_fp8(c.x.cuda(), c.w.cuda(), c.sl.cuda(), c.cu.cuda(), xs_t.cuda(), s.ws.cuda(), num_seq_per_group_avg=avg)
    torch.cuda.synchronize()
    return y.cpu()


def _run_entry(c, kind, row_index, scan):
    """(b) / (c) the C entry as csrc/fuse_moe.hip calls it: row-major scales (strides k / 128, 1), tile_m = 16, no col_base;
    (b) x and the scales read through row_index from a pool with spare rows, (c) row for row.  The output has guard rows."""
    import hpc
    from hpc import _C

    s = c.kinds[kind]
    x, xs = (c.pool, s.xs_pool) if row_index else (c.x, s.xs)
    # (rows behind the last one, as the fused op's workspace has them: zero codes and loud scales)
    x = torch.cat([x.view(torch.uint8), torch.zeros(PAD_ROWS, c.k, dtype=torch.uint8)]).view(F8)
    xs = torch.cat([xs, torch.full((PAD_ROWS, c.kb), qr.LOUD)])
    xd, wd, sld, cud, xsd, wsd, rid = (t.cuda() for t in (x, c.w, c.sl, c.cu, xs, s.ws, c.rows))
    cu128 = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum((c.sl + 127) // 128, 0).to(torch.int32)]).cuda()
    y = torch.full((c.total + GUARD_ROWS, c.n), SENTINEL, dtype=torch.bfloat16, device="cuda")
    rc = _C.lib.hpc_group_gemm_blockwise_fp8_async(_C.ptr(y), _C.ptr(xd), _C.ptr(wd), _C.ptr(sld), _C.ptr(cud), _C.ptr(xsd), _C.ptr(wsd),
                                                   _C.ptr(rid) if row_index else None, None, c.G, c.total, c.n, c.k, s.ws.shape[2], 16,
                                                   c.kb, 1, _C.ptr(cu128) if scan else None, _C.stream_of(y))
    assert rc == 0, rc
    torch.cuda.synchronize()
    y = y.cpu()
    assert bool((y[c.total :] == SENTINEL).all()), "rows behind m were written"
    return y[: c.total]


@pytest.mark.gpu
@pytest.mark.parametrize("case", OP_CASES, ids=_id)
def test_group_gemm_blockwise_exact(case):
    """(a) hpc.group_gemm_blockwise_fp8 on its default routes: <= 10 rows per group the streaming kernel at 16 tokens per pass,
    11 ... 20 at 32, above 20 the 256 x 256 kernel (n = 384: the 128 x 128 kernel); tile_m rungs 8, 16, 32, 48, 64 and 96 -> 48."""
    c = _case(*case)
    assert _both_bars(c, lambda kind: _run_op(c, kind), _id(case)) == []


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROW_INDEX_CASES, ids=_id)
def test_group_gemm_blockwise_row_index_exact(case):
    """(b) the fused MoE's gate-up form: below 16 rows per group the streaming kernel, from 16 the 256 x 256 kernel, n = 384 the
    128 x 128 kernel; without the scan and above 22 rows the streaming kernel's 48-tokens-per-pass form, which no other caller
    reaches with default keys"""
    seqlens, n, k, scan = case
    c = _case(seqlens, n, k, SPARE)
    assert _both_bars(c, lambda kind: _run_entry(c, kind, True, scan), "row_index " + _id(case)) == []


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROW_MAJOR_CASES, ids=_id)
def test_group_gemm_blockwise_row_major_exact(case):
    """(c) the fused MoE's down form: no row_index, the quantiser's row-major scales; 65 groups: the 256 x 256 kernel's work-item
    search takes a second round of 64 groups"""
    seqlens, n, k, scan = case
    c = _case(seqlens, n, k)
    assert _both_bars(c, lambda kind: _run_entry(c, kind, False, scan), "row-major " + _id(case)) == []


def _pinned(keys, run):
    for key, value in keys.items():
        dev_set(key, value)
    try:
        return run()
    finally:
        for key in keys:
            dev_set(key, 0)


def _pin_ids(keys):
    return "-".join(f"key{k}={v}" for k, v in keys.items())


# key 3: 1 streaming, 2 the 256 x 128 ring kernel (key 6 = 2 / 3: its 32- / 64-token forms, "12" / "22" of the tiled kernels' tests),
# 3 the 128 x 128 kernel, 4 the 256 x 256 kernel
TILED_PINS = [{3: 1}, {3: 2}, {3: 3}, {3: 4}, {3: 2, 6: 2}, {3: 2, 6: 3}]
# key 1: the streaming kernel's form (tokens per pass / waves); key 3 = 1 keeps the ragged groups on the streaming kernel at all
STREAM_PINS = [{3: 1, 1: v} for v in (1, 2, 3, 4, 16, 32)] + [{3: 1, 1: mt, 56: v} for mt in (1, 2) for v in (1, 2)]


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("keys", TILED_PINS + STREAM_PINS, ids=_pin_ids)
@pytest.mark.parametrize("n,k", PINNED_NK)
def test_group_gemm_blockwise_pinned_kernels_exact(keys, n, k):
    """every kernel form pinned through the development keys, ragged groups (empty, 1, 5, 128, 129, 257, 300), call form (a).
    (The 8-wave streaming forms need n % 128 == 0, which every blockwise call has: nothing is skipped.)"""
    c = _case(L_RAGGED, n, k)
    assert _both_bars(c, lambda kind: _pinned(keys, lambda: _run_op(c, kind)), f"{_pin_ids(keys)} n{n} k{k}") == []


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("keys", [{3: 1}, {3: 3}, {3: 4}], ids=_pin_ids)
@pytest.mark.parametrize("n,k", PINNED_NK)
def test_group_gemm_blockwise_pinned_kernels_row_index_exact(keys, n, k):
    """the streaming, the 128 x 128 and the 256 x 256 kernel pinned, through call form (b)"""
    c = _case(L_RAGGED, n, k, SPARE)
    assert _both_bars(c, lambda kind: _pinned(keys, lambda: _run_entry(c, kind, True, True)), f"row_index {_pin_ids(keys)} n{n} k{k}") == []


# ------------------------------------------------------------------------------------ the fused MoE equals its own stages
# (T, topk, E total, rank_ep, size_ep, H, inter, shared): rows per expert T * topk / E_local as fuse_moe hands it to the route
MOE_CASES = [(24, 2, 8, 0, 1, 256, 256, False),      # 6: streaming
             (48, 4, 8, 0, 1, 384, 512, True),       # 24: gate-up (n = 1024) the 256 x 256 kernel, down (n = 384) the 128 x 128 kernel
             (72, 2, 8, 0, 1, 512, 384, False),      # 18: with the scan the 256 x 256 kernel for both GEMMs; down k = 384
             (64, 4, 16, 1, 2, 512, 256, True),      # rank 1 of 2: half of the ids map to -1, 32 per local expert by m
             (48, 2, 16, 1, 4, 256, 128 * 3, False),  # rank 1 of 4: 24 by m, ~6 in fact
             ("sites", 1, 5, 0, 1, 512, 256, True)]  # EPILOGUE_SITE_ROWS: 265 / 40 / 100 / 456 / 296 rows, every epilogue site


@functools.lru_cache(maxsize=2)
def _moe_inputs(T, topk, E, rank_ep, size_ep, H, inter, shared):
    g = torch.Generator().manual_seed(H + inter + topk)
    if T == "sites":
        ids = topk1_ids_with_rows(EPILOGUE_SITE_ROWS)
        T = ids.shape[0]
    else:
        ids = torch.sort(torch.multinomial(torch.ones(T, E), topk, replacement=False, generator=g).to(torch.int32), dim=1)[0]
    el = E // size_ep
    x, guw = qr.gemm_exact_inputs((T,), 2 * inter, H, seed=T + H)
    guw = qr.gemm_exact_inputs((1,) * el, 2 * inter, H, seed=T + H + 1)[1]
    dw = qr.gemm_exact_inputs((1,) * el, H, inter, seed=T + H + 2)[1]
    xs, guws = qr.blockwise_scales(T, el, 2 * inter, H, seed=T + 1, kind="general")
    _, dws = qr.blockwise_scales(1, el, H, inter, seed=T + 2, kind="general")
    sc = torch.rand(T, topk, generator=g)
    sc = sc / sc.sum(1, keepdim=True)
    so = torch.randint(-8, 9, (T, H), generator=g).bfloat16() if shared else None
    return x, xs, guw, guws, dw, dws, ids, sc, so


@pytest.mark.gpu
@pytest.mark.parametrize("case", MOE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_fuse_moe_blockwise_equals_its_stages(case):
    """hpc.fuse_moe_blockwise_fp8 against count/slot -> gate-up GEMM -> activation -> down GEMM -> reduce, each called through
    the C ABI with exactly the arguments csrc/fuse_moe.hip::fuse_moe passes (m = T * topk whatever the rank keeps, tile_m = 128 for
    the scan and 16 for the GEMMs, row-major scales): the route is a pure function of the call, so both GEMMs run the fused op's
    kernels, and where the fused op has the activation in the gate-up epilogue tests/test_fuse_moe_blockwise.py pins that to the
    separate kernel's bits.  The outputs are equal BIT FOR BIT, and the chain's gate-up matrix is the CPU statement (exact
    integer inputs, general scales) bit for bit - the e4m3 ties of the activation cannot enter either."""
    import hpc
    from hpc import _C

    lib, p = _C.lib, _C.ptr
    _, topk, E, rank_ep, size_ep, H, inter, shared = case
    x, xs, guw, guws, dw, dws, ids, sc, so = _moe_inputs(*case)
    T, el, m = x.shape[0], E // size_ep, x.shape[0] * topk
    d = [t.cuda() if t is not None else None for t in (x, xs, guw, guws, dw, dws, ids, sc, so)]
    xd, xsd, guwd, guwsd, dwd, dwsd, idsd, scd, sod = d
    fused = hpc.fuse_moe_blockwise_fp8(xd, xsd, guwd, guwsd, dwd, dwsd, idsd, scd, rank_ep, E, sod)
    torch.cuda.synchronize()

    i32, st = dict(dtype=torch.int32, device="cuda"), _C.stream_of(xd)
    seqlens, cu, tiles, cu_tiles = torch.empty(el, **i32), torch.empty(el + 1, **i32), torch.empty(el, **i32), torch.empty(el + 1, **i32)
    pos, row_index = torch.empty(T, topk, **i32), torch.zeros(m, **i32)
    gate_up = torch.full((m + GUARD_ROWS, 2 * inter), SENTINEL, dtype=torch.bfloat16, device="cuda")
    down_in = torch.zeros((m + PAD_ROWS, inter), dtype=torch.uint8, device="cuda")
    down_in_scale = torch.full((m + PAD_ROWS, inter // 128), qr.LOUD, dtype=torch.float32, device="cuda")
    down_out = torch.full((m + GUARD_ROWS, H), SENTINEL, dtype=torch.bfloat16, device="cuda")
    y = torch.empty((T, H), dtype=torch.bfloat16, device="cuda")
    assert lib.hpc_moe_count_and_slot_async(p(idsd), T, topk, el, rank_ep, 128, p(seqlens), p(cu), p(tiles), p(cu_tiles), p(pos),
                                            p(row_index), st) == 0
    assert lib.hpc_group_gemm_blockwise_fp8_async(p(gate_up), p(xd), p(guwd), p(seqlens), p(cu), p(xsd), p(guwsd), p(row_index), None, el,
                                                  m, 2 * inter, H, guws.shape[2], 16, H // 128, 1, p(cu_tiles), st) == 0
    num_rows = ctypes_offset(cu, el)
    assert lib.hpc_act_mul_and_blockwise_quant_async(p(down_in), p(down_in_scale), p(gate_up), num_rows, m, inter, inter // 128, 1, None,
                                                     st) == 0
    assert lib.hpc_group_gemm_blockwise_fp8_async(p(down_out), p(down_in), p(dwd), p(seqlens), p(cu), p(down_in_scale), p(dwsd), None, None,
                                                  el, m, H, inter, dws.shape[2], 16, inter // 128, 1, p(cu_tiles), st) == 0
    assert lib.hpc_moe_reduce_async(p(y), p(down_out), p(pos), p(scd), p(sod), T, topk, H, st) == 0
    torch.cuda.synchronize()

    # the chain's gate-up matrix against the CPU statement: output row r of local expert e reads token row_index[r]
    sl, rows = seqlens.cpu(), row_index.cpu()
    total = int(sl.sum())
    local = (ids >= rank_ep * el) & (ids < (rank_ep + 1) * el)
    assert torch.equal(sl.long(), torch.bincount((ids[local] - rank_ep * el).long(), minlength=el)) and total == int(local.sum())
    group = torch.repeat_interleave(torch.arange(el), sl.long())
    tok = rows[:total].long()
    parts = qr.blockwise_block_sums(x.view(torch.uint8)[tok].view(F8), guw, group)
    tot, flagged, exact, _, _ = qr.blockwise_chain(parts, xs[tok].contiguous(), guws[group][:, :, : H // 128])
    assert flagged == 0
    got = gate_up.cpu()
    differ = int((got[:total].view(torch.int16) != tot.float().bfloat16().view(torch.int16)).sum())
    fused_differ = int((fused.view(torch.int16) != y.view(torch.int16)).sum())
    print(f"fused MoE {case}: {total} routed rows of {m}, longest group {int(sl.max())}; gate-up matrix: {differ}/{total * 2 * inter} "
          f"outputs differ from the statement; fused op against its stages: {fused_differ}/{y.numel()} outputs differ")
    assert bool((got[m:] == SENTINEL).all()) and bool((down_out[m:] == SENTINEL).all()), "rows behind m were written"
    assert differ == 0
    assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0
    assert fused_differ == 0


def ctypes_offset(t, index):
    """device pointer of element `index` of an int32 tensor"""
    import ctypes

    return ctypes.c_void_p(t.data_ptr() + 4 * index)
