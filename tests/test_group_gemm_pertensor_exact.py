"""The per-tensor grouped FP8 GEMMs on inputs that make the answer exact: x in -3 ... 3 and w in -4 ... 4 as e4m3, so every
partial sum of a row of x @ w[g].T is an integer below 12 * k <= 21504 < 2^15 - exact in fp32 in any order and any grouping
(tests/quant_ref.py::gemm_exact_inputs) - and the bf16 output is determined bit for bit.  Two bars per case:

* per-group scales that are powers of two, all different (2^-3 ... 2^1 cycled): the output equals bf16(exact * scale), rounded
  to nearest even, BIT FOR BIT.  Many of the integer sums sit exactly on bf16 ties (at least 1 % is asserted), so this pins the
  rounding mode too; a dropped or doubled half k-block, a neighbour's scale or a neighbour's row each change whole tiles.
* general scales rand + 0.5: within half a bf16 ulp plus 2^-22 of the value (tests/utils.py::quant_close).  Derived, not
  measured: the kernel's fp32 product exact * scale rounds once, 2^-24 relative, before the bf16 rounding; 2^-22 is that
  with a margin of 4 x.

CPU: five planted errors each fail both bars; every case's generator gives its share of ties.
Measured on the MI355X: none of the outputs of the 28 power-of-two cases differs (2.05 % ties the least); general scales,
worst excess 1.9e-9 = 0.008 x the slack.  The streaming and the 128 x 128 kernels missed the general bar while they folded
the scale into every k-block; they multiply the unscaled sum once now (csrc/group_gemm_blockwise.hip, csrc/group_gemm_tiled.hip)."""
import functools

import pytest
import torch

import quant_ref as qr
from utils import dev_set, quant_close, quant_excess, ulp_bf16

F8 = torch.float8_e4m3fn
GEMM_SLACK = 2.0 ** -22


def _eight(m):
    return (m, m, 0, m, m, m, m, m)


K_ALL = [64, 192, 1088, 1792]  # 192 and 1088 end in a half k-block (K % 128 == 64); 64 is one
MIXED = (0, 1, 129, 64, 65, 257, 16, 17)
# (seqlens, n, k): the shapes tests/test_fuse_moe_pertensor.py names for the routing table, then the mixed groups at every k
DEFAULT_CASES = [((0, 1, 129), 256, 64), ((0, 1, 129), 192, 128), (_eight(8), 1024, 1792), (_eight(30), 1024, 1792),
                 (_eight(70), 1024, 1792)] + [(MIXED, 512, k) for k in K_ALL]
TILED_SEQLENS = (200, 0, 129, 3, 260)
CP_ASYNC_CASES = [(48, 42, 512, 192), (8, 200, 256, 1024)]


def _cp_async_seqlens(num_group, actual_m):
    return tuple(actual_m - 5 if i == 1 else actual_m for i in range(num_group))


def _id(case):
    seqlens, n, k = case
    return f"{'x'.join(map(str, seqlens)) if len(seqlens) <= 8 else f'{len(seqlens)}groups'}-n{n}-k{k}"


def _scales(num_group, kind):
    if kind == "pow2":
        return torch.exp2(((torch.arange(num_group) % 5) - 3).float())
    return torch.rand(num_group, generator=torch.Generator().manual_seed(num_group)) + 0.5


@functools.lru_cache(maxsize=4)
def _case(seqlens, n, k, spare_rows=0):
    """-> (x pool, w, seqlens, cu, rows of the pool each output row reads, exact sums float64, group of every row); the exact
    sums are computed once and shared by both bars"""
    G, total = len(seqlens), sum(seqlens)
    pool, w = qr.gemm_exact_inputs(seqlens, n, k, seed=total * 31 + n + k, spare_rows=spare_rows)
    rows = torch.randperm(total + spare_rows, generator=torch.Generator().manual_seed(k))[:total] if spare_rows else torch.arange(total)
    sl = torch.tensor(seqlens, dtype=torch.int32)
    cu = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(sl, 0).to(torch.int32)])
    x = pool.view(torch.uint8)[rows].view(F8)
    acc = qr.group_gemm_pertensor_exact(x, w, sl, cu, torch.ones(G))
    assert float(acc.abs().max()) <= 12 * k < 2 ** 15 and bool((acc == acc.round()).all())
    return pool, w, sl, cu, rows.to(torch.int32), acc, torch.repeat_interleave(torch.arange(G), sl.long())


def _both_bars(acc, group, num_group, run, label):
    """run(scale) -> bf16 output; both bars on it.  -> list of the bars missed"""
    missed = []
    for kind in ("pow2", "general"):
        scale = _scales(num_group, kind)
        y64 = acc * scale[group].double().unsqueeze(1)
        got = run(scale)
        assert got.dtype == torch.bfloat16 and got.shape == y64.shape
        if kind == "pow2":
            want = qr.bf16_rne64(y64)
            same = got.view(torch.int16) == want.view(torch.int16)
            ties = qr.bf16_tie_share(y64)
            print(f"{label} pow2 scales: {int((~same).sum())}/{same.numel()} outputs differ from bf16(exact * scale); {ties:.2%} of them are ties")
            assert ties >= 0.01, ties  # the generator's part of the bargain
            if not bool(same.all()):
                bad = torch.nonzero(~same)[:10]
                for r, c in bad.tolist():
                    print(f"  ({r}, {c}) group {int(group[r])}: got {float(got[r, c]):.9g} want {float(want[r, c]):.9g} exact {float(y64[r, c]):.9g}")
                missed.append(kind)
        elif not quant_close(y64, got, ulp_bf16, GEMM_SLACK, f"{label} general scales"):
            missed.append(kind)
    return missed


# ------------------------------------------------------------------------------------------------------------ CPU
def test_bf16_rne64_and_ties():
    v = torch.tensor([257.0, 259.0, 258.0, -257.0, -259.0, 1.0, 0.0, 1027.0 * 0.125, 21504.0, 3.0 + 2.0 ** -30], dtype=torch.float64)
    want = torch.tensor([256.0, 260.0, 258.0, -256.0, -260.0, 1.0, 0.0, 128.0, 21504.0, 3.0]).bfloat16()
    assert torch.equal(qr.bf16_rne64(v), want)
    assert qr.bf16_tie_share(v) == 0.4  # 257, 259 and their negatives; 1027 / 8 is not half way
    assert torch.equal(qr.bf16_truncate64(v), torch.tensor([256.0, 258.0, 258.0, -256.0, -258.0, 1.0, 0.0, 128.0, 21504.0, 3.0]).bfloat16())
    g = torch.Generator().manual_seed(0)
    r = (torch.randn(4096, generator=g) * 300).bfloat16().double()  # what bf16 holds comes back as it is
    assert torch.equal(qr.bf16_rne64(r).double(), r)
    r32 = (torch.randint(-21504, 21505, (4096,), generator=g)).double()  # and what fp32 holds rounds as fp32 -> bf16 does
    assert torch.equal(qr.bf16_rne64(r32), r32.float().bfloat16())


@pytest.mark.parametrize("case", DEFAULT_CASES + [(TILED_SEQLENS, 512, k) for k in (1792, 1088, 192)], ids=_id)
def test_generator_gives_ties(case):
    _, _, _, _, _, acc, _ = _case(*case)
    assert qr.bf16_tie_share(acc) >= 0.01, qr.bf16_tie_share(acc)  # a power-of-two scale moves no tie


@pytest.mark.parametrize("num_group,actual_m,n,k", CP_ASYNC_CASES)
def test_generator_gives_ties_cp_async(num_group, actual_m, n, k):
    assert qr.bf16_tie_share(_case(_cp_async_seqlens(num_group, actual_m), n, k, 7)[5]) >= 0.01


MUTANTS = ["the neighbouring group's scale", "last 64 columns of k dropped", "last 64 columns of k counted twice",
           "one row taken from the next group", "truncating bf16 rounding"]


@pytest.mark.parametrize("k", [192, 1088])
@pytest.mark.parametrize("mutant", MUTANTS)
def test_bars_reject_mutant(mutant, k):
    _, w, sl, cu, _, acc, group = _case(TILED_SEQLENS, 512, k)
    x = _case(TILED_SEQLENS, 512, k)[0]

    def model(scale, mutant=None):
        a, g = acc, group
        if mutant and mutant.startswith("last 64"):
            tail = qr.group_gemm_pertensor_exact(x[:, k - 64 :], w[:, :, k - 64 :], sl, cu, torch.ones(len(sl)))
            a = acc - tail if mutant.endswith("dropped") else acc + tail
        if mutant == "one row taken from the next group":  # the last row of group 0 through group 2's weights and scale
            r = int(cu[1]) - 1
            a, g = acc.clone(), group.clone()
            a[r], g[r] = x[r].double() @ w[2].double().t(), 2
        if mutant == "the neighbouring group's scale":
            scale = scale.roll(1)
        y64 = a * scale[g].double().unsqueeze(1)
        return qr.bf16_truncate64(y64) if mutant == "truncating bf16 rounding" else qr.bf16_rne64(y64.float().double())

    assert _both_bars(acc, group, len(sl), model, f"model, k {k}") == []
    assert _both_bars(acc, group, len(sl), lambda s: model(s, mutant), f"{mutant}, k {k}") == ["pow2", "general"]
    y64 = acc * _scales(len(sl), "general")[group].double().unsqueeze(1)
    good, bad = (float(quant_excess(y64, model(_scales(len(sl), "general"), m), ulp_bf16).max()) for m in (None, mutant))
    print(f"{mutant}, k {k}: worst excess {bad:.3g} = {bad / GEMM_SLACK:.3g} x the slack of 2^-22; the model's own {good:.3g}")


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", DEFAULT_CASES, ids=_id)
def test_group_gemm_pertensor_exact(case):
    import hpc

    x, w, sl, cu, _, acc, group = _case(*case)
    xd, wd, sld, cud = x.cuda(), w.cuda(), sl.cuda(), cu.cuda()
    run = lambda scale: hpc.group_gemm_pertensor_fp8(xd, wd, sld, cud, scale.cuda(), num_seq_per_group_avg=int(sl.max())).cpu()  # noqa: E731
    assert _both_bars(acc, group, len(sl), run, _id(case)) == []


@pytest.mark.dev
@pytest.mark.gpu
@pytest.mark.parametrize("tiled_mode", [2, 3, 4, 12, 22])  # as tests/test_fuse_moe_pertensor.py::test_group_gemm_pertensor_tiled_kernels
@pytest.mark.parametrize("k", [1792, 1088, 192])
def test_group_gemm_pertensor_tiled_kernels_exact(tiled_mode, k):
    import hpc

    x, w, sl, cu, _, acc, group = _case(TILED_SEQLENS, 512, k)
    xd, wd, sld, cud = x.cuda(), w.cuda(), sl.cuda(), cu.cuda()

    def run(scale):
        dev_set(3, tiled_mode % 10)
        dev_set(6, 1 + tiled_mode // 10)  # 1x: 32-token tiles, 2x: 64-token tiles
        try:
            my = hpc.group_gemm_pertensor_fp8(xd, wd, sld, cud, scale.cuda(), num_seq_per_group_avg=int(sl.sum()) // len(sl))
            torch.cuda.synchronize()
        finally:
            dev_set(3, 0)
            dev_set(6, 0)
        return my.cpu()

    assert _both_bars(acc, group, len(sl), run, f"tiled mode {tiled_mode} k {k}") == []


@pytest.mark.gpu
@pytest.mark.parametrize("num_group,actual_m,n,k", CP_ASYNC_CASES)
@pytest.mark.parametrize("scatter", [False, True])
def test_group_gemm_cp_async_ops_exact(num_group, actual_m, n, k, scatter):
    """the scatter form reads its rows from a pool through row_indices, as tests/test_fuse_moe_pertensor.py has it"""
    import hpc  # noqa: F401

    pool, w, sl, cu, rows, acc, group = _case(_cp_async_seqlens(num_group, actual_m), n, k, 7)
    tiles = (sl + 63) // 64
    cu_tiles = torch.cat([torch.zeros(1, dtype=torch.int32), torch.cumsum(tiles, 0).to(torch.int32)])
    d = lambda t: t.cuda()  # noqa: E731
    x_compact = pool.view(torch.uint8)[rows.long()].view(F8)

    def run(scale):
        if scatter:
            my = torch.ops.hpc.group_gemm_fp8_scatter_cp_async(d(pool), d(w), d(scale), d(rows), d(sl), d(cu), d(tiles), d(cu_tiles), False)
        else:
            my = torch.ops.hpc.group_gemm_fp8_cp_async(d(x_compact), d(w), d(scale), d(sl), d(cu), d(tiles), d(cu_tiles), True)
        return my.cpu()

    assert _both_bars(acc, group, len(sl), run, f"cp_async scatter {scatter} {num_group}x{actual_m} n{n} k{k}") == []
