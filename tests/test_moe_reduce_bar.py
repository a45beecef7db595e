"""hpc.reduce (csrc/fuse_moe.hip::reduce_kernel) held to its statement: acc = fmaf(float(x[pos_j]), scale_j, acc) in j order,
pos < 0 skipped, then acc += shared, one bf16 rounding.

Inputs: x bf16 of integers in -200 ... 200; positions a random injective map into x with about a third of the entries -1 and one
token whose positions are ALL -1; every row of x that no position names (but row 0, which a `-1` read as an index would hit) is
NaN, and topk_scale is NaN at every skipped position: neither may reach the output.  hidden 8 / 520 / 2056 (one 16-byte vector,
one and a bit workgroups' worth, more than one workgroup per token), num_topk 1 / 8 / 128 (the kernel's limit), with and without
shared_output.  Two bars:

* power-of-two scales 2^-3 ... 2^1 and a shared_output of integers: every partial sum is a multiple of 2^-3 below 2^16 - exact in
  fp32 - so the output equals bf16(exact sum), rounded to nearest even, BIT FOR BIT.  At least 1 % of the sums are bf16 ties
  (asserted) - except for num_topk = 1 without shared_output, where the sum IS a bf16 value times a power of two and nothing is
  rounded at all.
* general scales (rand): |y - r| <= half a bf16 ulp of r + (num_topk + 1) 2^-24 A, r the float64 sum and A the sum of the
  absolute terms.  Derived, not measured: one fp32 rounding per FMA and one for the shared add, each at most 2^-24 of a partial
  sum that A bounds.

CPU: five planted errors (a -1 position read as row 0, the neighbouring token's scale, shared_output added twice or left out,
truncation) each fail both bars; the model passes them.
Measured on the MI355X: 0 of the outputs of the 18 power-of-two cases differ (2.08 % ties the least where any exist); general
scales, worst excess over half an ulp 0.012 x the derived bar."""
import functools
import types

import pytest
import torch

import quant_ref as qr
from utils import ulp_bf16

KINDS = ("pow2", "general")
HIDDEN, TOPK, TOKENS, ALL_SKIPPED = [8, 520, 2056], [1, 8, 128], 6, 2
MUTANTS = ["a -1 position read as row 0", "the neighbouring token's scale", "shared_output added twice", "shared_output left out",
           "truncating bf16 rounding"]


@functools.lru_cache(maxsize=None)
def _case(hidden, topk):
    g = torch.Generator().manual_seed(hidden * 131 + topk)
    rows = TOKENS * topk + 5
    x = torch.randint(-200, 201, (rows, hidden), generator=g).bfloat16()
    pos = torch.randperm(rows, generator=g)[: TOKENS * topk].reshape(TOKENS, topk).to(torch.int32)
    drop = torch.rand(TOKENS, topk, generator=g) < 1 / 3
    drop[ALL_SKIPPED], drop[0, 0], drop[1, 0] = True, False, True  # one kept and one skipped entry whatever the draw
    pos[drop] = -1
    named = torch.zeros(rows, dtype=torch.bool)
    named[pos[pos >= 0].long()] = True
    named[0] = True  # row 0 stays finite: reading a -1 as an index must show as a wrong VALUE, not only as a NaN
    x[~named] = float("nan")
    shared = torch.randint(-200, 201, (TOKENS, hidden), generator=g).bfloat16()
    c = types.SimpleNamespace(x=x, pos=pos, shared=shared, hidden=hidden, topk=topk, scale={}, ref={})
    for kind in KINDS:
        sc = torch.exp2(torch.randint(-3, 2, (TOKENS, topk), generator=g).float()) if kind == "pow2" else torch.rand(TOKENS, topk, generator=g)
        sc[pos < 0] = float("nan")
        c.scale[kind] = sc
        for with_shared in (False, True):
            acc, exact, big_a = qr.moe_reduce_chain(x, pos, sc, shared if with_shared else None)
            assert bool(torch.isfinite(exact).all()) and bool((exact[ALL_SKIPPED] == (shared[ALL_SKIPPED].double() if with_shared else 0)).all())
            if kind == "pow2":
                assert torch.equal(acc, exact) and float(big_a.max()) < 2.0 ** 16  # multiples of 2^-3: 19 bits
                if topk > 1 or with_shared:
                    assert qr.bf16_tie_share(exact) >= 0.01, qr.bf16_tie_share(exact)
            c.ref[kind, with_shared] = (acc, exact, big_a)
    return c


def _bars(c, run, label):
    """run(kind, shared or None) -> bf16 [TOKENS, hidden] on the CPU.  -> the (kind, with_shared) pairs that miss their bar"""
    missed = []
    for kind in KINDS:
        for with_shared in (False, True):
            acc, exact, big_a = c.ref[kind, with_shared]
            got = run(kind, c.shared if with_shared else None)
            assert got.dtype == torch.bfloat16 and got.shape == exact.shape
            if kind == "pow2":
                differ = int((got.view(torch.int16) != qr.bf16_rne64(exact).view(torch.int16)).sum())
                print(f"{label} pow2 scales, shared {with_shared}: {differ}/{got.numel()} outputs differ from bf16(exact); "
                      f"{qr.bf16_tie_share(exact):.2%} of the sums are ties")
                ok = differ == 0
            else:
                bar = (c.topk + 1) * 2.0 ** -24 * big_a
                over = ((got.double() - exact).abs() - 0.5 * ulp_bf16(exact)).nan_to_num(nan=float("inf"))
                over = torch.where(big_a == 0, (got.double() != 0).double() * float("inf"), over).nan_to_num(nan=0.0)
                worst = float((over / bar.clamp_min(1e-300)).max())
                print(f"{label} general scales, shared {with_shared}: worst excess over half an ulp = {worst:.3g} x the derived bar")
                ok = bool((over <= bar).all())
            if not ok:
                missed.append((kind, with_shared))
    return missed


def _model(c, kind, shared, mutant=None):
    sc = c.scale[kind].roll(1, 0) if mutant == MUTANTS[1] else c.scale[kind]
    times = 2 if mutant == MUTANTS[2] else (0 if mutant == MUTANTS[3] else 1)
    acc = qr.moe_reduce_chain(c.x, c.pos, sc, shared, skip=mutant != MUTANTS[0], shared_times=times)[0]
    return qr.bf16_truncate64(acc) if mutant == MUTANTS[4] else acc.float().bfloat16()


ALL_FOUR = [(k, s) for k in KINDS for s in (False, True)]


@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("topk", TOPK)
def test_model_passes(hidden, topk):
    c = _case(hidden, topk)
    assert _bars(c, lambda kind, shared: _model(c, kind, shared), f"model h{hidden} topk{topk}") == []


@pytest.mark.parametrize("hidden,topk", [(520, 8), (2056, 128)])
@pytest.mark.parametrize("mutant", MUTANTS)
def test_bars_reject_mutant(mutant, hidden, topk):
    """the two errors in the shared add can only show where there is a shared_output; the others miss all four bars"""
    c = _case(hidden, topk)
    want = [(k, True) for k in KINDS] if "shared_output" in mutant else ALL_FOUR
    assert _bars(c, lambda kind, shared: _model(c, kind, shared, mutant), f"{mutant}, h{hidden} topk{topk}") == want


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("topk", TOPK)
def test_reduce_bar(hidden, topk):
    import hpc

    c = _case(hidden, topk)

    def run(kind, shared):
        y = hpc.reduce(c.x.cuda(), c.pos.cuda(), c.scale[kind].cuda(), None if shared is None else shared.cuda())
        torch.cuda.synchronize()
        return y.cpu()

    assert _bars(c, run, f"hpc.reduce h{hidden} topk{topk}") == []
