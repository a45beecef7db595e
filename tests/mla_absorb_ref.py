"""The statements of hpc.mla_absorb_q / hpc.mla_unabsorb_o on CPU tensors, the knobs the tests turn to make mutants of them,
the bar, an fp32 restatement and the input builders.

    absorb_q     r[t, h, c] = sum_{d < 128} q_nope[t, h, d] * w_uk[h, d, c]        c < 512
    unabsorb_o   r[t, h, v] = sum_{c < 512} o_lat[t, h, c] * w_uv[h, v, c]         v < 128

Both statements are float64 and return (r, A) with A = sum |terms|, unrounded.  The ops return bf16(r) after an fp32
accumulation in some order.  A product of two bf16 values is exact in fp32, so the bar is derived, not measured:

    |y - r| <= 2^-8 |r| + K * 2^-23 * A        per element (K = 128 or 512)

the first term bf16's worst half ulp, the second the any-order fp32 summation bound K * 2^-24 * A doubled for the matrix
instruction's own adder (DESIGN, MLA-decode bars: worth about one more fp32 accumulation).

quant=True is the rule of tests/blockwise_quant_ref.py per (token, head) on the bf16-rounded o."""
import functools
from types import SimpleNamespace

import torch

import blockwise_quant_ref as bq

BF16 = torch.bfloat16
NOPE, LAT = 128, 512
# (T, H) of the GPU cases: partial and multiple token tiles at H = 16, the head counts at T = 17, and one shape past the
# threshold (H * 4 * ceil(T / 64) > 512) at which absorb_q's workgroups take 256 tokens, several blocks to a wave
SHAPES = ((1, 16), (15, 16), (16, 16), (17, 16), (64, 16), (65, 16), (130, 16), (17, 1), (17, 48), (17, 128), (130, 128))
TOKEN_BLOCK = 16  # tokens of one matrix-instruction block: what the row mutant moves across


# ------------------------------------------------------------------------------------------------------ the statements
def absorb_q_statement(q_nope, w_uk, head_shift=0, drop_last=0, d_contiguous=False, row_from_neighbour=False):
    """(r, A) float64 [T, H, 512].  Knobs (mutants): head h uses head h + head_shift's weight; the last drop_last of the
    reduction dropped; w_uk's [128, 512] block read as if d were contiguous ([512, 128] transposed); the last row of every
    16-token block taken from the next token."""
    x, w = q_nope.double(), w_uk.double()
    return _product(x, w.transpose(1, 2), head_shift, drop_last, d_contiguous, row_from_neighbour)


def unabsorb_o_statement(o_lat, w_uv, head_shift=0, drop_last=0, row_from_neighbour=False):
    """(r, A) float64 [T, H, 128]; knobs as absorb_q_statement's"""
    return _product(o_lat.double(), w_uv.double(), head_shift, drop_last, False, row_from_neighbour)


def _product(x, w_nk, head_shift, drop_last, reinterpret, row_from_neighbour):
    """x [T, H, K], w_nk [H, N, K] -> sum_k x[t, h, k] w_nk[h, n, k] and the sum of the terms' magnitudes"""
    if reinterpret:  # the [K, N] block of memory read as [N, K]
        H, N, K = w_nk.shape
        w_nk = w_nk.transpose(1, 2).contiguous().view(H, N, K)
    if head_shift:
        w_nk = torch.roll(w_nk, -head_shift, 0)
    if drop_last:
        x, w_nk = x[..., :-drop_last], w_nk[..., :-drop_last]
    if row_from_neighbour:
        x = x.clone()
        T = x.shape[0]
        for t in range(TOKEN_BLOCK - 1, T - 1, TOKEN_BLOCK):
            x[t] = x[t + 1]
    r = torch.einsum("thk,hnk->thn", x, w_nk)
    A = torch.einsum("thk,hnk->thn", x.abs(), w_nk.abs())
    return r.contiguous(), A.contiguous()


def bar(r, A, K):
    return 2.0 ** -8 * r.abs() + K * 2.0 ** -23 * A


def worst_ratio(y, r, A, K):
    """max over elements of |y - r| / bar; an element with bar 0 must be exact"""
    err, b = (y.double() - r).abs(), bar(r, A, K)
    assert bool((err[b == 0] == 0).all())
    return float((err / b.clamp_min(1e-300)).max())


def fp32_restatement(x, w_nk):
    """bf16( fp32 sum ), accumulated in 32-wide steps like the matrix instruction: x [T, H, K] bf16, w_nk [H, N, K] bf16"""
    K = x.shape[-1]
    acc = torch.zeros(x.shape[0], x.shape[1], w_nk.shape[1], dtype=torch.float32)
    for k in range(0, K, 32):
        acc += torch.einsum("thk,hnk->thn", x[..., k: k + 32].float(), w_nk[..., k: k + 32].float())
    return acc.to(BF16)


def quant_statement(o_bf16, head_shift=0, cols=128):
    """o_bf16 [T, H * 128] -> (codes e4m3fn [T, H * 128], scale f32 [T, H]): tests/blockwise_quant_ref.py::quant.  Knobs: the
    scale of head h + head_shift; a scale taken over the first `cols` columns of a head only."""
    T, HN = o_bf16.shape
    H = HN // NOPE
    if head_shift == 0 and cols == 128:
        return bq.quant(o_bf16)
    b = o_bf16.float().view(T, H, NOPE)
    s = b[..., :cols].abs().amax(-1) / 448.0
    s = torch.roll(s, -head_shift, 1)
    q = (b * (1.0 / (s + 1e-8)).unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(T, HN), s


# ------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def random_case(T, H, seed=0):
    """activations with per-(token, head) magnitudes 2^e, e in -6 .. 6 - a wrong head or row index cannot hide -, weights
    randn * 0.05 as the two halves of one [H, 256, 512] kv_b weight"""
    g = torch.Generator().manual_seed(1000 * T + H + seed)
    mag = lambda: 2.0 ** torch.randint(-6, 7, (T, H, 1), generator=g).double()  # noqa: E731
    q = (torch.randn(T, H, NOPE, generator=g).double() * mag()).to(BF16)
    o_lat = (torch.randn(T, H, LAT, generator=g).double() * mag()).to(BF16)
    w_kv_b = (torch.randn(H, 2 * NOPE, LAT, generator=g) * 0.05).to(BF16)
    return _finish(T, H, q, o_lat, w_kv_b)


@functools.lru_cache(maxsize=None)
def exact_case(T, H, seed=0):
    """small integers, three in four of them zero: every partial sum is an integer far below 2^24, so the fp32 sum is exact in
    any order and the op's output is the float64 statement rounded once - bit for bit"""
    g = torch.Generator().manual_seed(2000 * T + H + seed)

    def ints(*shape, hi):
        v = torch.randint(-hi, hi + 1, shape, generator=g)
        return (v * (torch.randint(0, 4, shape, generator=g) == 0)).to(BF16)

    return _finish(T, H, ints(T, H, NOPE, hi=8), ints(T, H, LAT, hi=8), ints(H, 2 * NOPE, LAT, hi=4))


def _finish(T, H, q, o_lat, w_kv_b):
    c = SimpleNamespace(T=T, H=H, q=q, o_lat=o_lat, w_kv_b=w_kv_b, w_uk=w_kv_b[:, :NOPE], w_uv=w_kv_b[:, NOPE:])
    c.q_ref = absorb_q_statement(c.q, c.w_uk)      # computed once, shared read-only
    c.o_ref = unabsorb_o_statement(c.o_lat, c.w_uv)
    return c
