"""The PyTorch statement of hpc.gemm_blockwise_fp8 (no reference kernel exists) and the builders of its test inputs.
CPU tensors only; the cached builders' results are shared between tests and must not be written."""
import functools

import torch

import blockwise_quant_ref

F8 = torch.float8_e4m3fn


def _partials(xq, wq):
    """float64 [M, N, K/128]: the dot product of every (token, weight row) pair inside every block of 128 consecutive k."""
    m, k = xq.shape
    n = wq.shape[0]
    return torch.einsum("mbk,nbk->mnb", xq.double().view(m, k // 128, 128), wq.double().view(n, k // 128, 128))


def ref(xq, xs, wq, ws):
    """xq e4m3 [M, K], xs f32 [M, K/128], wq e4m3 [N, K], ws f32 [ceil(N/128), K/128] -> (r, A), both float64 [M, N]:
        r[m, n] = sum_kb xs[m, kb] * ws[n // 128, kb] * sum_{k in block kb} xq[m, k] * wq[n, k]
        A[m, n] = sum_kb |xs[m, kb] * ws[n // 128, kb] * (that block's sum)|
    r is NOT rounded to bf16; A bounds the magnitudes an fp32 evaluation adds up."""
    assert xq.device.type == "cpu" and xq.dtype == F8 and wq.dtype == F8 and xq.shape[1] == wq.shape[1] and xq.shape[1] % 128 == 0
    n = wq.shape[0]
    assert xs.shape == (xq.shape[0], xq.shape[1] // 128) and ws.shape == ((n + 127) // 128, xq.shape[1] // 128)
    wsn = ws.double().repeat_interleave(128, 0)[:n]  # [N, KB]
    term = xs.double()[:, None, :] * wsn[None, :, :] * _partials(xq, wq)
    return term.sum(-1), term.abs().sum(-1)


def bar(r, a, k):
    """What |y - r| may be, per element: bf16's worst half ulp of r, plus one fp32 rounding per rescale, accumulate and plane add
    (K/128 blocks + at most 16 planes + slack = K/128 + 24 roundings) on magnitudes bounded by A."""
    return 2.0 ** -8 * r.abs() + (k // 128 + 24) * 2.0 ** -23 * a


def fp32_restatement(xq, xs, wq, ws, splits):
    """The kernel's arithmetic in float32 on the CPU: per K slice tot += (block dot in fp32) * (xs * ws), then the slices'
    planes summed in slice order; bf16 at the end.  Returns bfloat16 [M, N]."""
    m, k = xq.shape
    n, kb = wq.shape[0], k // 128
    x32, w32 = xq.float().view(m, kb, 128), wq.float().view(n, kb, 128)
    wsn = ws.float().repeat_interleave(128, 0)[:n]
    total = None
    for s in range(splits):
        tot = torch.zeros(m, n, dtype=torch.float32)
        for b in range(kb * s // splits, kb * (s + 1) // splits):
            tot = tot + (x32[:, b] @ w32[:, b].t()) * (xs[:, b, None] * wsn[None, :, b])
        total = tot if total is None else total + tot
    return total.bfloat16()


@functools.lru_cache(maxsize=None)
def exact_inputs(m, n, k, seed=0):
    """(xq, xs, wq, ws, want): codes are integers in -2 .. 2, both scale tensors powers of two in 2^-3 .. 2^1 drawn per (row,
    block) and per weight block.  Every partial sum is a multiple of 2^-6 below 2^17, exact in fp32 in any order, so
    want = bf16(ref) must come out bit for bit whatever the split count."""
    g = torch.Generator().manual_seed(seed * 1000003 + m * 7919 + n * 31 + k)
    kb = k // 128
    xq = torch.randint(-2, 3, (m, k), generator=g).float().to(F8)
    wq = torch.randint(-2, 3, (n, k), generator=g).float().to(F8)
    xs = torch.pow(2.0, torch.randint(-3, 2, (m, kb), generator=g).float())
    ws = torch.pow(2.0, torch.randint(-3, 2, ((n + 127) // 128, kb), generator=g).float())
    r, _ = ref(xq, xs, wq, ws)
    assert torch.equal(r.float().double(), r)
    return xq, xs, wq, ws, r.float().bfloat16()


def quant_weight(w):
    """w float [N, K] -> (e4m3 [N, K], f32 [ceil(N/128), K/128]): one scale = amax / 448 per 128 x 128 block (the last row
    block may be short), q = e4m3(w / scale)."""
    n, k = w.shape
    nb, kb = (n + 127) // 128, k // 128
    wp = torch.zeros(nb * 128, k, dtype=torch.float32)
    wp[:n] = w.float()
    blocks = wp.view(nb, 128, kb, 128)
    s = (blocks.abs().amax(dim=(1, 3)) / 448.0).clamp_min(1e-12)
    q = (blocks / s[:, None, :, None]).to(F8).view(nb * 128, k)[:n].contiguous()
    return q, s


@functools.lru_cache(maxsize=None)
def random_weight(n, k, seed=0):
    g = torch.Generator().manual_seed(seed * 1000003 + n * 31 + k + 17)
    return quant_weight(torch.randn(n, k, generator=g) * 0.05)


@functools.lru_cache(maxsize=None)
def random_inputs(m, n, k, seed=0):
    """(xq, xs, wq, ws, r, A): activations randn * 2^e with e in -6 .. 6 drawn per (row, block) and quantised by the statement of
    tests/blockwise_quant_ref.py - neighbouring blocks' scales differ by up to 2^12, so a wrong scale index cannot hide -;
    weights randn * 0.05 quantised per 128 x 128 block."""
    g = torch.Generator().manual_seed(seed * 1000003 + m * 7919 + n * 31 + k + 5)
    kb = k // 128
    e = torch.randint(-6, 7, (m, kb), generator=g).float()
    a = (torch.randn(m, kb, 128, generator=g) * torch.pow(2.0, e)[:, :, None]).view(m, k)
    xq, xs = blockwise_quant_ref.quant(a)
    wq, ws = random_weight(n, k, seed)
    r, big_a = ref(xq, xs, wq, ws)
    return xq, xs, wq, ws, r, big_a
