"""The PyTorch statement of hpc.speculative_verify (no reference kernel exists) and the input generator of its tests.

Acceptance probabilities are float64 (fp32 torch softmax is already 4e-5 off at V = 131080); tokens are computed the way
oracle.sampler.ref_temperature_sample computes them - fp32 logits / T + gumbel, then arg-max - so they are comparable bit
for bit with the kernel, which evaluates the same expression."""
import math

import torch

from oracle.sampler import ref_temperature_sample

P_BAR = 1e-3  # relative bar on p = softmax(logits / T)[draft]: no input may put a uniform closer to its p than this


def num_valid(draft, V):
    """n_b: the number of leading entries in [0, V) of every row of draft [B, K]."""
    ok = ((draft >= 0) & (draft < V)).to(torch.int64)
    return ok.cumprod(dim=1).sum(dim=1)


def draft_probs(logits, draft, temperature):
    """float64 [B, K]: softmax(logits[r] / T)[draft] for the positions j < n_b of requests with T > 0, NaN elsewhere."""
    B, K = draft.shape
    V = logits.shape[1]
    T = torch.as_tensor(temperature, dtype=torch.float32).expand(B)
    n = num_valid(draft, V)
    p = torch.full((B, K), float("nan"), dtype=torch.float64)
    for b in range(B):
        if not T[b] > 0:
            continue
        for j in range(int(n[b])):
            r = b * (K + 1) + j
            p[b, j] = torch.softmax(logits[r].double() / T[b].double(), -1)[draft[b, j]]
    return p


def ref_speculative_verify(logits, draft, temperature, uniform, gumbel):
    """logits [B * (K + 1), V] float32 / bfloat16, draft int64 [B, K], temperature scalar or float32 [B], uniform float32
    [B, K], gumbel float32 [B * (K + 1), V]; CPU tensors.  Returns (output_token_ids int32 [B, K + 1], num_accepted int32
    [B], p float64 [B, K])."""
    B, K = draft.shape
    R, V = logits.shape
    assert R == B * (K + 1)
    T = torch.as_tensor(temperature, dtype=torch.float32).expand(B).contiguous()
    n = num_valid(draft, V)
    p = draft_probs(logits, draft, T)
    out = torch.full((B, K + 1), -1, dtype=torch.int32)
    acc = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        greedy = not T[b] > 0
        j = 0
        while True:
            r = b * (K + 1) + j
            row = logits[r : r + 1]
            if j < int(n[b]):
                d = int(draft[b, j])
                if greedy:
                    accept = d == int(row.float().argmax(-1))
                else:
                    accept = bool(uniform[b, j].double() < p[b, j])
                if accept:
                    out[b, j] = d
                    j += 1
                    continue
                mask = draft[b, j : j + 1]
            else:
                mask = None
            if greedy:
                out[b, j] = int(row.float().argmax(-1))
            else:
                out[b, j] = int(ref_temperature_sample(row, T[b : b + 1], gumbel[r : r + 1], mask))
            acc[b] = j
            break
    return out, acc, p


def gumbel_like(shape, generator):
    u = torch.rand(shape, generator=generator).clamp_min(1e-20)
    return -torch.log((-torch.log(u)).clamp_min(1e-20))


def make_case(V, B, K, seed, dtype, temperature=None, draft=None, lift=True):
    """randn logits; every valid leading draft's logit is lifted so that its p lands at a target drawn in (0.2, 0.95);
    T drawn in 0.3-1.8 per request unless given (scalar or [B]).  Returns a dict of CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    R = B * (K + 1)
    logits = torch.randn(R, V, generator=g)
    drawn = torch.randint(0, V, (B, K), generator=g)
    draft = drawn if draft is None else draft.clone()
    T = torch.rand(B, generator=g) * 1.5 + 0.3
    if temperature is not None:
        T = torch.as_tensor(temperature, dtype=torch.float32).expand(B).contiguous()
    want = torch.rand(B, K, generator=g) * 0.75 + 0.2
    n = num_valid(draft, V)
    if lift:
        for b in range(B):
            if not T[b] > 0:
                continue
            for j in range(int(n[b])):
                r, d = b * (K + 1) + j, draft[b, j]
                x = logits[r].double() / T[b].double()
                x[d] = -1e30
                w = want[b, j].double()
                logits[r, d] = ((torch.logsumexp(x, 0) + math.log(w / (1 - w))) * T[b].double()).float()
    logits = logits.to(dtype)
    u = torch.rand(B, K, generator=g)
    gum = gumbel_like((R, V), g)
    return dict(logits=logits, draft=draft, T=T, u=u, gumbel=gum, n=n)


def assert_decidable(p, u):
    """In float64, on the inputs alone: no live position has its uniform within P_BAR (relative) of its p, so a kernel
    whose p is within P_BAR decides every position as the reference does."""
    live = ~torch.isnan(p)
    margin = ((u.double() - p).abs() / p)[live]
    assert margin.numel() == 0 or float(margin.min()) > P_BAR, float(margin.min())
