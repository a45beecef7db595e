"""The PyTorch statement of hpc.token_logprobs (no reference kernel exists), the input generators of its tests, the check
they share, and a CPU model of the op's two phases that takes planted errors.

The statement: y = x / T (x when T == 0) is formed in float32, which is the kernel's own expression bit for bit; the
log-probabilities are formed from y in float64; ranks and top ids come from the stable descending sort of x.float()."""
import math

import numpy as np
import torch

UNIT = 2.0 ** -24  # a logprob passes when |got - lp64| <= C_BAR * UNIT * (1 + |lp64|)


def row_temperature(temperature, R):
    """float32 [R]: a scalar for every row, or entry r // (R / C) of a tensor of C elements."""
    if not isinstance(temperature, torch.Tensor):
        return torch.full((R,), float(temperature), dtype=torch.float32)
    t = temperature.detach().cpu().float().flatten()
    assert t.numel() >= 1 and R % t.numel() == 0
    return t.repeat_interleave(R // t.numel())


def scaled(logits, temperature):
    """y float32 [R, V], formed as the kernel forms it."""
    x = logits.float()
    T = row_temperature(temperature, x.shape[0]).view(-1, 1)
    return torch.where(T > 0, x / torch.where(T > 0, T, torch.ones_like(T)), x)


def ref_token_logprobs(logits, token_ids, temperature, num_top):
    """logits [R, V] float32 / bfloat16, token_ids R integers in any shape, temperature scalar or float32 tensor; CPU
    tensors.  Returns (token_logprobs float64 [R], token_ranks int32 [R], top_ids int32 [R, num_top], top_logprobs float64
    [R, num_top]); a row whose token is outside [0, V) gives 0.0, 0, -1 ..., 0.0 ... and is not looked at."""
    R, V = logits.shape
    tok = token_ids.reshape(-1).to(torch.int64)
    assert tok.numel() == R
    live = (tok >= 0) & (tok < V)
    x = logits.float()
    x = torch.where(live.view(-1, 1), x, torch.zeros_like(x))  # a dead row's logits are not looked at
    y = scaled(x, temperature).double()
    logp = y - torch.logsumexp(y, dim=-1, keepdim=True)
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices
    place = torch.empty_like(order)
    place.scatter_(1, order, torch.arange(V).expand(R, V).contiguous())
    t = tok.clamp(0, V - 1).view(-1, 1)
    lp = torch.where(live, logp.gather(1, t).flatten(), torch.zeros(R, dtype=torch.float64))
    rank = torch.where(live, place.gather(1, t).flatten() + 1, torch.zeros(R, dtype=torch.int64)).to(torch.int32)
    ids = order[:, :num_top]
    top_lp = torch.where(live.view(-1, 1), logp.gather(1, ids), torch.zeros(R, num_top, dtype=torch.float64))
    ids = torch.where(live.view(-1, 1), ids, torch.full_like(ids, -1)).to(torch.int32)
    return lp, rank, ids, top_lp


def units(got, want64):
    """The error of float32 `got` against float64 `want64` in units of 2^-24 (1 + |want|); an exact -inf must come back
    as -inf, anything else non-finite is an infinite error."""
    got, want64 = got.double().flatten(), want64.flatten()
    if got.numel() == 0:
        return 0.0
    ninf = want64 == -math.inf
    err = (got - want64).abs() / (UNIT * (1 + want64.abs()))
    err = torch.where(ninf, torch.where(got == -math.inf, 0.0, math.inf), err)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    return float(err.max())


def check(got, ref, token_ids, num_top, c_bar):
    """Everything the statement says about one call: got = (token_logprobs, token_ranks, top_ids, top_logprobs) of the op or
    of the model, CPU tensors; ref = ref_token_logprobs(..., num_top >= this num_top).  Equalities are asserted, the worst
    logprob error in units is returned after it has been held to c_bar."""
    lp, rank, ids, tlp = got
    rlp, rrank, rids, rtlp = ref
    R = rlp.numel()
    assert (lp.dtype, rank.dtype, ids.dtype, tlp.dtype) == (torch.float32, torch.int32, torch.int32, torch.float32)
    assert lp.shape == (R,) and rank.shape == (R,) and ids.shape == (R, num_top) and tlp.shape == (R, num_top)
    rids, rtlp = rids[:, :num_top], rtlp[:, :num_top]
    assert torch.equal(rank, rrank), (rank.tolist()[:8], rrank.tolist()[:8])
    assert torch.equal(ids, rids), (ids.tolist()[:2], rids.tolist()[:2])
    dead = rrank == 0
    if bool(dead.any()):
        assert torch.equal(lp[dead], torch.zeros(int(dead.sum()))) and torch.equal(tlp[dead], torch.zeros(int(dead.sum()), num_top))
    worst = max(units(lp, rlp), units(tlp, rtlp))
    assert worst <= c_bar, worst
    # the top list's slot of the token: the same id and the same bits
    sel = ~dead & (rank <= num_top)
    if bool(sel.any()):
        tok = token_ids.reshape(-1).to(torch.int64)[sel]
        k = (rank[sel].to(torch.int64) - 1).view(-1, 1)
        assert torch.equal(ids[sel].gather(1, k).flatten().to(torch.int64), tok)
        assert torch.equal(tlp[sel].gather(1, k).flatten().view(torch.int32), lp[sel].view(torch.int32))
    return worst


# ---- generators -------------------------------------------------------------------------------------------------------------
def make_case(V, R, seed, dtype, scale=1.0, temperature=None, tensor_count=None):
    """randn * scale logits; T drawn in 0.3-1.8, a scalar unless tensor_count is given (then that many entries); tokens:
    even rows one of the row's 40 most likely (on both sides of every num_top), odd rows any token.  CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(R, V, generator=g) * scale).to(dtype)
    if temperature is None:
        n = 1 if tensor_count is None else tensor_count
        temperature = torch.rand(n, generator=g) * 1.5 + 0.3
        if tensor_count is None:
            temperature = float(temperature[0])
    order = torch.topk(logits.float(), min(40, V), dim=-1).indices
    tok = torch.randint(0, V, (R,), generator=g)
    near = order.gather(1, torch.randint(0, min(40, V), (R, 1), generator=g)).flatten()
    tok = torch.where(torch.arange(R) % 2 == 0, near, tok)
    return dict(logits=logits, tok=tok, T=temperature)


def segments_of(V):
    return max(16, -(-V // 8192))


def segment_size(V):
    return -(-V // segments_of(V))


# ---- a CPU model of the two phases, with planted errors ----------------------------------------------------------------------
def _keys(x, canonical_zero=True):
    """torch_topk_key of float32 x as uint64: the order of the floats with -0.0 == +0.0 (unless canonical_zero is off)."""
    x = np.asarray(x, dtype=np.float32)
    if canonical_zero:
        x = x + np.float32(0.0)
    u = x.view(np.uint32).astype(np.uint64)
    return np.where(u & np.uint64(0x80000000), (~u) & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))


PLANTS = ("drop_segment", "drop_last", "no_temperature", "max_as_logsum", "ties_to_larger", "negzero_below", "rank_zero_based")


def two_phase_model(logits, token_ids, temperature, num_top, plant=None):
    """What the kernels do, in float32 on the CPU: per segment the (max, sum exp) of y, the count of composites above the
    token's and the segment's top num_top composites; per row the fold of the statistics, the sum of the counts, the top
    num_top of the candidates and (y - m) - log(sum).  plant: one of PLANTS."""
    assert plant is None or plant in PLANTS
    R, V = logits.shape
    S, seg = segments_of(V), segment_size(V)
    tok = token_ids.reshape(-1).to(torch.int64).tolist()
    T = row_temperature(temperature, R).numpy()
    X = logits.float().numpy()
    lp = torch.zeros(R, dtype=torch.float32)
    rank = torch.zeros(R, dtype=torch.int32)
    ids = torch.full((R, num_top), -1, dtype=torch.int32)
    tlp = torch.zeros(R, num_top, dtype=torch.float32)
    f32 = np.float32
    for r in range(R):
        t = tok[r]
        if t < 0 or t >= V:
            continue
        x = X[r]
        n = V - 1 if plant == "drop_last" else V
        temp = f32(1.0) if plant == "no_temperature" or not T[r] > 0 else T[r]
        key = _keys(x, canonical_zero=plant != "negzero_below")
        idx = np.arange(V, dtype=np.uint64)
        comp = (key << np.uint64(20)) | (idx if plant == "ties_to_larger" else np.uint64(0xFFFFF) - idx)
        value = lambda i: (x[i] + f32(0.0)) / temp  # noqa: E731  (the value decoded from the key, scaled)
        m, total, above, cand = f32(-np.inf), f32(0.0), 0, []
        for s in range(S):
            i0, i1 = s * seg, min(n, (s + 1) * seg)
            if i0 >= i1:
                continue
            above += int((comp[i0:i1] > comp[t]).sum())
            cand.append(np.sort(comp[i0:i1])[::-1][:num_top])
            if plant == "drop_segment" and s == 1:
                continue
            y = (x[i0:i1] / temp).astype(f32)
            m2 = y.max()
            s2 = np.exp(y - (f32(0.0) if m2 == -np.inf else m2), dtype=f32).sum(dtype=f32)
            mx = max(m, m2)
            sub = f32(0.0) if mx == -np.inf else mx
            total = f32(total * np.exp(m - sub, dtype=f32) + s2 * np.exp(m2 - sub, dtype=f32))
            m = mx
        log_sum = f32(0.0) if plant == "max_as_logsum" else np.log(total, dtype=f32)
        lp[r] = float(f32(f32(value(t) - m) - log_sum))
        rank[r] = above + (0 if plant == "rank_zero_based" else 1)
        if num_top:
            win = np.sort(np.concatenate(cand))[::-1][:num_top]
            win_ids = (win & np.uint64(0xFFFFF)) if plant == "ties_to_larger" else np.uint64(0xFFFFF) - (win & np.uint64(0xFFFFF))
            win_ids = win_ids.astype(np.int64)
            ids[r] = torch.from_numpy(win_ids.astype(np.int32))
            tlp[r] = torch.from_numpy(((value(win_ids) - m).astype(f32) - log_sum).astype(f32))
    return lp, rank, ids, tlp
