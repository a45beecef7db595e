"""The statement of the DSA lightning indexer (hpc.mla_indexer_store_k_fp8 / _logits_fp8 / _topk / _topk_fp8) in float64 PyTorch
(CPU), the knobs the bar tests turn to make mutants, the input generators the CPU and GPU tests share, and the eager-torch
indexer a caller would run without the ops.

The index-key cache: uint8, logically [num_blocks, P * 132].  Within a page the codes of its P tokens come first
([P, 128] float8_e4m3fn at byte 0), the P float32 scales follow at byte P * 128.  A column is fp32(code[d]) * scale.

    q            float8_e4m3fn [B * Sq, Hi, 128]     Sq = mtp + 1
    weights      float32 [B * Sq, Hi]
    block_ids    int32 [B, max_blocks]
    lens_total   int [B]                             L_b: tokens of request b INCLUDING the Sq new ones

    vis(b, s) = L_b - Sq + s + 1;  for 0 <= j < min(vis(b, s), max_blocks * P):
    logit[b*Sq+s, j] = kscale_b[j] * sum_h weights[b*Sq+s, h] * relu( sum_{d<128} q[b*Sq+s, h, d] * kcode_b[j, d] )
    a position whose page id lies outside [0, num_blocks) gets -inf; columns at or past the bound are not written (NaN here)

    top-k of row r over columns [0, n_r), n_r = clamp(vis, 0, columns): the min(topk, n_r) best positions under (torch_topk_key
    descending, position ascending), written in ascending position order, then -1."""
import torch

DIM, TOKEN_BYTES = 128, 132
F8 = torch.float8_e4m3fn


# ---- the cache ----------------------------------------------------------------------------------------------------------------
def pack(codes, scales):
    """codes float8_e4m3fn [num_blocks, P, 128], scales float32 [num_blocks, P] -> uint8 [num_blocks, P * 132]"""
    nb, P, _ = codes.shape
    cache = torch.empty(nb, P * TOKEN_BYTES, dtype=torch.uint8)
    cache[:, : P * DIM] = codes.contiguous().view(torch.uint8).reshape(nb, P * DIM)
    cache[:, P * DIM:] = scales.contiguous().view(torch.uint8).reshape(nb, P * 4)
    return cache


def unpack(cache):
    """uint8 [num_blocks, P * 132] -> (codes float8_e4m3fn [num_blocks, P, 128], scales float32 [num_blocks, P])"""
    nb, P = cache.shape[0], cache.shape[1] // TOKEN_BYTES
    codes = cache[:, : P * DIM].contiguous().view(F8).reshape(nb, P, DIM)
    scales = cache[:, P * DIM:].contiguous().view(torch.float32).reshape(nb, P)
    return codes, scales


def vis_of(lens_total, num_seq_q, b, s):
    return int(lens_total[b]) - num_seq_q + s + 1


# ---- logits -------------------------------------------------------------------------------------------------------------------
def logits_statement(q, weights, k_cache, block_ids, lens_total, num_seq_q, *, relu=True, weight_roll=0, scale_shift=0,
                     key_cols=DIM, vis_delta=0, translate=True, absolute=False):
    """float64 [B * Sq, max_blocks * P]; NaN marks a column the op does not write.  Mutations, all off by default: relu False
    drops the ReLU; weight_roll rotates the weights by that many heads; scale_shift takes the scale of token j + shift;
    key_cols < 128 drops the key columns from there on; vis_delta moves every row's bound; translate False takes j // P as the
    pool's page id.  absolute: the bound's A - absolute values everywhere and no ReLU."""
    codes, scales = unpack(k_cache)
    nb, P = codes.shape[0], codes.shape[1]
    sq, B = num_seq_q, len(lens_total)
    cols = block_ids.shape[1] * P
    out = torch.full((B * sq, cols), float("nan"), dtype=torch.float64)
    w = weights.double().roll(weight_roll, -1)
    for b in range(B):
        top = min(max(vis_of(lens_total, sq, b, sq - 1) + vis_delta, 0), cols)
        if top == 0:
            continue
        j = torch.arange(top)
        page = block_ids[b].long()[j // P] if translate else j // P
        ok = (page >= 0) & (page < nb)
        page = torch.where(ok, page, torch.zeros_like(page))
        k = codes[page, j % P].double()                       # [top, 128]
        ks = scales[page, j % P].double().roll(-scale_shift)  # [top]
        k[:, key_cols:] = 0
        for s in range(sq):
            r = b * sq + s
            n = min(max(vis_of(lens_total, sq, b, s) + vis_delta, 0), cols)
            qr = q[r].double()
            if absolute:
                d = qr.abs() @ k[:n].abs().T                  # [Hi, n]
                v = ks[:n].abs() * (w[r].abs()[:, None] * d).sum(0)
            else:
                d = qr @ k[:n].T
                v = ks[:n] * (w[r][:, None] * (d.clamp_min(0) if relu else d)).sum(0)
                v = torch.where(ok[:n], v, torch.full_like(v, float("-inf")))
            out[r, :n] = v
    return out


def same_written(a, b):
    """do two logits tensors mark the same columns as written?"""
    return torch.equal(a.isnan(), b.isnan())


def equal_where_written(got, want):
    """the op's float32 result against a statement's float64 one: the same columns written, the same values there"""
    g, w = got.double().cpu(), want.to(torch.float32).double()
    return same_written(g, w) and torch.equal(g[~w.isnan()], w[~w.isnan()])


def worst_ratio(got, want, A):
    """max over written, finite columns of |got - want| / (2^-24 * A) (0 / 0 counts as 0); inf where the written sets, or the
    -inf positions, differ"""
    g, w = got.double().cpu(), want
    if not same_written(g, w) or not torch.equal(g == float("-inf"), w == float("-inf")):
        return float("inf")
    m = torch.isfinite(w)
    err, bound = (g[m] - w[m]).abs(), 2.0 ** -24 * A[m]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- top-k --------------------------------------------------------------------------------------------------------------------
def topk_key(x):
    """csrc/ordered_key.h::torch_topk_key of float32 values, as int64: -0.0 == +0.0, every NaN above +inf, monotonic otherwise"""
    x = x.float() + 0.0
    bits = x.contiguous().view(torch.int32).long() & 0xFFFFFFFF
    bits = torch.where(x.isnan(), torch.full_like(bits, 0x7FC00000), bits)
    return torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits | 0x80000000)


def topk_statement(logits, lens_total, num_seq_q, topk, *, ties_larger=False, score_order=False, vis_delta=0):
    """int32 [rows, topk].  Mutations: ties_larger gives a tie to the larger position; score_order leaves the list in score
    order; vis_delta moves every row's bound."""
    rows, cols = logits.shape
    out = torch.full((rows, topk), -1, dtype=torch.int32)
    for r in range(rows):
        b, s = divmod(r, num_seq_q)
        n = min(max(vis_of(lens_total, num_seq_q, b, s) + vis_delta, 0), cols)
        if n <= topk:
            out[r, :n] = torch.arange(n, dtype=torch.int32)
            continue
        key = topk_key(logits[r, :n])
        if ties_larger:
            order = (n - 1) - torch.sort(key.flip(0), descending=True, stable=True)[1]
        else:
            order = torch.sort(key, descending=True, stable=True)[1]
        take = order[:topk]
        out[r] = (take if score_order else torch.sort(take)[0]).to(torch.int32)
    return out


# ---- inputs the CPU and GPU tests share ---------------------------------------------------------------------------------------
CONTEXTS = [1, 15, 16, 17, 63, 64, 65, 300, 2100, 5000]          # L_b
CONFIGS = [(64, 0, 64), (16, 1, 16), (32, 3, 128), (64, 3, 32)]  # (Hi, mtp, P)
POISONED = 1 << 20                                                # a page id outside every pool here


def _pages(lens_total, P, gen, poison):
    """block_ids with one column past the longest request, -1 where a request has no page, and (poison) one page id per
    request outside the pool; (block_ids, pool size, the poisoned (request, slot) pairs)"""
    nblocks = [-(-max(L, 0) // P) for L in lens_total]
    used = sum(nblocks)
    pool = used + 3
    perm = torch.randperm(pool, generator=gen).to(torch.int32)
    block_ids = torch.full((len(lens_total), max(nblocks) + 1), -1, dtype=torch.int32)
    off, dead = 0, []
    for b, nb in enumerate(nblocks):
        block_ids[b, :nb] = perm[off: off + nb]
        off += nb
        if poison and nb:
            slot = int(torch.randint(0, nb, (1,), generator=gen))
            block_ids[b, slot] = POISONED if b % 2 else -7
            dead.append((b, slot))
    return block_ids, pool, dead


def inputs(Hi, mtp, P, *, exact, lens_total=CONTEXTS, seed=0, poison=True):
    """exact: q and key codes integer-valued in [-8, 8], weights integers in [-8, 8], scales powers of two - every partial sum
    an integer below 2^24, so the float32 result is the statement's whatever the order of the sums.  Otherwise random e4m3
    codes (no NaN code), scales in [2^-6, 2^-2], signed normal weights."""
    gen = torch.Generator().manual_seed(seed + 1000 * Hi + 10 * mtp + P)
    sq, B = mtp + 1, len(lens_total)
    block_ids, pool, dead = _pages(lens_total, P, gen, poison)
    if exact:
        codes = torch.randint(-8, 9, (pool, P, DIM), generator=gen).float().to(F8)
        scales = torch.exp2(torch.randint(-6, -1, (pool, P), generator=gen).float())
        q = torch.randint(-8, 9, (B * sq, Hi, DIM), generator=gen).float().to(F8)
        weights = torch.randint(-8, 9, (B * sq, Hi), generator=gen).float()
    else:
        def random_codes(*shape):
            raw = torch.randint(0, 256, shape, generator=gen, dtype=torch.int32)
            raw[(raw & 0x7F) == 0x7F] = 0x38  # the two NaN codes -> 1.0
            return raw.to(torch.uint8).view(F8)
        codes, q = random_codes(pool, P, DIM), random_codes(B * sq, Hi, DIM)
        scales = torch.exp2(-6 + 4 * torch.rand(pool, P, generator=gen))
        weights = torch.randn(B * sq, Hi, generator=gen)
    return dict(q=q, weights=weights, k_cache=pack(codes, scales), block_ids=block_ids,
                lens_total=torch.tensor(lens_total, dtype=torch.int32), num_seq_q=sq, P=P, Hi=Hi, dead=dead)


def statement(inp, **mutation):
    return logits_statement(inp["q"], inp["weights"], inp["k_cache"], inp["block_ids"], inp["lens_total"], inp["num_seq_q"],
                            **mutation)


# the mutants of plausible bugs the logits bar must reject
LOGITS_MUTANTS = {
    "no ReLU": dict(relu=False),
    "weights rotated by one head": dict(weight_roll=1),
    "the scale of token j + 1": dict(scale_shift=1),
    "key columns 64.. dropped": dict(key_cols=64),
    "vis off by one": dict(vis_delta=1),
    "page id taken as j // P untranslated": dict(translate=False),
}
TOPK_MUTANTS = {
    "ties to the larger position": dict(ties_larger=True),
    "output in score order": dict(score_order=True),
    "vis off by one": dict(vis_delta=-1),
}


# ---- what a caller runs without the ops ----------------------------------------------------------------------------------------
def indexer_eager(q, weights, k_cache, block_ids, lens_total, num_seq_q, topk):
    """The indexer in eager torch on q's device: a gather of the index keys through the page table, a [T, Hi, L] einsum, ReLU
    and a weighted head sum, a mask from the lengths and torch.topk, then a sort into ascending position order.  lens_total: an
    int tensor on q's device.  int64 [T, min(topk, columns)] with -1 where a row sees fewer tokens."""
    sq, P = num_seq_q, k_cache.shape[1] // TOKEN_BYTES
    nb, R = k_cache.shape[0], q.shape[0]
    B, cols = block_ids.shape[0], block_ids.shape[1] * P
    codes = k_cache[:, : P * DIM].view(F8).reshape(nb, P, DIM)
    scales = k_cache[:, P * DIM:].view(torch.float32).reshape(nb, P)
    page = block_ids.long()
    ok = (page >= 0) & (page < nb)
    page = torch.where(ok, page, torch.zeros_like(page))
    k = codes[page].reshape(B, cols, DIM).to(torch.bfloat16)               # exact: e4m3 fits bf16
    ks = scales[page].reshape(B, cols)
    d = torch.einsum("bshd,bjd->bshj", q.to(torch.bfloat16).view(B, sq, -1, DIM), k).float()
    logit = (d.relu() * weights.view(B, sq, -1, 1)).sum(2) * ks[:, None, :]  # [B, sq, cols]
    logit = logit.masked_fill(~ok.repeat_interleave(P, 1)[:, None, :], float("-inf"))
    vis = lens_total.long()[:, None] - sq + torch.arange(sq, device=q.device)[None, :] + 1
    seen = torch.arange(cols, device=q.device)[None, None, :] < vis[:, :, None]
    kk = min(topk, cols)
    val, idx = logit.masked_fill(~seen, float("-inf")).view(R, cols).topk(kk, dim=-1)
    idx = torch.where(seen.view(R, cols).gather(1, idx), idx, torch.full_like(idx, cols + 1))
    idx = idx.sort(-1)[0]
    return torch.where(idx > cols, torch.full_like(idx, -1), idx)
