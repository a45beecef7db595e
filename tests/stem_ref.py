"""CPU restatement of the Stem mask pipeline (hpc.stem) for the tests: vectorised PyTorch, float64 where the kernels
accumulate in float32, so that the tests can bound the kernels' rounding; the TPD stage is exact (integer order keys,
float32 budget arithmetic one operation at a time).

S = 128 (stem block), R = 16 (stride: groups), 8 samples per group, D = 128.  Kb_r = ceil(kv_len / S),
Qb_r = ceil(q_len / S), off = (kv_len - q_len + S - 1) / S with C (truncating) division."""
import torch

S, R, N, D = 128, 16, 8, 128


def cdiv(a, b):
    return (a + b - 1) // b


def c_div(a, b):
    """C integer division (truncates towards zero) of an int tensor by a positive int."""
    return torch.div(a, b, rounding_mode="trunc")


def _group_sums(x):
    """x [T_pad, H, D] (T_pad multiple of S) -> [H, blocks, 16 groups, D]: group g of block b sums tokens b S + g + s R."""
    t, h, d = x.shape
    return x.reshape(t // S, N, R, h, d).sum(1).permute(2, 0, 1, 3)


def _gather_pages(cache, ids, L):
    """cache [pages, P, H, D] fp8 -> float64 [L, H, D] of one request."""
    P = cache.shape[1]
    return cache[ids[: cdiv(L, P)].long()].double().reshape(-1, cache.shape[2], cache.shape[3])[:L]


def kscale_per_token(kscale, ids, L, P):
    """Per-token K scale of one request -> float64 [L, Hkv]: fp32 at [page, r // 32, head, r % 32] (the fp8 view of the
    cache's tail rows is reinterpreted as that float32 layout)."""
    ks = kscale if kscale.dtype == torch.float32 else kscale.contiguous().view(torch.float32)
    ks = ks[ids[: cdiv(L, P)].long()].double()  # [n, P/32, Hkv, 32]
    return ks.permute(0, 1, 3, 2).reshape(-1, ks.shape[2])[:L]


def prep_paged_kv(kcache, vcache, kscale, vscale, kv_indices, kv_seq_lens, lambda_mag=0.3, quant_type=1):
    """-> kflat float64 [B, Hkv, max_Kb, 2048] (not rounded), vbias float64 [B, Hkv, max_Kb]."""
    B, hkv, P = kv_seq_lens.numel(), kcache.shape[2], kcache.shape[1]
    lens = [int(x) for x in kv_seq_lens]
    max_kb = cdiv(max(lens), S) if B else 0
    kflat = torch.zeros(B, hkv, max_kb, R * D, dtype=torch.float64)
    vbias = torch.zeros(B, hkv, max_kb, dtype=torch.float64)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        kb, ids = cdiv(L, S), kv_indices[b]
        k = _gather_pages(kcache, ids, L)
        v = _gather_pages(vcache, ids, L)
        if quant_type == 1:
            k = k * float(kscale.reshape(-1)[0])
            vs = torch.full((hkv,), float(vscale.reshape(-1)[0]), dtype=torch.float64)
        else:
            k = k * kscale_per_token(kscale, ids, L, P)[:, :, None]
            vs = vscale[:hkv].double()
        kp = torch.zeros(kb * S, hkv, D, dtype=torch.float64)
        kp[:L] = k
        kflat[b, :, :kb] = _group_sums(kp).flip(2).reshape(hkv, kb, R * D)
        norms = torch.zeros(kb * S, hkv, dtype=torch.float64)
        norms[:L] = (v * vs[None, :, None]).norm(dim=-1)
        vnorm = norms.reshape(kb * N, R, hkv).amax(1).t()  # [Hkv, Kb*8]
        lg = torch.log(vnorm + 1e-6)
        mu = lg.mean(1, keepdim=True)
        sd = lg.std(1, keepdim=True) if lg.shape[1] > 1 else torch.zeros_like(mu)
        z = torch.relu((lg - mu) / (sd + 1e-6))
        vbias[b, :, :kb] = (lambda_mag * z).reshape(hkv, kb, N).mean(-1)
    return kflat, vbias


def prep_varlen_q(q_fp8, qscale, q_seq_lens, cu_seqlens_q):
    """-> qflat float64 [B, Hq, max_Qb, 2048] (not rounded)."""
    B, hq = q_seq_lens.numel(), q_fp8.shape[1]
    lens = [int(x) for x in q_seq_lens]
    max_qb = cdiv(max(lens), S) if B else 0
    qflat = torch.zeros(B, hq, max_qb, R * D, dtype=torch.float64)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        qb, a0 = cdiv(L, S), int(cu_seqlens_q[b])
        q = q_fp8[a0:a0 + L].double() * qscale[b, :, :L].t().double()[:, :, None]
        qp = torch.zeros(qb * S, hq, D, dtype=torch.float64)
        qp[:L] = q
        qflat[b, :, :qb] = _group_sums(qp).reshape(hq, qb, R * D)
    return qflat


def valid_mask(q_seq_lens, kv_seq_lens, max_qb, max_kb, causal=True):
    """bool [B, 1, max_Qb, max_Kb]: where oam_gemm writes a finite logit."""
    ql, kl = q_seq_lens.long(), kv_seq_lens.long()
    nqb, nkb = cdiv(ql, S), cdiv(kl, S)
    off = c_div(kl - ql + S - 1, S)
    r = torch.arange(max_qb)[None, :, None]
    c = torch.arange(max_kb)[None, None, :]
    ok = (r < nqb[:, None, None]) & (c < nkb[:, None, None])
    if causal:
        ok &= ~(r + off[:, None, None] < c)
    return ok[:, None]


def oam_gemm(qflat, kflat, vbias, q_seq_lens, kv_seq_lens, causal=True):
    """float64 logits [B, Hq, max_Qb, max_Kb] from the given (bf16 or float) inputs, -inf where masked."""
    hq, hkv = qflat.shape[1], kflat.shape[1]
    g = hq // hkv
    kf = kflat.double().repeat_interleave(g, dim=1)
    lg = torch.matmul(qflat.double(), kf.transpose(-1, -2)) / 64.0 + vbias.double().repeat_interleave(g, dim=1)[:, :, None, :]
    ok = valid_mask(q_seq_lens, kv_seq_lens, qflat.shape[2], kflat.shape[2], causal)
    return lg.masked_fill(~ok, float("-inf"))


# ---- TPD ------------------------------------------------------------------------------------------------------------
def order_keys(logits_bf16):
    """bf16 -> int32 order key in [0, 0xffff]: bits ^ 0x8000 (sign clear), ~bits (sign set); non-finite -> 0x7f."""
    bits = logits_bf16.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    key = torch.where(bits & 0x8000 != 0, (~bits) & 0xFFFF, bits ^ 0x8000)
    return torch.where((bits & 0x7F80) == 0x7F80, torch.full_like(key, 0x7F), key)


def budgets(q_seq_lens, kv_seq_lens, num_prompt_tokens, max_qb, block_size=128, alpha=1.0, rate_medium=0.2,
            bias_medium=30, rate_large=0.1, bias_large=30):
    """int64 [B, max_Qb] per-row budgets, float32 arithmetic one operation at a time."""
    f32 = torch.float32
    P = cdiv(num_prompt_tokens.long(), block_size)
    km = (P.to(f32) * torch.tensor(rate_medium, dtype=f32)).long() + bias_medium  # float -> int truncates (P >= 0)
    kl = (P.to(f32) * torch.tensor(rate_large, dtype=f32)).long() + bias_large
    k = torch.where(P < 56, P, torch.where(P < 160, km, kl))[:, None]
    off = c_div(kv_seq_lens.long() - q_seq_lens.long() + block_size - 1, block_size)
    q_pos = torch.arange(max_qb)[None, :] + off[:, None]
    decay = (P[:, None] - k)
    kf = k.to(f32)
    k_end = kf * torch.tensor(alpha, dtype=f32)
    t = (q_pos - k).to(f32) / (decay - 1).to(f32)
    v = kf + t * (k_end - kf)
    dec = torch.floor(v).long().clamp(min=1)
    dec = torch.minimum(dec, k.expand_as(dec))
    return torch.where((q_pos < k) | (decay <= 1), k.expand_as(dec), dec)


def thresholds(keys, budget):
    """Exact threshold per row by a 16-round bitwise search: the largest T with #{key >= T} >= budget, or 0x80 (every
    finite key) when budget >= #finite.  keys int32 [..., n] (invalid columns 0), budget int64 [...]."""
    nfin = (keys >= 0x80).sum(-1)
    T = torch.zeros(keys.shape[:-1], dtype=torch.int32)
    for bit in range(15, -1, -1):
        cand = T | (1 << bit)
        cnt = (keys >= cand[..., None]).sum(-1)
        T = torch.where(cnt >= budget, cand, T)
    return torch.where(budget >= nfin, torch.full_like(T, 0x80), T)


def tpd(block_logits, q_seq_lens, kv_seq_lens, num_prompt_tokens, block_size=128, alpha=1.0, initial_blocks=4,
        window_size=4, k_block_num_rate_medium=0.2, k_block_num_bias_medium=30, k_block_num_rate_large=0.1,
        k_block_num_bias_large=30, return_threshold=False):
    """uint8 mask [B, H, max_Qb, max_Kb] (and the int32 thresholds [B, H, max_Qb] when asked)."""
    B, H, max_qb, max_kb = block_logits.shape
    nqb = cdiv(q_seq_lens.long(), block_size)
    nkb = torch.clamp(cdiv(kv_seq_lens.long(), block_size), max=max_kb)
    col = torch.arange(max_kb)
    colv = col[None, :] < nkb[:, None]  # [B, Kb]
    keys = torch.where(colv[:, None, None, :], order_keys(block_logits), torch.zeros((), dtype=torch.int32))
    bud = budgets(q_seq_lens, kv_seq_lens, num_prompt_tokens, max_qb, block_size, alpha, k_block_num_rate_medium,
                  k_block_num_bias_medium, k_block_num_rate_large, k_block_num_bias_large)
    T = thresholds(keys, bud[:, None, :].expand(B, H, max_qb))
    off = c_div(kv_seq_lens.long() - q_seq_lens.long() + block_size - 1, block_size)
    diag = torch.minimum(torch.arange(max_qb)[None, :] + off[:, None], nkb[:, None] - 1)[:, None, :, None]
    c = col[None, None, None, :]
    sel = (keys >= T[..., None]) | (c < initial_blocks) | ((c > diag - window_size) & (c <= diag)) | (c == diag)
    rowv = (torch.arange(max_qb)[None, :] < nqb[:, None])[:, None, :, None]
    mask = (sel & colv[:, None, None, :] & rowv).to(torch.uint8)
    return (mask, T) if return_threshold else mask


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (float64)."""
    a = x.abs().double().clamp(min=2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)
