"""RoPE + QK-norm + paged KV store oracle — TEST INFRASTRUCTURE (see oracle/__init__.py).
Restates reference tests/test_rope.py:14-117 (generate_cos_sin_cache, apply_rms_norm_reference,
apply_rotary_pos_emb_neox_reference, rope_norm_ref) for CPU tensors."""
import torch


def generate_cos_sin_cache(max_position, head_dim, base=10000.0):
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2).float() / head_dim))
    freqs = torch.outer(torch.arange(max_position).float(), inv_freq)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1)


def rms_norm(x, weight, eps=1e-6):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * weight


def rotary_neox(x, cos_sin):
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    c, s = cos_sin[:, :h].unsqueeze(1), cos_sin[:, h:].unsqueeze(1)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rope_rows(num_seqlen_per_req, q_index, num_rows):
    """Per qkv row: its request and absolute position (int64 [num_rows] each), -1 for rows that belong to no request:
    rows past q_index[-1], and rows whose position would be negative (the length-0 requests of an align-8 padded decode
    batch own the padding rows)."""
    ns, qi = num_seqlen_per_req.long(), q_index.long()
    q_lens = qi[1:] - qi[:-1]
    req = torch.full((num_rows,), -1, dtype=torch.long)
    owned = min(int(qi[-1]), num_rows)
    req[:owned] = torch.repeat_interleave(torch.arange(len(q_lens)), q_lens)[:owned]
    r = req.clamp_min(0)
    pos = ns[r] - (qi[r + 1] - torch.arange(num_rows))
    gone = (req < 0) | (pos < 0)
    return req.masked_fill(gone, -1), pos.masked_fill(gone, -1)


def rope_norm_ref64(kcache, vcache, qkv, cos_sin, num_seqlen_per_req, q_index, kv_indices, q_norm_weight,
                    k_norm_weight, qk_norm_policy, eps=1e-6):
    """The op stated in float64, unrounded: from the bf16 qkv, the given fp32 cos_sin table and the fp32 norm weights.
    Same arguments as rope_norm_ref; the caches only give the head counts and are not written.  Returns
    (q64 [rows, Hq, 128], k64 [rows, Hkv, 128], row_req [rows], row_pos [rows]); rows of no request (rope_rows) are zero
    in q64 / k64.  V is a copy of qkv's V heads and is not returned.

    Where the K / V rows land, and which cache cells are cleared, is not stated here but by the cache-expectation helper
    of the tests (tests/rope_cases.py::cache_expectation), because the kernel's rule differs from rope_norm_ref's: the
    kernel zeroes the tail of a request's last page whenever seqlen > 0, rope_norm_ref only when the request has a new
    token in this call."""
    num_kv, qk_dim, v_dim = kcache.shape[2], kcache.shape[3], vcache.shape[3]
    num_q = (qkv.shape[1] - num_kv * qk_dim - num_kv * v_dim) // qk_dim
    rows = qkv.shape[0]
    req, pos = rope_rows(num_seqlen_per_req, q_index, rows)
    x = qkv.double()
    q = x[:, : num_q * qk_dim].view(rows, num_q, qk_dim)
    k = x[:, num_q * qk_dim : (num_q + num_kv) * qk_dim].view(rows, num_kv, qk_dim)
    h = qk_dim // 2
    cs = cos_sin.double()[pos.clamp_min(0)]
    cos, sin = cs[:, None, :h], cs[:, None, h:]

    # written out here, not through rms_norm / rotary_neox above: an error in those must not cancel against this statement
    def norm(t, w):
        return t / torch.sqrt((t * t).sum(-1, keepdim=True) / qk_dim + eps) * w.double()

    def rotate(t):  # neox pairing: element i turns with element i + 64
        a, b = t[..., :h], t[..., h:]
        return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)

    if qk_norm_policy == 2:
        q, k = norm(q, q_norm_weight), norm(k, k_norm_weight)
    q, k = rotate(q), rotate(k)
    if qk_norm_policy == 1:
        q, k = norm(q, q_norm_weight), norm(k, k_norm_weight)
    live = (req >= 0).view(rows, 1, 1)
    return q * live, k * live, req, pos


def rope_norm_ref(kcache, vcache, qkv, cos_sin, num_seqlen_per_req, q_index, kv_indices, q_norm_weight,
                  k_norm_weight, qk_norm_policy):
    """Updates kcache / vcache in place, returns q (reference tests/test_rope.py:47-117)."""
    dtype = qkv.dtype
    num_kv, v_dim, qk_dim, blk = kcache.shape[2], vcache.shape[3], kcache.shape[3], kcache.shape[1]
    num_q = (qkv.shape[1] - num_kv * qk_dim - num_kv * v_dim) // qk_dim
    num_req = num_seqlen_per_req.shape[0]
    q_lens = (q_index[1:] - q_index[:-1]).tolist()
    num_rows = int(q_index[-1])
    q = qkv[:, : num_q * qk_dim].float().view(num_rows, num_q, qk_dim)
    k = qkv[:, num_q * qk_dim : (num_q + num_kv) * qk_dim].float().view(num_rows, num_kv, qk_dim)
    v = qkv[:, (num_q + num_kv) * qk_dim :].view(num_rows, num_kv, v_dim)
    cs = torch.zeros(num_rows, qk_dim, dtype=torch.float32)
    off = 0
    for i in range(num_req):
        sl, ql = int(num_seqlen_per_req[i]), q_lens[i]
        if ql > 0:
            cs[off : off + ql] = cos_sin[sl - ql : sl]
        off += ql
    if qk_norm_policy == 2:
        q, k = rms_norm(q, q_norm_weight), rms_norm(k, k_norm_weight)
    q, k = rotary_neox(q, cs), rotary_neox(k, cs)
    if qk_norm_policy == 1:
        q, k = rms_norm(q, q_norm_weight), rms_norm(k, k_norm_weight)
    tok = 0
    for ri in range(num_req):
        sl, ql = int(num_seqlen_per_req[ri]), q_lens[ri]
        for pos in range(sl - ql, sl):
            bi, pb = pos // blk, pos % blk
            cb = int(kv_indices[ri, bi])
            kcache[cb, pb] = k[tok].to(dtype)
            vcache[cb, pb] = v[tok].to(dtype)
            if pos == sl - 1 and pb + 1 < blk:
                kcache[cb, pb + 1 :] = 0
                vcache[cb, pb + 1 :] = 0
            tok += 1
    return q.to(dtype)
