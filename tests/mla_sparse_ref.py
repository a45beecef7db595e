"""The statement of hpc.attention_decode_mla_sparse_bf16 / _fp8 in float64 PyTorch (CPU), and the knobs the bar tests turn to
make mutants.  The dense statement is tests/mla_ref.py; the FP8 op is this statement on the dequantised cache (tests/mla_fp8_ref.py).

    q            bf16 [B * Sq, H, 576]      Sq = mtp + 1
    ckv_cache    bf16 logical [num_blocks, P, 576]
    block_ids    int32 [B, max_blocks]
    lens_total   int [B]                    L_b: tokens of request b INCLUDING the Sq new ones
    indices      int32 [B * Sq, topk]       row b * Sq + s: LOGICAL token positions of request b, shared by all H heads

    vis(b, s) = L_b - Sq + s + 1
    entry k of row (b, s) is valid when 0 <= idx_k < vis(b, s), idx_k // P < max_blocks and block_ids[b, idx_k // P] lies in
    [0, num_blocks); every other entry contributes nothing
    z_k   = softmax_scale * sum_{d < 576} q[b*Sq+s, h, d] * c_b[idx_k, d]          over valid k
    out[b*Sq+s, h, :] = sum_k softmax(z)_k * c_b[idx_k, :512]                       (a position listed twice counts twice)
    lse[b*Sq+s, h]    = log sum_k exp(z_k)
    a row without a valid entry: out = 0, lse = -inf

Both come back in float64 (round `out` with .to(torch.bfloat16) to compare with the op)."""
import torch

DIM, DIM_V = 576, 512


def vis_of(lens_total, num_seq_q, b, s):
    return int(lens_total[b]) - num_seq_q + s + 1


def gather_list(ckv_cache, block_ids_row, idx, vis, *, mask_vis=True, neg_as_zero=False, translate=True):
    """(rows float64 [topk, 576] with zeros where the entry is invalid, valid bool [topk]) of one list.  The mutations, all off
    by default: mask_vis False admits positions at or past vis; neg_as_zero reads a negative entry as token 0; translate False
    takes idx // P as the pool's page id."""
    num_blocks, P = ckv_cache.shape[0], ckv_cache.shape[1]
    idx = idx.long().clone()
    if neg_as_zero:
        idx[idx < 0] = 0
    valid = (idx >= 0) & (idx // P < block_ids_row.numel())
    if mask_vis:
        valid &= idx < vis
    slot = torch.where(valid, idx // P, torch.zeros_like(idx))
    page = block_ids_row.long()[slot] if translate else slot
    valid &= (page >= 0) & (page < num_blocks)
    page = torch.where(valid, page, torch.zeros_like(page))
    rows = ckv_cache[page, torch.where(valid, idx % P, torch.zeros_like(idx))].double()
    return rows * valid[:, None], valid


def sparse_statement(q, ckv_cache, block_ids, lens_total, indices, num_seq_q, softmax_scale, *, use_rope=True, ignore_list=False,
                     drop_slots=None, list_row=None, **gather_mutation):
    """(out float64 [B * Sq, H, 512], lse float64 [B * Sq, H]).  Mutations, all off by default: use_rope False ignores columns
    512..575 of the key; ignore_list attends to every visible token; drop_slots(valid) -> slots no row sees; list_row(b, s) ->
    the row of `indices` row (b, s) reads; the rest are gather_list's."""
    sq, H = num_seq_q, q.shape[1]
    B = len(lens_total)
    out = torch.zeros(B * sq, H, DIM_V, dtype=torch.float64)
    lse = torch.full((B * sq, H), float("-inf"), dtype=torch.float64)
    for b in range(B):
        for s in range(sq):
            r = b * sq + s
            vis = vis_of(lens_total, sq, b, s)
            idx = indices[r if list_row is None else list_row(b, s)]
            if ignore_list:
                idx = torch.arange(max(vis, 0), dtype=torch.int32)
            c, valid = gather_list(ckv_cache, block_ids[b], idx, vis, **gather_mutation)
            if drop_slots is not None:
                valid = valid.clone()
                valid[[k for k in drop_slots(valid) if 0 <= k < len(valid)]] = False
            if not bool(valid.any()):
                continue
            k = c if use_rope else torch.cat([c[:, :DIM_V], torch.zeros(len(c), DIM - DIM_V, dtype=torch.float64)], 1)
            z = softmax_scale * (q[r].double() @ k.T)  # [H, topk]
            z = z.masked_fill(~valid[None, :], float("-inf"))
            l = torch.logsumexp(z, -1)
            lse[r] = l
            out[r] = torch.exp(z - l[:, None]) @ c[:, :DIM_V]
    return out, lse


def sparse_eager(q, ckv_cache, block_ids, lens_total, indices, num_seq_q, softmax_scale):
    """The same attention in eager torch on q's device and in its dtype (index arithmetic, a row gather through the page table,
    two batched matmuls, a masked softmax): what a caller runs without the op, and what tools/tune_mla_sparse.py times it
    against.  lens_total: an int tensor on q's device.  Rows without a valid entry come back as zeros."""
    sq, P = num_seq_q, ckv_cache.shape[1]
    R = q.shape[0]
    req = torch.arange(R, device=q.device) // sq
    vis = lens_total.long()[req] - sq + torch.arange(R, device=q.device) % sq + 1
    idx = indices.long()
    valid = (idx >= 0) & (idx < vis[:, None]) & (idx // P < block_ids.shape[1])
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    page = block_ids.long()[req[:, None], safe // P]
    valid &= (page >= 0) & (page < ckv_cache.shape[0])
    page = torch.where(valid, page, torch.zeros_like(page))
    c = ckv_cache[page, safe % P]  # [R, topk, 576]
    z = torch.einsum("rhd,rkd->rhk", q, c).float() * softmax_scale
    z = z.masked_fill(~valid[:, None, :], float("-inf"))
    p = torch.softmax(z, -1).nan_to_num(0.0)
    return torch.einsum("rhk,rkd->rhd", p.to(q.dtype), c[..., :DIM_V])
