"""The statement of hpc.attention_decode_mla_bf16 in float64 PyTorch (CPU), and the knobs the bar tests turn to make mutants.

    q            bf16 [B * Sq, H, 576]      Sq = mtp + 1; columns 0..511 latent (q_nope W_UK), 512..575 RoPE
    ckv_cache    bf16 logical [num_blocks, P, 576]   one latent row per token
    block_ids    int32 [B, max_blocks]      entries past a request's pages are not looked at
    lens_total   int [B]                    L_b: tokens of request b INCLUDING the Sq new ones

    row (b, s, h) sees tokens j < L_b - Sq + s + 1
    z_j   = softmax_scale * sum_{d < 576} q[b*Sq+s, h, d] * c_b[j, d]
    out[b*Sq+s, h, :] = sum_j softmax(z)_j * c_b[j, :512]
    lse[b*Sq+s, h]    = log sum_j exp(z_j)

Both come back in float64 (round `out` with .to(torch.bfloat16) to compare with the op)."""
import torch

DIM, DIM_V = 576, 512


def latent_rows(ckv_cache, block_ids_row, length):
    """the `length` latent rows of one request, through its page table"""
    P = ckv_cache.shape[1]
    pages = block_ids_row[: (length + P - 1) // P].long()
    return ckv_cache[pages].reshape(-1, ckv_cache.shape[-1])[:length]


def mla_statement(q, ckv_cache, block_ids, lens_total, num_seq_q, softmax_scale, *, use_rope=True, v_shift=0,
                  causal_shift=0, drop=None):
    """(out float64 [B * Sq, H, 512], lse float64 [B * Sq, H]).  Mutations, all off by default: use_rope False ignores columns
    512..575 of the key; v_shift takes columns v_shift .. v_shift + 511 as the value; causal_shift moves every row's limit;
    drop(L) -> token positions no row sees."""
    sq, H = num_seq_q, q.shape[1]
    B = len(lens_total)
    out = torch.zeros(B * sq, H, DIM_V, dtype=torch.float64)
    lse = torch.zeros(B * sq, H, dtype=torch.float64)
    for b in range(B):
        L = int(lens_total[b])
        c = latent_rows(ckv_cache, block_ids[b], L).double()
        k = c if use_rope else torch.cat([c[:, :DIM_V], torch.zeros(L, DIM - DIM_V, dtype=torch.float64)], 1)
        z = softmax_scale * torch.einsum("shd,jd->shj", q[b * sq: (b + 1) * sq].double(), k)
        vis = torch.arange(L)[None, :] < (L - sq + torch.arange(sq) + 1 + causal_shift)[:, None]
        if drop is not None:
            vis[:, [t for t in drop(L) if 0 <= t < L]] = False
        z = z.masked_fill(~vis[:, None, :], float("-inf"))
        l = torch.logsumexp(z, -1)
        lse[b * sq: (b + 1) * sq] = l
        out[b * sq: (b + 1) * sq] = torch.exp(z - l[..., None]) @ c[:, v_shift: v_shift + DIM_V]
    return out, lse


def mla_eager(q, ckv_cache, block_ids, lens_total, num_seq_q, softmax_scale):
    """The same attention in eager torch on q's device and in its dtype (page gather, two batched matmuls, softmax): what a
    caller runs without the op, and what tools/tune_mla.py times it against.  lens_total: a list of ints."""
    sq = num_seq_q
    outs = []
    for b, L in enumerate(lens_total):
        c = latent_rows(ckv_cache, block_ids[b], L)
        z = torch.einsum("shd,jd->shj", q[b * sq: (b + 1) * sq], c).float() * softmax_scale
        if sq > 1:
            vis = torch.arange(L, device=q.device)[None, :] < (L - sq + torch.arange(sq, device=q.device) + 1)[:, None]
            z = z.masked_fill(~vis[:, None, :], float("-inf"))
        outs.append(torch.softmax(z, -1).to(q.dtype) @ c[:, :DIM_V])
    return torch.cat(outs, 0)
