"""The statements of hpc.attention_prefill_mla_bf16 and hpc.merge_attn_states in float64 PyTorch (CPU), and the knobs the bar
tests turn to make mutants.

    q            bf16 [Tq, H, 192]     columns 0..127 nope, 128..191 RoPE'd
    k_nope, v    bf16 [Tk, H, 128]
    k_pe         bf16 [Tk, 64]         one RoPE'd head shared by all H heads
    cu_q, cu_k   int [B + 1]           request b: q rows cu_q[b] .. cu_q[b + 1], keys cu_k[b] .. cu_k[b + 1]

    request b has Sq q rows and Lk keys; with causal, row s sees keys j <= Lk - Sq + s (bottom-right aligned), without it every
    j < Lk
    z_j = softmax_scale * (q[s, h, :128] . k_nope[j, h] + q[s, h, 128:] . k_pe[j])
    out[s, h, :] = sum_j softmax(z)_j * v[j, h, :]
    lse[s, h]    = log sum_j exp(z_j)
    a row that sees no key: out = 0, lse = -inf

Both come back in float64 (round `out` with .to(torch.bfloat16) to compare with the op).

    merge: m = max(la, lb), wa = exp(la - m), wb = exp(lb - m), out = (wa a + wb b) / (wa + wb), lse = m + log(wa + wb);
    one side -inf: the other side as it is; both: zeros and -inf"""
import math

import torch

DIM_NOPE, DIM_PE, DIM_V = 128, 64, 128
DIM_QK = DIM_NOPE + DIM_PE


def prefill_statement(q, k_nope, k_pe, v, cu_q, cu_k, softmax_scale, causal=True, *, use_pe=True, pe_row_of_head=False,
                      v_from_k_nope=False, causal_shift=0, top_left=False, drop=None):
    """(out float64 [Tq, H, 128], lse float64 [Tq, H]).  cu_k None: cu_q.  Mutations, all off by default: use_pe False ignores
    k_pe; pe_row_of_head reads head h's k_pe from row (j * H + h) % Lk of the request (a kernel that takes k_pe for a
    [Tk, H, 64] tensor); v_from_k_nope takes k_nope as the value; causal_shift moves every causal row's limit; top_left aligns
    the causal mask at the first key (row s sees j <= s); drop(Lk) -> key positions no row sees."""
    cu_k = cu_q if cu_k is None else cu_k
    Tq, H = q.shape[0], q.shape[1]
    out = torch.zeros(Tq, H, DIM_V, dtype=torch.float64)
    lse = torch.full((Tq, H), float("-inf"), dtype=torch.float64)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        Sq, Lk = q1 - q0, k1 - k0
        if Sq == 0 or Lk == 0:
            continue
        qq = q[q0:q1].double()
        kn, kp, vv = k_nope[k0:k1].double(), k_pe[k0:k1].double(), (k_nope if v_from_k_nope else v)[k0:k1].double()
        z = torch.einsum("shd,jhd->shj", qq[..., :DIM_NOPE], kn)
        if use_pe:
            if pe_row_of_head:
                rows = (torch.arange(Lk)[:, None] * H + torch.arange(H)[None, :]) % Lk  # [Lk, H]
                z = z + torch.einsum("shd,jhd->shj", qq[..., DIM_NOPE:], kp[rows])
            else:
                z = z + torch.einsum("shd,jd->shj", qq[..., DIM_NOPE:], kp)
        z = z * softmax_scale
        s = torch.arange(Sq)[:, None]
        if causal:
            vis = torch.arange(Lk)[None, :] <= (s if top_left else Lk - Sq + s) + causal_shift
        else:
            vis = torch.ones(Sq, Lk, dtype=torch.bool)
        if drop is not None:
            vis[:, [t for t in drop(Lk) if 0 <= t < Lk]] = False
        z = z.masked_fill(~vis[:, None, :], float("-inf"))
        l = torch.logsumexp(z, -1)
        seen = vis.any(-1)[:, None].expand(Sq, H)
        p = torch.exp(z - torch.where(seen, l, torch.zeros_like(l))[..., None])  # rows without a key: exp(-inf) = 0
        out[q0:q1] = torch.einsum("shj,jhd->shd", p, vv)
        lse[q0:q1] = torch.where(seen, l, torch.full_like(l, float("-inf")))
    return out, lse


def merge_statement(out_a, lse_a, out_b, lse_b, *, swap_weights=False, lse_is_max=False):
    """(out float64 [T, H, D], lse float64 [T, H]) of the merge.  Mutations: swap_weights gives a the weight of b and b that of
    a; lse_is_max returns m without the log term."""
    a, b, la, lb = out_a.double(), out_b.double(), lse_a.double(), lse_b.double()
    m = torch.maximum(la, lb)
    ms = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    wa, wb = torch.exp(la - ms), torch.exp(lb - ms)
    if swap_weights:
        wa, wb = wb, wa
    den = wa + wb
    out = (wa[..., None] * a + wb[..., None] * b) / torch.where(den > 0, den, torch.ones_like(den))[..., None]
    lse = m if lse_is_max else torch.where(den > 0, ms + torch.log(den), torch.full_like(m, float("-inf")))
    return out, lse


def prefill_eager(q, k_nope, k_pe, v, cu_q, cu_k, softmax_scale, causal=True):
    """The same attention in eager torch on q's device and in its dtype: the 192-wide k assembled by a concat, then
    scaled_dot_product_attention per request (the float32 statement where it cannot express the mask: a causal request whose
    q and k counts differ).  What a caller runs without the op, and what tools/tune_mla_prefill.py times it against.  cu_q,
    cu_k: lists of ints."""
    cu_k = cu_q if cu_k is None else cu_k
    H = q.shape[1]
    outs = []
    for b in range(len(cu_q) - 1):
        qq = q[cu_q[b]: cu_q[b + 1]].transpose(0, 1)  # [H, Sq, 192]
        kn, kp, vv = k_nope[cu_k[b]: cu_k[b + 1]], k_pe[cu_k[b]: cu_k[b + 1]], v[cu_k[b]: cu_k[b + 1]]
        Sq, Lk = qq.shape[1], kn.shape[0]
        if Lk == 0:
            outs.append(torch.zeros(Sq, H, DIM_V, dtype=q.dtype, device=q.device))
            continue
        k = torch.cat([kn, kp[:, None, :].expand(Lk, H, DIM_PE)], -1).transpose(0, 1)  # the tensor the op never builds
        if not causal or Sq == Lk:
            y = torch.nn.functional.scaled_dot_product_attention(qq[None], k[None], vv.transpose(0, 1)[None], is_causal=causal,
                                                                 scale=softmax_scale)[0]
        else:
            z = (qq.float() @ k.float().transpose(1, 2)) * softmax_scale
            vis = torch.arange(Lk, device=q.device)[None, :] <= (Lk - Sq + torch.arange(Sq, device=q.device))[:, None]
            z = z.masked_fill(~vis[None], float("-inf"))
            y = (torch.softmax(z, -1).nan_to_num(0.0) @ vv.transpose(0, 1).float()).to(q.dtype)
        outs.append(y.transpose(0, 1))
    return torch.cat(outs, 0)


def merge_eager(out_a, lse_a, out_b, lse_b):
    """the merge in eager torch, float32, on the inputs' device"""
    m = torch.maximum(lse_a, lse_b)
    wa, wb = torch.exp(lse_a - m), torch.exp(lse_b - m)
    den = wa + wb
    out = (wa[..., None] * out_a.float() + wb[..., None] * out_b.float()) / den[..., None]
    return out.to(out_a.dtype), m + torch.log(den)


def lse_err(ref64, got):
    """worst |got - ref| of an lse where the reference is finite; where it is -inf the other must be -inf too (else inf);
    NaN counts as infinite"""
    r, g = ref64.double(), got.double().cpu()
    fin = torch.isfinite(r)
    if not torch.equal(g[~fin], r[~fin]):
        return float("inf")
    if not bool(fin.any()):
        return 0.0
    return float((g[fin] - r[fin]).abs().nan_to_num(nan=float("inf")).max())


SCALE = 1.0 / math.sqrt(DIM_QK)  # the models' softmax scale without a YaRN factor
