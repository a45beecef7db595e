"""Needle inputs, a CPU model of the kernel's online softmax and the measured bars for hpc.attention_prefill_mla_bf16 and
hpc.merge_attn_states (after tests/prefill_needles.py; the statements are tests/mla_prefill_ref.py).

Needles, 192 / 128.  Of the 128 nope columns the first 72 are channels that every key and every row use, the 64 RoPE columns
are channels too:

* key token j of a request is zero on them except the value T_KEY on position channel j % 64, on region channel
  64 + (j // 64) % 8 (a region = one 64-token tile of the kernel) and - in k_pe, the head all heads share - on RoPE channel
  ((j // 512) + j % 64) % 64; nope columns 72..127 hold noise that depends on j % 64 and the head only;
* a q row whose last visible key is `lim` has alpha / scale on ONE position channel a, on up to TWO region channels and on
  up to TWO RoPE channels, alpha in [0.8, 1.4] per (row, head), and noise on nope columns 72..127.  A key that matches all
  three kinds scores 3 alpha T_KEY; the second target's region channel is lower, so that it scores 0.5 ... 2.5 below the
  first: two weights of the same order whose ratio moves with the softmax scale.  Position and region repeat every 512
  tokens; only the RoPE channel tells those keys apart, so a kernel that ignores k_pe sees decoys as full matches (and one
  that reads k_pe from another row loses the needle);
* rows of even heads aim at their last visible key (the diagonal must be included) and at the key of the same position
  channel in a far region: tile 0, the tile of the last context token, of the first new token, the tile before their own, or
  any earlier one;
* rows of odd heads aim at key lim + 1 - 64 and at key lim + 1: a full match the causal mask must hide - the next row's own
  token, for the last row the first key of the next request or a poison row.

All matches of one target are the same bytes on every coordinate q touches: exact ties, which keeps the bar tight.  V of head h
is scaled by 1 + 0.5 (h % 4).

Memory as the op's intended callers have it: k_nope / v are the halves kv[..., :128] / kv[..., 128:] of one [rows, H, 256]
buffer, k_pe is columns 512.. of a [rows, 576] buffer.  Poison, all finite: PAD rows before the first request and after
cu_seqlens[-1] (POISON on every channel of k_nope and k_pe, 4 x V); columns :512 of every 576-wide row; the rows of the
neighbouring requests carry the same channels, so a read across a request's end finds full matches; seen through a head stride
of 128 the other half of the 256-wide buffer is V (or, for v, K's T_KEY).

Online model: how the kernel computes, restated in fp32 - scores as a column-ordered chain of fp32 multiply-adds over the 192
columns, scaled into log2 units, stages of 64 tokens from token 0, a running maximum m, P = bf16(exp2(t - m)), an fp32 sum of
the unrounded values, O and l rescaled at every stage, out = bf16(O * (1 / l)), lse = (m + log2 l) ln 2.

Bars.  TAU_* is the bar of utils.attn_close on `out`, LSE_BAR_* the absolute bar on `lse`; each is set from the model's worst
disagreement with the float64 statement on the calibration cases of tests/test_attention_prefill_mla.py and
tests/test_merge_attn_states.py (which measure them again on every run, assert model <= bar <= 3 x model and print both)."""
import math

import torch

import mla_prefill_ref as ref

D_NOPE, D_PE, D_V, D_QK = ref.DIM_NOPE, ref.DIM_PE, ref.DIM_V, ref.DIM_QK
SCALE = ref.SCALE
CA, CB = 64, 8  # position channels (j % 64), region channels ((j // 64) % 8)
NCH = CA + CB
T_KEY = 8.0
POISON = 40.0
SIGMA_Q, SIGMA_K = 0.3, 0.5
PAD = 70  # poison rows in front of the first request and behind the last
KV_TILE = 64
GAP = (0.5, 2.5)  # how far, in logits, a row's second target scores below its first

# measured worst case of the online model beside each bar (the tests print them)
TAU_NEEDLE = 0.016         # model 0.0069 of the row's scale: one bf16 ulp of the row's largest element (a double rounding)
LSE_BAR_NEEDLE = 4.5e-5    # model 1.89e-5: the fp32 multiply-add chain of a needle score of ~400 before the scale, lse <= 34 (ulp 3.8e-6)
TAU_MERGE = 0.008          # model 0.0037 of the row's scale against the UNROUNDED statement: half a bf16 ulp of the largest element
LSE_BAR_MERGE = 4.5e-6     # model 1.8e-6: one fp32 ulp of an lse of 16 .. 32


def pe_channel(j):
    return ((j // 512) + j % CA) % D_PE


def needle_inputs(seq_q, seq_k=None, H=2, causal=True, seed=0):
    """Needle inputs on the CPU.  seq_q: q rows per request; seq_k: keys per request (None: the same, and cu_k is cu_q).
    Returns a dict: q bf16 [Tq, H, 192]; kv bf16 [PAD + Tk + PAD, H, 256] and ckv bf16 [PAD + Tk + PAD, 576] with the views
    k_nope, v, k_pe on rows PAD .. PAD + Tk; cu_q, cu_k int32; max_q, max_k; H, causal, scale."""
    self_attn = seq_k is None
    seq_k = list(seq_q) if self_attn else list(seq_k)
    B = len(seq_q)
    assert len(seq_k) == B
    cu_q = torch.zeros(B + 1, dtype=torch.int32)
    cu_q[1:] = torch.tensor(seq_q, dtype=torch.int32).cumsum(0)
    cu_k = torch.zeros(B + 1, dtype=torch.int32)
    cu_k[1:] = torch.tensor(seq_k, dtype=torch.int32).cumsum(0)
    Tq, Tk = int(cu_q[-1]), int(cu_k[-1])
    gen = torch.Generator().manual_seed(seed)
    rows = PAD + Tk + PAD
    K = torch.zeros(rows, H, D_NOPE)
    V = torch.randn(rows, H, D_V, generator=gen) * (1 + 0.5 * (torch.arange(H) % 4))[None, :, None]
    PE = torch.zeros(rows, D_PE)
    knoise = torch.randn(CA, H, D_NOPE, generator=gen) * SIGMA_K
    knoise[..., :NCH] = 0
    # poison rows on both sides
    for sl in (slice(0, PAD), slice(PAD + Tk, rows)):
        K[sl] = torch.randn(K[sl].shape, generator=gen) * SIGMA_K
        K[sl, :, :NCH] = POISON
        PE[sl] = POISON
        V[sl] *= 4
    q = torch.randn(Tq, H, D_QK, generator=gen) * SIGMA_Q
    q[..., :NCH] = 0
    q[..., D_NOPE:] = 0
    alpha = 0.8 + 0.6 * torch.rand(Tq, H, generator=gen)
    h = torch.arange(H)[None, :]
    odd = (h & 1) == 1
    for b in range(B):
        Sq, Lk = int(seq_q[b]), int(seq_k[b])
        k0 = PAD + int(cu_k[b])
        j = torch.arange(Lk)
        kk = knoise[j % CA].clone()
        kk[j, :, j % CA] = T_KEY
        kk[j, :, CA + (j // 64) % CB] = T_KEY
        K[k0: k0 + Lk] = kk
        PE[k0 + j, pe_channel(j)] = T_KEY
        if Sq == 0:
            continue
        s = torch.arange(Sq)[:, None]
        lim = (Lk - Sq + s) if causal else torch.full_like(s, Lk - 1)  # [Sq, 1]: the last key the row sees
        seen = (lim >= 0).expand(Sq, H)
        lim = lim.clamp_min(0).expand(Sq, H)
        shifted = odd & (lim + 1 - CA >= 0)
        j1 = torch.where(shifted, lim + 1 - CA, lim)
        a = j1 % CA
        own = lim // 64
        past = max(Lk - Sq, 0)
        rnd = (torch.rand(Sq, H, generator=gen) * (own + 1)).long()
        cand = torch.stack([torch.zeros_like(rnd), torch.full_like(rnd, max(past - 1, 0) // 64), torch.full_like(rnd, past // 64),
                            rnd, (own - 1).clamp_min(0)])
        R = torch.gather(cand, 0, ((s + 3 * h + 7 * b) % 5)[None])[0]
        R = torch.where(64 * R + a > lim, R - 1, R)
        j2 = torch.where(R < 0, j1, 64 * R + a)
        j2 = torch.where(shifted, lim + 1, j2)  # odd heads: key lim + 1 is a full match they must not see
        r0 = int(cu_q[b]) + torch.arange(Sq)[:, None].expand(Sq, H)
        hh = h.expand(Sq, H)
        val = alpha[int(cu_q[b]): int(cu_q[b + 1])] / SCALE
        val = torch.where(seen, val, torch.zeros_like(val))  # a row without a key: noise only
        # the second target scores `gap` below the first (its region channel is lower): two weights of the same order whose
        # ratio moves with the softmax scale
        gap = GAP[0] + (GAP[1] - GAP[0]) * torch.rand(Sq, H, generator=gen)
        low = torch.where(seen, val - gap / (SCALE * T_KEY), torch.zeros_like(val))
        q[r0, hh, a] = val
        for jt, rv in ((j1, val), (j2, low)):
            q[r0, hh, CA + (jt // 64) % CB] = rv
            q[r0, hh, D_NOPE + pe_channel(jt)] = val
    kv = torch.cat([K, V], -1).to(torch.bfloat16)
    ckv = torch.full((rows, 576), POISON)
    ckv[:, 512:] = PE
    ckv = ckv.to(torch.bfloat16)
    inp = dict(q=q.to(torch.bfloat16), kv=kv, ckv=ckv, cu_q=cu_q, cu_k=None if self_attn else cu_k, seq_q=list(seq_q), seq_k=seq_k,
               max_q=max(list(seq_q) + [0]), max_k=max(seq_k + [0]), H=H, causal=causal, scale=SCALE, Tk=Tk)
    return with_views(inp)


def with_views(inp):
    """(re)derive the three views from the buffers (after a .cuda() of kv / ckv, say)"""
    Tk = inp["Tk"]
    inp["k_nope"] = inp["kv"][PAD: PAD + Tk, :, :D_NOPE]
    inp["v"] = inp["kv"][PAD: PAD + Tk, :, D_NOPE:]
    inp["k_pe"] = inp["ckv"][PAD: PAD + Tk, 512:]
    return inp


def statement(inp, **mutation):
    """(out bf16, lse float64) of the float64 statement on `inp`; keyword arguments are prefill_statement's mutations, plus
    scale= for another softmax scale"""
    scale = mutation.pop("scale", inp["scale"])
    out, lse = ref.prefill_statement(inp["q"], inp["k_nope"], inp["k_pe"], inp["v"], inp["cu_q"], inp["cu_k"], scale,
                                     inp["causal"], **mutation)
    return out.to(torch.bfloat16), lse


def online_model(inp, stage=KV_TILE):
    """(out bf16 [Tq, H, 128], lse float32 [Tq, H]) of the online model (module docstring)"""
    q, H = inp["q"], inp["H"]
    cu_q = inp["cu_q"]
    cu_k = cu_q if inp["cu_k"] is None else inp["cu_k"]
    out = torch.zeros(q.shape[0], H, D_V, dtype=torch.bfloat16)
    lse = torch.full((q.shape[0], H), float("-inf"), dtype=torch.float32)
    k2 = torch.tensor(inp["scale"], dtype=torch.float32) * torch.tensor(math.log2(math.e), dtype=torch.float32)
    ln2 = torch.tensor(math.log(2.0), dtype=torch.float32)
    for b in range(len(cu_q) - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        Sq, Lk = q1 - q0, k1 - k0
        if Sq == 0 or Lk == 0:
            continue
        qf = q[q0:q1].float()
        kn, kp, vf = inp["k_nope"][k0:k1].float(), inp["k_pe"][k0:k1].float(), inp["v"][k0:k1].float()
        # the score as a column-ordered chain of fp32 multiply-adds, spelled out so that it is the same on every host.  How the
        # matrix instruction adds the 32 products of a step is not documented for bf16 operands, so the model assumes no more
        # than fp32 accumulation gives
        t = torch.zeros(Sq, H, Lk, dtype=torch.float32)
        for c in range(D_NOPE):
            t = t + qf[:, :, c, None] * kn[:, :, c].t()[None]
        for c in range(D_PE):
            t = t + qf[:, :, D_NOPE + c, None] * kp[None, None, :, c]
        t = t * k2
        s = torch.arange(Sq)[:, None]
        vis = torch.arange(Lk)[None, :] <= (Lk - Sq + s if inp["causal"] else torch.full_like(s, Lk - 1))
        t = t.masked_fill(~vis[:, None, :], float("-inf"))
        m = torch.full((Sq, H), float("-inf"))
        l = torch.zeros(Sq, H)
        o = torch.zeros(Sq, H, D_V)
        for t0 in range(0, Lk, stage):
            st = t[:, :, t0: t0 + stage]
            mn = torch.maximum(m, st.amax(-1))
            ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
            w = torch.exp2(st - ms[..., None])
            r = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - ms))
            l = l * r + w.sum(-1)
            o = o * r[..., None] + torch.einsum("shj,jhd->shd", w.to(torch.bfloat16).float(), vf[t0: t0 + stage])
            m = mn
        seen = l > 0
        inv = torch.where(seen, 1.0 / torch.where(seen, l, torch.ones_like(l)), torch.zeros_like(l))
        out[q0:q1] = (o * inv[..., None]).to(torch.bfloat16)
        lse[q0:q1] = torch.where(seen, (torch.where(seen, m, torch.zeros_like(m)) + torch.log2(torch.where(seen, l, torch.ones_like(l)))) * ln2,
                                 torch.full_like(l, float("-inf")))
    return out, lse


def merge_model(out_a, lse_a, out_b, lse_b):
    """(out bf16, lse float32) of the merge as the kernel computes it: fp32, one reciprocal, one rounding to bf16"""
    a, b = out_a.float(), out_b.float()
    la, lb = lse_a.float(), lse_b.float()
    m = torch.maximum(la, lb)
    dead_a, dead_b = torch.isinf(la) & (la < 0), torch.isinf(lb) & (lb < 0)
    ms = torch.where(dead_a & dead_b, torch.zeros_like(m), m)
    wa, wb = torch.exp(la - ms), torch.exp(lb - ms)
    den = wa + wb
    inv = 1.0 / torch.where(den > 0, den, torch.ones_like(den))
    out = ((wa[..., None] * a + wb[..., None] * b) * inv[..., None]).to(torch.bfloat16)
    lse = ms + torch.log(torch.where(den > 0, den, torch.ones_like(den)))
    one = dead_a | dead_b
    out = torch.where(one[..., None], torch.where(dead_a[..., None], out_b, out_a), out)
    out = torch.where((dead_a & dead_b)[..., None], torch.zeros_like(out), out)
    lse = torch.where(one, m, lse)
    return out, lse


def merge_inputs(T, H, D, spread=30.0, seed=0, dead=True):
    """random states: out_* randn bf16 [T, H, D], lse_* uniform over +-spread; with `dead` a few rows have -inf on one side or
    on both"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(T, H, D, generator=g).to(torch.bfloat16)
    b = (torch.randn(T, H, D, generator=g) * 2).to(torch.bfloat16)
    la = (torch.rand(T, H, generator=g) * 2 - 1) * spread
    lb = (torch.rand(T, H, generator=g) * 2 - 1) * spread
    near = torch.rand(T, H, generator=g) < 0.5  # half of the rows: the two sides within a few units, both weights count
    lb = torch.where(near, la + (torch.rand(T, H, generator=g) * 2 - 1) * 3, lb)
    if dead and T * H >= 6:
        flat_a, flat_b = la.view(-1), lb.view(-1)
        n = T * H
        flat_a[0] = float("-inf")
        flat_b[n // 2] = float("-inf")
        flat_a[n - 1] = float("-inf")
        flat_b[n - 1] = float("-inf")
    return a, la, b, lb
