"""Needle inputs, a CPU model of the split-KV arithmetic and the measured bars for hpc.attention_decode_mla_bf16
(after tests/decode_needles.py; the statement is tests/mla_ref.py).

Needles.  Every (request, row s, head h) owns one latent column (`needle_columns`: one in eight of them a RoPE column
512..575, so the RoPE part must count) and has one token, at an edge position, whose value in that column makes it take
most of the row's softmax: token 0, P - 1, P, P + 1, 63, 64, 65, the boundaries of the pieces of 2, 3 and 8 splits and
their neighbours, the last cached token, the row's own new token.  Unlike a GQA cache the latent row is key AND value, so a
needle token keeps its background in every other column and |y| ~ 1.  The owned columns carry a tenth of the background
elsewhere (they are multiplied by the large own coordinate of q).

Poison (all finite) dominates every head if it is read: the slots of each request's last page past its length, every pool
page outside all block tables, and - for row s - the new token of row s + 1, which holds the poison in row s's columns.
block_ids entries past a request's pages are -999999.

Split model: how the kernel computes, restated on the CPU in fp32 - scores as a column-ordered chain of fp32 multiply-adds, scaled into
log2 units, a per-piece maximum,
P = bf16(exp2(t - m)), an fp32 sum of the unrounded exponentials, an fp32 P V, a merge of the pieces by their maxima and sums,
one division, a bf16 result, lse = (M + log2(sum)) ln 2.

Bars.  TAU_* is the bar of utils.attn_close on `out`, LSE_BAR_* the absolute bar on `lse`; each is set from the model's
worst disagreement with the float64 statement over piece lengths 16 ... 4096 on the calibration cases of
tests/test_attention_decode_mla.py (which measures them again on every run, asserts model <= bar <= 3 x model and prints
both)."""
import math

import torch

import mla_ref

DIM, DIM_V = mla_ref.DIM, mla_ref.DIM_V
SCALE = 1.0 / math.sqrt(128 + 64)  # the models' softmax scale without a YaRN factor
SIGMA_Q, SIGMA_C = 0.3, 0.5        # background q / latent noise per coordinate: background logits have std ~0.26
OWN_BG = 0.1                       # the owned columns' background, relative to SIGMA_C
POISON = 8.0                       # poison value in the owned columns: logit 8 alpha >= 32, above every needle (ln 20004 + 2.2 < 13)
PIECE_LENS = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
KV_TILE = 64

# measured worst case of the split model beside each bar (test_split_model_within_bars prints them)
TAU_NEEDLE = 0.02         # model 0.00735 of the row's scale (one bf16 ulp of the row's largest element: a double rounding)
LSE_BAR_NEEDLE = 3.0e-5   # model 1.22e-5: the fp32 multiply-add chain of a needle score of ~190 before the scale (ulp 1.5e-5), lse <= 13
TAU_UNIFORM = 0.02        # model 0.00775
LSE_BAR_UNIFORM = 3.0e-6  # model 1.11e-6 (lse ~ ln L <= 9.1: three fp32 ulps)


def piece_len(L, splits):
    """tokens per piece of a request of L tokens: ceil(L / splits) rounded up to the kernel's KV tile"""
    return (-(-L // splits) + KV_TILE - 1) // KV_TILE * KV_TILE


def edge_lens(P):
    """cached-token counts before the step that every parity configuration runs"""
    return [0, 1, 2, P - 1, P, P + 1, 63, 64, 65, 127, 129, 1023, 1025, 4 * P + 1, 5000]


def needle_columns(nrows):
    """the latent column owned by row index i = s * H + h: every eighth a RoPE column while they last"""
    nope, rope = iter(range(DIM_V)), iter(range(DIM_V, DIM))
    cols = []
    for i in range(nrows):
        c = next(rope, None) if i % 8 == 7 else None
        cols.append(next(nope) if c is None else c)
    return torch.tensor(cols, dtype=torch.long)


def _pages(lens_total, P, spare, gen):
    nblocks = (lens_total + P - 1) // P
    used = int(nblocks.sum())
    perm = torch.randperm(used + spare, generator=gen).to(torch.int32)
    block_ids = torch.full((len(lens_total), max(1, int(nblocks.max()))), -999999, dtype=torch.int32)
    off = 0
    for i, nb in enumerate(nblocks.tolist()):
        block_ids[i, :nb] = perm[off: off + nb]
        off += nb
    return block_ids, nblocks, used + spare, perm[used:]


def _poison(ckv, block_ids, nblocks, lens_total, spare, cols, gen):
    P = ckv.shape[1]
    for b, nb in enumerate(nblocks.tolist()):
        first = int(lens_total[b]) - (nb - 1) * P
        if first < P:
            page = int(block_ids[b, nb - 1])
            ckv[page, first:] = torch.randn(P - first, DIM, generator=gen) * 2
            ckv[page, first:, cols] = POISON
    if len(spare):
        sp = spare.long()
        ckv[sp] = torch.randn(len(sp), P, DIM, generator=gen) * 2
        ckv[sp[:, None, None], torch.arange(P)[None, :, None], cols[None, None, :]] = POISON


def needle_inputs(lens_before, num_seq_q, P, H, seed=0):
    """Needle inputs on the CPU: q bf16 [B * Sq, H, 576], ckv bf16 [pool, P, 576], block_ids, lens_before / lens_total int32,
    scale, and the spare (unlisted) pool pages."""
    sq = num_seq_q
    lens_before = torch.as_tensor(lens_before, dtype=torch.int32)
    lens_total = lens_before + sq
    B = len(lens_total)
    gen = torch.Generator().manual_seed(seed)
    block_ids, nblocks, pool, spare = _pages(lens_total, P, 3, gen)
    cols = needle_columns(sq * H)
    alpha = 4.0 + 2.0 * torch.rand(B * sq, H, generator=gen)  # the own-coordinate logit per unit of the planted value
    ckv = torch.randn(pool, P, DIM, generator=gen) * SIGMA_C
    ckv[:, :, cols] *= OWN_BG
    q = torch.randn(B * sq, H, DIM, generator=gen) * SIGMA_Q
    q[:, :, cols] = 0  # no cross-talk with the other rows' / heads' columns
    _poison(ckv, block_ids, nblocks, lens_total, spare, cols, gen)
    for b in range(B):
        lb, L = int(lens_before[b]), int(lens_total[b])
        for s in range(sq):
            vis = lb + s + 1
            cands = [0, P - 1, P, P + 1, 63, 64, 65, lb - 1, lb + s]
            for splits in (2, 3, 8):
                bd = piece_len(L, splits)
                cands += [bd - 1, bd, bd + 1, 2 * bd - 1, 2 * bd]
            cands = sorted({p for p in cands if 0 <= p < vis})
            for h in range(H):
                i = s * H + h
                a = float(alpha[b * sq + s, h])
                share = 0.3 + 1.9 * float(torch.rand(1, generator=gen))  # the needle takes ~54 ... 89 % of the softmax
                pos = cands[(h + 3 * s + 7 * b) % len(cands)]
                ckv[int(block_ids[b, pos // P]), pos % P, cols[i]] = (math.log(vis) + share) / a
                q[b * sq + s, h, cols[i]] = a / SCALE
            if s + 1 < sq:  # row s + 1's new token: dominates row s if row s could see it
                t = lb + s + 1
                ckv[int(block_ids[b, t // P]), t % P, cols[s * H: (s + 1) * H]] = POISON
    return dict(q=q.to(torch.bfloat16), ckv=ckv.to(torch.bfloat16), block_ids=block_ids, nblocks=nblocks,
                lens_before=lens_before, lens_total=lens_total, num_seq_q=sq, P=P, H=H, scale=SCALE, spare=spare)


def uniform_inputs(lens_before, num_seq_q, P, H, seed=41):
    """the reference tests' generator carried over to the latent cache: randn latents, randn q / sqrt(576) - a near-uniform
    softmax, |y| ~ 1e-2"""
    sq = num_seq_q
    lens_before = torch.as_tensor(lens_before, dtype=torch.int32)
    lens_total = lens_before + sq
    gen = torch.Generator().manual_seed(seed)
    block_ids, nblocks, pool, spare = _pages(lens_total, P, 3, gen)
    ckv = torch.randn(pool, P, DIM, generator=gen)
    q = torch.randn(len(lens_total) * sq, H, DIM, generator=gen) / math.sqrt(DIM)
    return dict(q=q.to(torch.bfloat16), ckv=ckv.to(torch.bfloat16), block_ids=block_ids, nblocks=nblocks,
                lens_before=lens_before, lens_total=lens_total, num_seq_q=sq, P=P, H=H, scale=SCALE, spare=spare)


def statement(inp, **mutation):
    """(out bf16, lse float64) of the float64 statement on `inp`; keyword arguments are mla_ref.mla_statement's mutations,
    plus scale= for another softmax scale"""
    scale = mutation.pop("scale", inp["scale"])
    out, lse = mla_ref.mla_statement(inp["q"], inp["ckv"], inp["block_ids"], inp["lens_total"], inp["num_seq_q"], scale,
                                     **mutation)
    return out.to(torch.bfloat16), lse


def split_model(inp, plen, drop_piece=None):
    """(out bf16 [B * Sq, H, 512], lse float32 [B * Sq, H]) of the split model (module docstring) with pieces of `plen`
    tokens.  drop_piece: index of a piece the merge leaves out (a mutant)."""
    sq, H = inp["num_seq_q"], inp["H"]
    B = len(inp["lens_total"])
    out = torch.empty(B * sq, H, DIM_V, dtype=torch.bfloat16)
    lse = torch.empty(B * sq, H, dtype=torch.float32)
    k2 = torch.tensor(inp["scale"], dtype=torch.float32) * torch.tensor(math.log2(math.e), dtype=torch.float32)
    ln2 = torch.tensor(math.log(2.0), dtype=torch.float32)
    for b in range(B):
        L = int(inp["lens_total"][b])
        c = mla_ref.latent_rows(inp["ckv"], inp["block_ids"][b], L).float()
        # the score as a column-ordered chain of fp32 multiply-adds, spelled out so that it is the same on every host (an fp32
        # matmul's summation order is the host library's).  How the matrix instruction adds the 32 products of a step is not
        # documented for bf16 operands, so the model assumes no more than fp32 accumulation gives
        qf = inp["q"][b * sq: (b + 1) * sq].float()
        t = torch.zeros(sq, H, L, dtype=torch.float32)
        for k in range(DIM):
            t = t + qf[:, :, k, None] * c[None, None, :, k]
        t = t * k2
        vis = torch.arange(L)[None, :] < (L - sq + torch.arange(sq) + 1)[:, None]
        t = t.masked_fill(~vis[:, None, :], float("-inf"))
        n = -(-L // plen)
        pad = n * plen - L
        tr = torch.nn.functional.pad(t, (0, pad), value=float("-inf")).reshape(sq, H, n, plen)
        vr = torch.nn.functional.pad(c[:, :DIM_V], (0, 0, 0, pad)).reshape(n, plen, DIM_V)
        m = tr.amax(-1)
        ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        w = torch.exp2(tr - ms[..., None])
        lsum = w.sum(-1)
        o = torch.einsum("shnt,ntd->shnd", w.to(torch.bfloat16).float(), vr)
        M = m.amax(-1, keepdim=True)
        a = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - M))
        if drop_piece is not None and -n <= drop_piece < n and n > 1:
            a[..., drop_piece] = 0
        den = (a * lsum).sum(-1, keepdim=True)
        out[b * sq: (b + 1) * sq] = ((a[..., None] * o).sum(2) / den).to(torch.bfloat16)
        lse[b * sq: (b + 1) * sq] = ((M + torch.log2(den)) * ln2)[..., 0]
    return out, lse


def lse_err(ref64, got):
    """worst |got - ref| of an lse, NaN counted as infinite"""
    return float((got.double().cpu() - ref64).abs().nan_to_num(nan=float("inf")).max())
