"""Needle inputs and a CPU model of the prefill kernels' online softmax, for the prefill-attention parity tests.

Why: with the reference tests' generators the softmax is almost uniform and a row's output is a mean of V over its whole
visible context, |y| ~ 1e-2: the absolute tolerances of those tests (0.1 for fp8, 0.016 for bf16) accept an all-zero
answer, a causal limit off by one, another request's pages, permuted q heads (tests/test_prefill_bar.py pins the first).

Needles.  Decode gives each of its <= 32 rows per kv head its own key coordinate; prefill has thousands of rows per kv
head, so here the first 96 of the 128 coordinates are channels that every key and every row use:

* key token j of a request is zero on them except the value T_KEY on position channel j % 64 and on region channel
  64 + (j // 64) % 32 (a region = one 64-token tile of the kernels); the other 32 coordinates hold noise;
* a q row at absolute position p (cached prefix included) has alpha sqrt(D) on ONE position channel a and on TWO region
  channels r1, r2, alpha in [0.6, 1.4] per (row, head), and noise on the 31 free coordinates.  A key that matches a and one
  of the regions scores 2 alpha T_KEY, a key that matches one of the two alpha T_KEY, the rest ~0: the few full matches
  (one per 2048 tokens and region) take 70 ... 99 % of the softmax, so every row has |y| of the order of V;
* rows of even local heads aim at their own token (a = p % 64, r1 = region of p: the diagonal must be included) and at a
  far region r2: tile 0, the tile of the last cached token, of the first new token, the tile before their own, or any
  earlier one;
* rows of odd local heads aim at token p + 1 - 64 (r1) and have r2 = the region of token p + 1: that key is a full match
  which the causal mask must hide, in a page tail or a foreign page for the last row.

The noise coordinates of a live key depend on j % 64 and the kv head only, so all full matches of a row are the same
bytes on every coordinate that q touches: exact maxima with P exactly 256 in e4m3, which keeps the bar tight.  Coordinate 96
is zero in q and holds 8, 16 or 32 in a key, at random per (token, kv head): the per-token K scales then differ by
powers of two between neighbours while the channels still dequantise to exactly T_KEY.  V of kv head g is scaled by
1 + 0.5 (g % 4), so the per-head V scales differ.

Poison (all finite, as in tests/decode_needles.py and for its reason): the slots of each request's last page past its
length and every pool page outside all block tables hold POISON on all 96 channels and 4 x V; block_ids beyond a request's
pages are -999999; qscale beyond a request's seq_q, and beyond max_seqlens_q, is junk (100 ... 110).

The online model restates how the kernels compute: stages of 128 tokens from token 0, a running maximum m, P =
e4m3(256 exp(s - m)) (fp8) or bf16(exp(s - m)) (bf16), the row sum in fp32 over the unrounded exponentials, O and l
rescaled at every stage, a bf16 result; the pinned oracles round P against the row's global maximum.  The bars (TAU_*) are
set from this model's worst disagreement with the oracles at stages of 64 and 128 tokens over BAR_CASES
(tests/test_prefill_bar.py asserts on every run that the model is within them and that they are at most 3 x that)."""
import math

import torch

from decode_needles import F8, POISON, SIGMA_K, SIGMA_Q, _pages

D = 128
CA, CB = 64, 32  # position channels (j % 64), region channels (region j // 64, % 32)
NCH = CA + CB
T_KEY = 8.0

# Bars of attn_close (relative error per (token, q head) row), each 2.2 ... 2.8 x the online model's worst disagreement
# with the pinned oracle over stages of 64 and 128 tokens (tests/test_prefill_bar.py measures it on every run and prints
# it).  Needle inputs over BAR_CASES: model <= 0.78 % = one bf16 ulp of the row's largest element, for fp8 per-tensor, fp8
# per-token K and bf16 alike (the needles are exact maxima: their P is 256 in e4m3 against any running maximum; in bf16
# the oracle's softmax is fp32 and the model rounds P to bf16).  The reference generators (near-uniform softmax, the shapes
# of tests/test_attention_prefill_*.py): 6.4 % (fp8 per-tensor: ragged 4 / 32 heads on pages of 16), 4.5 % (fp8 per-token
# K), 0.78 % (bf16).
TAU_PREFILL_NEEDLE_FP8 = 0.022
TAU_PREFILL_NEEDLE_FP8_KTOK = 0.022
TAU_PREFILL_NEEDLE_BF16 = 0.02
TAU_PREFILL_UNIFORM_FP8 = 0.14
TAU_PREFILL_UNIFORM_FP8_KTOK = 0.12
TAU_PREFILL_UNIFORM_BF16 = 0.02


# the cases the needle bars are calibrated on and the kernels run on (tests/test_attention_prefill_needles.py): name ->
# (seq_q, past, (Hkv, Hq), P, skip ratio of the block mask or None).  "edges": edge_batch(G, P).  The long request and the
# full-length plain prefill run at few heads: the CPU oracle's cost is q heads x q tokens x kv tokens.
BAR_CASES = {
    "edges_g1": ("edges", None, (4, 4), 16, None),
    "edges_g2": ("edges", None, (2, 4), 32, None),
    "edges_g4": ("edges", None, (2, 8), 64, None),
    "edges_g8": ("edges", None, (8, 64), 32, None),
    "edges_g16": ("edges", None, (2, 32), 64, None),
    "long_20k": ([300, 40, 1], [20000, 0, 4097], (1, 4), 64, None),
    "full_4k": ([4000, 7], [0, 1], (1, 8), 64, None),
    "sparse_g4": ([300, 129, 1, 260, 0, 700], [613, 0, 639, 1100, 9, 1], (2, 8), 64, 0.5),
    "sparse_g8": ([300, 129, 1, 260, 0, 700], [613, 0, 639, 1100, 9, 1], (1, 8), 32, 0.9),
    "sparse_g16": ([300, 129, 1, 260, 0, 700], [613, 0, 639, 1100, 9, 1], (1, 16), 16, 0.5),
}


def case_inputs(name, kind="fp8", k_per_token=False, P=None, seed=17):
    seq_q, past, heads, P0, skip = BAR_CASES[name]
    P = P or P0
    if seq_q == "edges":
        seq_q, past = edge_batch(heads[1] // heads[0], P)
    if kind == "bf16c":
        past = [0] * len(seq_q)
    # max_seqlens_q above the longest request; mask columns beyond what the longest request needs
    return needle_inputs(seq_q, past, P, heads, kind, k_per_token, seed, max_seqlens_q=max(seq_q) + 70, skip=skip,
                         extra_cols=3 if skip else 0)


def needle_tau(kind, k_per_token=False):
    if kind.startswith("bf16"):
        return TAU_PREFILL_NEEDLE_BF16
    return TAU_PREFILL_NEEDLE_FP8_KTOK if k_per_token else TAU_PREFILL_NEEDLE_FP8


def edge_batch(G, P):
    """(seq_q, past) of one ragged batch at the edges: seq_q 1, 5, 16/G +- 1, 128/G (one workgroup's positions) and one
    more, 300, a request without q tokens between two others; past 0, 1, not a multiple of 16, multiples of 64 and 128 and
    +- 1; kv lengths 1, P - 1, P, P + 1; a plain prefill (q == kv)."""
    pairs = [(1, 0), (5, 1), (max(1, 16 // G - 1), 13), (16 // G + 1, 63), (128 // G, 64), (128 // G + 1, 65), (0, 50),
             (300, 127), (1, P - 2), (2, P - 2), (3, P - 2), (70, 128), (33, 129), (max(1, 128 // G - 1), 191),
             (150, 256), (300, 0)]
    return [s for s, _ in pairs], [p for _, p in pairs]


def needle_inputs(seq_q, past, P, heads, kind="fp8", k_per_token=False, seed=0, max_seqlens_q=None, skip=None,
                  extra_cols=0):
    """Needle prefill inputs (CPU).  seq_q / past: new and cached tokens per request; kind "fp8" | "bf16" (paged) |
    "bf16c" (contiguous K / V, past all 0, P ignored).  skip: a block mask [B, Hq, ceil(max_seqlens_q / 128), columns]
    with that share of tiles off is added; the tiles from 64 tokens before a q tile's first row to its last row's own
    stay on for every head.  Returns a dict: q, k / v (token rows [pool, P, Hkv, D], or [total, Hkv, D]), k_full /
    v_full (with the scale rows), qscale [B, Hq, pad], kscale, vscale, cu, block_ids, lens (kv tokens incl. the new
    ones), seq_q, past, max_seqlens_q, block_mask."""
    Hkv, Hq = heads
    G = Hq // Hkv
    contiguous = kind == "bf16c"
    seq_q_t, past_t = torch.tensor(seq_q, dtype=torch.int32), torch.tensor(past, dtype=torch.int32)
    lens = seq_q_t + past_t
    B, total_q = len(seq_q), int(seq_q_t.sum())
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = seq_q_t.cumsum(0)
    gen = torch.Generator().manual_seed(seed)
    if contiguous:
        assert int(past_t.sum()) == 0
        block_ids, pool, P = None, total_q, 1
    else:
        block_ids, _, pool, _ = _pages(lens, P, max(4, int(((lens + P - 1) // P).sum()) // 16), gen)
    K = torch.randn(pool * P, Hkv, D, generator=gen) * SIGMA_K
    V = torch.randn(pool * P, Hkv, D, generator=gen) * (1 + 0.5 * (torch.arange(Hkv) % 4))[None, :, None]
    knoise = torch.randn(CA, Hkv, D, generator=gen) * SIGMA_K
    live = torch.zeros(pool * P, dtype=torch.bool)
    q = torch.randn(total_q, Hq, D, generator=gen) * SIGMA_Q
    q[..., : NCH + 1] = 0
    alpha = 0.6 + 0.8 * torch.rand(total_q, Hq, generator=gen)
    inp = dict(cu=cu, block_ids=block_ids, lens=lens, seq_q=seq_q_t, past=past_t, P=P, heads=heads, kind=kind,
               k_per_token=k_per_token, max_seqlens_q=int(max_seqlens_q or max(seq_q)), block_mask=None)
    h = torch.arange(Hq)[None, :]
    odd = (h % G) & 1 == 1
    for b in range(B):
        sq, pa, L = int(seq_q_t[b]), int(past_t[b]), int(lens[b])
        j = torch.arange(L)
        slots = key_slots(inp, b, L)
        live[slots] = True
        kk = knoise[j % CA]
        kk[..., :NCH] = 0
        kk[..., NCH] = 8.0 * 2.0 ** torch.randint(0, 3, (L, Hkv), generator=gen)
        kk[j, :, j % CA] = T_KEY
        kk[j, :, CA + (j // 64) % CB] = T_KEY
        K[slots] = kk
        if sq == 0:
            continue
        p = pa + torch.arange(sq)[:, None]
        shifted = odd & (p + 1 - CA >= 0)
        j1 = torch.where(shifted, p + 1 - CA, p.expand(sq, Hq))
        a = j1 % CA
        own = p // 64
        rnd = (torch.rand(sq, Hq, generator=gen) * (own + 1)).long()
        cand = torch.stack([torch.zeros_like(rnd), torch.full_like(rnd, max(pa - 1, 0) // 64), torch.full_like(rnd, pa // 64),
                            rnd, (own - 1).clamp_min(0).expand(sq, Hq)])
        R = torch.gather(cand, 0, ((p + 3 * h + 7 * b) % 5)[None])[0]
        R = torch.where(64 * R + a > p, R - 1, R)
        R = torch.where(R < 0, j1 // 64, R)
        R = torch.where(shifted, (p + 1) // 64, R)  # odd local heads: key p + 1 is a full match they must not see
        rows = (int(cu[b]) + torch.arange(sq))[:, None]
        val = alpha[int(cu[b]): int(cu[b + 1])] * math.sqrt(D)
        q[rows, h, a] = val
        q[rows, h, CA + (j1 // 64) % CB] = val
        q[rows, h, CA + R % CB] = val
    dead = ~live
    K[dead, :, :NCH] = POISON
    V[dead] *= 4
    if skip is not None:
        nrow = (inp["max_seqlens_q"] + 127) // 128
        ncol = (int(lens.max()) + 127) // 128 + extra_cols
        bm = torch.rand(B, Hq, nrow, ncol, generator=gen) >= skip
        for b in range(B):
            sq, pa = int(seq_q_t[b]), int(past_t[b])
            for r in range((sq + 127) // 128):
                bm[b, :, r, max(0, pa + r * 128 - 64) // 128: (pa + min(sq - 1, r * 128 + 127)) // 128 + 1] = True
        inp["block_mask"] = bm
    if kind != "fp8":
        shape = (pool, Hkv, D) if contiguous else (pool, P, Hkv, D)
        inp["q"], inp["k"], inp["v"] = q.bfloat16(), K.reshape(shape).bfloat16(), V.reshape(shape).bfloat16()
        inp["k_full"], inp["v_full"] = inp["k"], inp["v"]
        return inp
    qs_row = q.abs().amax(-1) / 448
    inp["q"] = (q / qs_row[..., None]).to(F8)
    pad = (inp["max_seqlens_q"] + 127) // 128 * 128 + 128
    qscale = 100 + 10 * torch.rand(B, Hq, pad, generator=gen)
    for b in range(B):
        qscale[b, :, : int(seq_q_t[b])] = qs_row[int(cu[b]): int(cu[b + 1])].t()
    inp["qscale"] = qscale
    K, V = K.reshape(pool, P, Hkv, D), V.reshape(pool, P, Hkv, D)
    if k_per_token:
        from oracle import attention as oattn

        rows = P * 4 // D
        kfull = torch.zeros(pool, P + rows, Hkv, D)
        kfull[:, :P] = K
        inp["k_full"], inp["kscale"] = oattn.quant_paged_cache_pertoken(kfull, P)
        vscale = V.abs().amax((0, 1, 3)) / 448
        vfull = torch.zeros(pool, P + rows, Hkv, D, dtype=F8)
        vfull[:, :P] = (V / vscale[None, None, :, None]).to(F8)
        inp["v_full"], inp["vscale"] = vfull, vscale
    else:
        kscale, vscale = (K.abs().amax() / 448).reshape(1), (V.abs().amax() / 448).reshape(1)
        inp["k_full"], inp["v_full"] = (K / kscale).to(F8), (V / vscale).to(F8)
        inp["kscale"], inp["vscale"] = kscale, vscale
    inp["k"], inp["v"] = inp["k_full"][:, :P], inp["v_full"][:, :P]
    return inp


def key_slots(inp, b, n, block_ids=None):
    """flat (page * P + slot, or row) indices of request b's first n key tokens"""
    j = torch.arange(n)
    if inp["block_ids"] is None:
        return int(inp["cu"][b]) + j
    bids = inp["block_ids"] if block_ids is None else block_ids
    return bids[b, (j // inp["P"]).long()].long() * inp["P"] + j % inp["P"]


def uniform_inputs(kind, seq_q, seq_kv, heads, P, k_per_token=False, seed=10086):
    """the reference tests' generators (tests/test_attention_prefill_fp8.py::make_case with the per-token quantisation of
    test_prefill_fp8_k_per_token, tests/test_attention_prefill_bf16.py::paged_case) in this module's dict"""
    Hkv, Hq = heads
    if kind == "bf16c":  # tests/test_attention_prefill_bf16.py::test_attention_prefill_bf16_contiguous
        g = torch.Generator().manual_seed(seed)
        total = sum(seq_q)
        lens = torch.tensor(seq_q, dtype=torch.int32)
        cu = torch.zeros(len(seq_q) + 1, dtype=torch.int32)
        cu[1:] = lens.cumsum(0)
        return dict(q=(torch.randn(total, Hq, D, generator=g) / math.sqrt(D)).bfloat16(),
                    k=(torch.randn(total, Hkv, D, generator=g) / math.sqrt(D)).bfloat16(),
                    v=torch.randn(total, Hkv, D, generator=g).bfloat16(), cu=cu, block_ids=None, lens=lens, seq_q=lens,
                    past=lens * 0, P=1, heads=heads, kind=kind, k_per_token=False, max_seqlens_q=max(seq_q), block_mask=None)
    seq_q_t, lens = torch.tensor(seq_q, dtype=torch.int32), torch.tensor(seq_kv, dtype=torch.int32)
    inp = dict(lens=lens, seq_q=seq_q_t, past=lens - seq_q_t, P=P, heads=heads, kind=kind, k_per_token=k_per_token,
               max_seqlens_q=max(seq_q), block_mask=None)
    if kind == "bf16":
        from test_attention_prefill_bf16 import paged_case

        inp["q"], kv, inp["cu"], inp["block_ids"], _ = paged_case(seq_q, seq_kv, Hq, Hkv, P, seed)
        inp["k"], inp["v"] = inp["k_full"], inp["v_full"] = kv[:, 0], kv[:, 1]
        return inp
    from oracle import attention as oattn
    from test_attention_prefill_fp8 import make_case

    inp["q"], kv, inp["qscale"], inp["kscale"], inp["vscale"], inp["cu"], inp["block_ids"], _ = make_case(
        seq_q, seq_kv, Hq, Hkv, P, seed)
    inp["k"], inp["v"] = inp["k_full"], inp["v_full"] = kv[:, 0], kv[:, 1]
    if k_per_token:
        rows = P * 4 // D
        raw = torch.randn(kv.shape[0], 2, P + rows, Hkv, D, generator=torch.Generator().manual_seed(5)).bfloat16()
        kc, _ = oattn.quant_paged_cache_pertoken(raw[:, 0], P)
        vc, inp["vscale"] = oattn.quant_paged_cache_perhead(raw[:, 1], P)
        inp["k"], inp["v"], inp["kscale"] = kc[:, :P], vc[:, :P], kc[:, P:]
        inp["k_full"], inp["v_full"] = kc, vc
    return inp


def oracle(inp, pinned=False, **over):
    """the pinned oracle's arithmetic on `inp` (pinned=False: its memory-safe twin, bit-equal); `over` replaces entries of
    `inp` (mutants made by altered inputs)"""
    from oracle import attention as oattn

    c = dict(inp, **over)
    if c["kind"] != "fp8":
        if pinned:
            return oattn.ref_prefill_bf16(c["q"], c["k"], c["v"], c["cu"], c["block_ids"], c["lens"])
        return oattn.ref_prefill_by_kv_head(c["q"], c["k"], c["v"], c["cu"], c["block_ids"], c["lens"])
    if pinned:
        return oattn.ref_prefill_fp8(c["q"], c["k"], c["v"], c["qscale"], c["kscale"], c["vscale"], c["cu"], c["block_ids"],
                                     c["lens"], k_per_token=c["k_per_token"], block_mask=c["block_mask"])
    return oattn.ref_prefill_by_kv_head(c["q"], c["k"], c["v"], c["cu"], c["block_ids"], c["lens"], c["qscale"], c["kscale"],
                                        c["vscale"], c["k_per_token"], c["block_mask"])


def online_model(inp, stage=128, drop=None, causal_shift=0, block_ids=None, kv_head_map=None, q_head_map=None,
                 qscale_index=None, block_mask="inp", mask_row_shift=0, mask_col_shift=0, mask_head_map=None,
                 mask_from_q0=False, mask_first_half_only=False, mask_any_head_off=False, kscale_shift=0,
                 vscale_head_map=None, q_chunk=1024):
    """CPU model of the prefill kernels' online softmax (module docstring) on `inp`; stage None: one stage over the whole
    row = the oracle's arithmetic.  Mutations (tests/test_prefill_bar.py): drop(L, past) -> key positions left out;
    causal_shift: row s sees keys <= past + s + shift (within the request's pages); block_ids / kv_head_map: read these
    pages / kv head kv_head_map[g] for g; q_head_map: head h is computed from the q of head q_head_map[h];
    qscale_index(b, h, pos) -> the (b, h, pos) whose qscale is used; kscale_shift: the per-token K scale of token
    j + shift; vscale_head_map; block_mask (default: the input's) read at row + mask_row_shift, column + mask_col_shift,
    head mask_head_map[h], columns counted from the first q token (mask_from_q0), honoured on the first 64 tokens of a
    column only, the rest attended (mask_first_half_only), or a tile skipped for all heads of a kv head when one of
    them has it off (mask_any_head_off)."""
    fp8 = inp["kind"] == "fp8"
    Hkv, Hq = inp["heads"]
    G, P = Hq // Hkv, inp["P"]
    q, cu = inp["q"], inp["cu"]
    paged = inp["block_ids"] is not None
    Kf, Vf = inp["k"].reshape(-1, Hkv, D), inp["v"].reshape(-1, Hkv, D)
    bm_all = inp["block_mask"] if isinstance(block_mask, str) else block_mask
    if fp8:
        qscale = inp["qscale"]
        if inp["k_per_token"]:
            ks_all = inp["kscale"].contiguous().view(torch.float32)  # [pool, rows, Hkv, 32]: token 32 row + i
    out = torch.empty(q.shape, dtype=torch.bfloat16)
    for b in range(len(inp["lens"])):
        a0, a1 = int(cu[b]), int(cu[b + 1])
        sq, L = a1 - a0, int(inp["lens"][b])
        if sq == 0:
            continue
        pa = L - sq
        Lk = min(L + max(causal_shift, 0), (L + P - 1) // P * P) if paged else L
        slots = key_slots(inp, b, Lk, block_ids)
        col = torch.arange(Lk)
        vis = col[None, :] <= (pa + torch.arange(sq) + causal_shift)[:, None]
        if drop is not None:
            vis[:, drop(L, pa)] = False
        for g in range(Hkv):
            gk = g if kv_head_map is None else kv_head_map[g]
            hs = torch.arange(g * G, (g + 1) * G)
            hq = hs if q_head_map is None else torch.as_tensor(q_head_map)[hs]
            kf, vf = Kf[slots, gk].float(), Vf[slots, gk].float()
            if fp8 and inp["k_per_token"]:
                ktok = ks_all[slots // P, (slots % P) // 32, gk, slots % 32].float()
                if kscale_shift:
                    ktok = torch.roll(ktok, -kscale_shift)
            for c0 in range(0, sq, q_chunk):
                c1 = min(sq, c0 + q_chunk)
                pos = torch.arange(c0, c1)
                s = q[a0 + c0: a0 + c1][:, hq].float().transpose(0, 1) @ kf.t()
                if fp8:
                    bi, hi, pi = (b, hs[:, None], pos[None, :]) if qscale_index is None else qscale_index(
                        b, hs[:, None], pos[None, :])
                    qs = qscale[bi % qscale.shape[0], hi % Hq, torch.as_tensor(pi).clamp(0, qscale.shape[2] - 1)]
                    s = s * qs.unsqueeze(-1) / math.sqrt(D)
                    s = s * (ktok[None, None, :] if inp["k_per_token"] else inp["kscale"][0])
                else:
                    s = s / math.sqrt(D)
                ok = vis[None, c0:c1]
                if bm_all is not None:
                    bm = bm_all[b].bool()
                    hm = hs if mask_head_map is None else torch.as_tensor(mask_head_map)[hs]
                    ri = (pos // 128 + mask_row_shift).clamp(0, bm.shape[1] - 1)
                    cj = (col - pa).clamp_min(0) if mask_from_q0 else col
                    ci = (cj // 128 + mask_col_shift).clamp(0, bm.shape[2] - 1)
                    em = bm[hm][:, ri][:, :, ci]
                    if mask_first_half_only:
                        em = em | (col % 128 >= 64)[None, None, :]
                    if mask_any_head_off:
                        em = em.all(0, keepdim=True).expand(G, -1, -1)
                    ok = ok & em
                s = s.masked_fill(~ok, float("-inf"))
                m = torch.full((G, c1 - c0), float("-inf"))
                l = torch.zeros(G, c1 - c0)
                o = torch.zeros(G, c1 - c0, D)
                T = Lk if stage is None else stage
                for t0 in range(0, Lk, T):
                    st = s[:, :, t0: t0 + T]
                    mn = torch.maximum(m, st.amax(-1))
                    ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
                    w = torch.exp(st - ms[..., None])
                    r = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - ms))
                    wq = (w * 256.0).to(F8).float() if fp8 else w.to(torch.bfloat16).float()
                    l = l * r + w.sum(-1)
                    o = o * r[..., None] + wq @ vf[t0: t0 + T]
                    m = mn
                y = o / l[..., None]
                if fp8:
                    gv = gk if vscale_head_map is None else vscale_head_map[gk]
                    y = y * inp["vscale"][gv] / 256.0 if inp["k_per_token"] else y * (inp["vscale"][0] / 256.0)
                out[a0 + c0: a0 + c1, hs] = y.transpose(0, 1).to(torch.bfloat16)
    return out
