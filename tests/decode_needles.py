"""Needle inputs and a CPU model of split-K decode arithmetic, for the decode-attention parity tests.

Why: with the reference tests' generators (randn K / sqrt(d), randn V) the softmax is almost uniform and the output is
an average of V over the whole context, |y| ~ 1e-3 ... 2e-2 - an absolute atol of 0.1 / 0.2 accepts an all-zero answer.
Here every (request, q row, q head) gets its own key direction, planted at one position (an "edge needle": token 0,
P - 1, P, multiples of 1024 +- 1, the middle, the last cached token, the row's own new token) or as a comb of equal-score
needles every 8 P tokens; the needle takes a large share of the softmax, so |y| ~ 1 and losing, doubling or misplacing
it moves that row by O(1) of its own scale (tests/utils.py::attn_close).

Poison (all finite): the slots of each request's last page past its length, and every pool page outside all block
tables, hold keys that would dominate every head if they were read, with large V; with num_seq_q > 1 row s + 1's new
token holds a key that dominates row s, which row s must not see (causal mask).  NaN bytes in page tails are NOT
used: in the reference kernel (sm90 decode, apply_casual_mask_with_scale) the mask replaces the SCORE of a token past
the length with -inf, but the P V product still multiplies that token's P = 0 with its V tile, and 0 * NaN = NaN - so
a NaN V in a page tail is not defined behaviour there, and it is not a contract of this project's kernels either.

The split model restates how the kernels compute: a per-range maximum m_r, P = e4m3(256 exp(s - m_r)) (fp8) or
bf16(exp(s - m_r)) (bf16), a per-range fp32 sum of the unrounded exponentials, an lse merge of the ranges and a bf16
result; the pinned oracles round P against the request's global maximum instead.  The bars (TAU_*) are set from this
model's worst disagreement with the oracles over range lengths 16 ... 4096 (tests/test_attn_bar.py asserts that the
model stays within them and that they are at most 3 x that worst case)."""
import math

import torch

D = 128
F8 = torch.float8_e4m3fn
SIGMA_Q, SIGMA_K = 0.3, 0.5   # background q / K noise (per coordinate); background logits have std ~0.5
POISON = 40.0                 # a poison key coordinate: logit 40 alpha >= 20, above every needle (ln 131072 + 2 < 14)
RANGE_LENS = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)

# Bars of attn_close (relative error per (request, row, head)), each 2.3 ... 3 x the split model's worst disagreement
# with the oracle (tests/test_attn_bar.py measures it on every run and prints it).  Needle inputs: model <= 0.9 % (fp8
# per-tensor), 2.8 % (fp8 per-token K: pages of 32 at 8 / 64 heads), 0.8 % (bf16, where P is rounded to bf16 and the
# oracle's softmax is fp32); the reference generators (near-uniform softmax, |y| ~ 1e-3): <= 4.7 % (fp8 per-tensor), 6 %
# (fp8 per-token K), 0.8 % (bf16).
TAU_NEEDLE_FP8 = 0.026
TAU_NEEDLE_FP8_KTOK = 0.07
TAU_NEEDLE_BF16 = 0.02
TAU_UNIFORM_FP8 = 0.12
TAU_UNIFORM_FP8_KTOK = 0.15
TAU_UNIFORM_BF16 = 0.02

# the reference benchmark's named decode cases (benchmark/attention_decode/bench_attention_decode_fp8.py:57-67;
# tools/suite.py), total tokens per request including the new ones
NAMED_CASES = {
    "skewed_mix": [128] * 32 + [4096] * 32,
    "skewed_extreme": [64] * 15 + [16384],
    "two_32k_30x4k": [32768] * 2 + [4096] * 30,
    "one_64k_31x4k": [65536] + [4096] * 31,
    "one_128k_31x4k": [131072] + [4096] * 31,
    "uniform_512": [512] * 64,
}


def needle_tau(kind, k_per_token):
    return TAU_NEEDLE_BF16 if kind == "bf16" else TAU_NEEDLE_FP8_KTOK if k_per_token else TAU_NEEDLE_FP8


def edge_lens(P, num_seq_q):
    """cached-token counts (before the Sq new ones) at the edges: empty cache, 1 token, multiples of P and +-1, a request
    split over many ranges"""
    base = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 3 * P, 1023, 1024, 1025, 4 * P + 1, 5000, 9000 - num_seq_q, 20000]
    return torch.tensor(base, dtype=torch.int32)


def _pages(lens_total, P, spare, gen):
    nblocks = (lens_total + P - 1) // P
    used = int(nblocks.sum())
    pool = used + spare
    perm = torch.randperm(pool, generator=gen).to(torch.int32)
    block_ids = torch.full((len(lens_total), max(1, int(nblocks.max()))), -999999, dtype=torch.int32)
    off = 0
    for i, nb in enumerate(nblocks.tolist()):
        block_ids[i, :nb] = perm[off: off + nb]
        off += nb
    return block_ids, nblocks, pool, perm[used:]


def _plan(lens_before, Sq, P, heads, gen, combs):
    """needle / poison positions.  Returns lists of (request, token, kv head, coordinate, key value) and the per
    (q row, q head) weights alpha of the own coordinate of q."""
    Hkv, Hq = heads
    G = Hq // Hkv
    B = len(lens_before)
    alpha = 0.5 + torch.rand(B * Sq, Hq, generator=gen)  # the own-coordinate size: q scales differ per row and head
    keys = []
    for b in range(B):
        lb = int(lens_before[b])
        for s in range(Sq):
            vis = lb + s + 1
            for h in range(Hq):
                g, hg = divmod(h, G)
                j = s * G + hg
                a = float(alpha[b * Sq + s, h])
                c = 0.3 + 1.9 * float(torch.rand(1, generator=gen))  # the needle takes ~54 ... 89 % of the softmax
                if combs and h % 4 == 3 and vis >= 16 * P:
                    phase = (37 * h + 11 * s + 5 * b) % (8 * P)
                    pos = list(range(phase, vis, 8 * P))
                    t = (math.log(vis / len(pos)) + c) / a
                    keys += [(b, p, g, j, t) for p in pos]
                    continue
                cands = [0, P - 1, P, vis // 2, lb - 1, lb + s]
                for k in range(1, vis // 1024 + 1):
                    cands += [1024 * k - 1, 1024 * k + 1]
                cands = [p for p in cands if 0 <= p < vis]
                pos = cands[(h + 3 * s + 7 * b) % len(cands)]
                keys.append((b, pos, g, j, (math.log(vis) + c) / a))
            if s + 1 < Sq:  # row s + 1's new token: dominates row s if row s could see it
                for hg in range(G):
                    for g in range(Hkv):
                        keys.append((b, lb + s + 1, g, s * G + hg, POISON))
    return keys, alpha


def needle_inputs(lens_before, num_seq_q, P, heads, kind="fp8", k_per_token=False, seed=0, device="cpu", combs=True):
    """Needle decode inputs.  lens_before: int32 [B] cached tokens before the num_seq_q new ones.  kind "fp8" | "bf16".
    Returns a dict of DEVICE tensors: q, kv [pool, 2, P (+ scale rows), Hkv, D] (the layout of
    tests/test_attention_decode_fp8.py::_run), k_scale (per-tensor [1] or the tail-row view), v_scale, q_scale, plus
    CPU block_ids, nblocks, lens_before, lens_total and the plan's spare pool pages."""
    Hkv, Hq = heads
    G, Sq = Hq // Hkv, num_seq_q
    assert Sq * G <= 32 and D >= 32
    lens_before = lens_before.to(torch.int32).cpu()
    lens_total = lens_before + Sq
    gen = torch.Generator().manual_seed(seed)
    block_ids, nblocks, pool, spare = _pages(lens_total, P, max(4, int(nblocks_sum(lens_total, P)) // 16), gen)
    keys, alpha = _plan(lens_before, Sq, P, heads, gen, combs)
    dgen = torch.Generator(device=device).manual_seed(seed)
    K = torch.randn(pool, P, Hkv, D, generator=dgen, device=device) * SIGMA_K
    V = torch.randn(pool, P, Hkv, D, generator=dgen, device=device)
    # poison: the tail slots of every request's last page, every spare page
    npos = Sq * G
    tails = [(int(block_ids[b, nb - 1]), int(lens_total[b]) - (nb - 1) * P) for b, nb in enumerate(nblocks.tolist())]
    for page, first in tails:
        if first < P:
            K[page, first:, :, :npos] = POISON
            V[page, first:] *= 4
    if len(spare):
        sp = spare.long().to(device)
        K[sp, :, :, :npos] = POISON
        V[sp] *= 4
    if keys:
        kt = torch.tensor([(int(block_ids[b, t // P]), t % P, g, j) for b, t, g, j, _ in keys], dtype=torch.long)
        vals = torch.tensor([v for *_, v in keys], dtype=torch.float32, device=device)
        kt = kt.to(device)
        K[kt[:, 0], kt[:, 1], kt[:, 2]] = 0  # a needle key is its planted coordinates alone: the needles of a comb are
        K[kt[:, 0], kt[:, 1], kt[:, 2], kt[:, 3]] = vals  # the same bytes, so equal scores (exact maxima in e4m3)
    q = torch.randn(len(lens_total) * Sq, Hq, D, generator=dgen, device=device) * SIGMA_Q
    q[:, :, :npos] = 0  # no cross-talk with the other rows' / heads' needle coordinates
    own = torch.tensor([(r, h, (r % Sq) * G + h % G) for r in range(len(lens_total) * Sq) for h in range(Hq)],
                       dtype=torch.long, device=device)
    q[own[:, 0], own[:, 1], own[:, 2]] = (alpha.to(device) * math.sqrt(D)).reshape(-1)
    out = dict(block_ids=block_ids, nblocks=nblocks, lens_before=lens_before, lens_total=lens_total, spare=spare,
               num_seq_q=Sq, P=P, heads=heads, kind=kind, k_per_token=k_per_token)
    if kind == "bf16":
        out["q"] = q.to(torch.bfloat16)
        out["kv"] = torch.stack([K, V], 1).to(torch.bfloat16)
        return out
    q_scale = q.abs().amax(-1) / 448
    out["q"], out["q_scale"] = (q / q_scale[:, :, None]).to(F8), q_scale
    rows = P * 4 // D if k_per_token else 0
    kv = torch.zeros(pool, 2, P + rows, Hkv, D, dtype=F8, device=device)
    if k_per_token:
        from oracle import attention as oattn

        kfull = torch.zeros(pool, P + rows, Hkv, D, device=device)
        kfull[:, :P] = K
        kv[:, 0], _ = oattn.quant_paged_cache_pertoken(kfull, P)
        out["k_scale"] = kv[:, 0, P:]
        v_scale = V.abs().amax((0, 1, 3)) / 448
        kv[:, 1, :P] = (V / v_scale[None, None, :, None]).to(F8)
    else:
        k_scale = (K.abs().amax() / 448).reshape(1)
        v_scale = (V.abs().amax() / 448).reshape(1)
        kv[:, 0] = (K / k_scale).to(F8)
        kv[:, 1] = (V / v_scale).to(F8)
        out["k_scale"] = k_scale
    out["kv"], out["v_scale"] = kv, v_scale
    return out


def nblocks_sum(lens_total, P):
    return int(((lens_total + P - 1) // P).sum())


def uniform_inputs_fp8(lens_before, num_seq_q, P, heads, k_per_token, seed=41):
    """the reference tests' generator (tests/test_attention_decode_fp8.py::_case + _run's quantisation), CPU"""
    from oracle import attention as oattn
    from test_attention_decode_fp8 import _case

    q8, q_scale, kv, block_ids, nblocks = _case(len(lens_before), num_seq_q, lens_before, P, heads, k_per_token, seed)
    if k_per_token:
        kc, _ = oattn.quant_paged_cache_pertoken(kv[:, 0], P)
        vc, v_scale = oattn.quant_paged_cache_perhead(kv[:, 1], P)
        kv8 = torch.empty_like(kv, dtype=F8)
        kv8[:, 0], kv8[:, 1] = kc, vc
        k_scale = kv8[:, 0, P:]
    else:
        kv8 = kv.to(F8)
        k_scale, v_scale = torch.rand(1) + 0.1, torch.rand(1) + 0.1
    return dict(q=q8, q_scale=q_scale, kv=kv8, k_scale=k_scale, v_scale=v_scale, block_ids=block_ids, nblocks=nblocks,
                lens_before=lens_before, lens_total=lens_before + num_seq_q, num_seq_q=num_seq_q, P=P, heads=heads,
                kind="fp8", k_per_token=k_per_token)


def cpu(inp, key):
    t = inp.get(key)
    return t.cpu() if isinstance(t, torch.Tensor) else t


def oracle(inp, rows=None, literal_qscale_row=False):
    """the pinned oracle on `inp` (CPU), [len(rows), Sq, Hq, D]"""
    from oracle import attention as oattn

    P = inp["P"]
    kv = cpu(inp, "kv")[:, :, :P]
    if inp["kind"] == "bf16":
        return oattn.ref_attn_by_kv_head(cpu(inp, "q"), kv, inp["block_ids"], inp["num_seq_q"], inp["lens_total"], rows)
    return oattn.ref_attn_by_kv_head(cpu(inp, "q"), kv, inp["block_ids"], inp["num_seq_q"], inp["lens_total"], rows,
                                     cpu(inp, "q_scale"), cpu(inp, "k_scale"), cpu(inp, "v_scale"), inp["k_per_token"],
                                     literal_qscale_row)


def split_model(inp, range_len=None, rows=None, drop=None, causal_shift=0, range_mult=None, block_ids=None,
                kv_head_map=None):
    """CPU model of split-K decode (module docstring) on `inp`, per kv head.  range_len None: one range (fp8: the oracle's
    arithmetic, bit for bit).  Mutations (for tests/test_attn_bar.py): drop(seqlen) -> token positions left out;
    causal_shift: row s sees tokens <= len - Sq + s + shift; range_mult (index, factor): that range of every request
    is counted `factor` times; block_ids / kv_head_map: read these pages / kv head kv_head_map[g] for head g."""
    fp8 = inp["kind"] == "fp8"
    q, kvc = cpu(inp, "q"), cpu(inp, "kv")
    P, sq = inp["P"], inp["num_seq_q"]
    Hkv, Hq = inp["heads"]
    G = Hq // Hkv
    bids = inp["block_ids"] if block_ids is None else block_ids
    lens = inp["lens_total"]
    rows = range(len(lens)) if rows is None else rows
    qb = q.reshape(len(lens), sq, Hq, D)
    if fp8:
        qs = cpu(inp, "q_scale").reshape(len(lens), sq, Hq)
        ks, vs = cpu(inp, "k_scale"), cpu(inp, "v_scale")
    out = torch.empty(len(rows), sq, Hq, D, dtype=torch.bfloat16)
    for oi, bi in enumerate(rows):
        L = int(lens[bi])
        blk = bids[bi, : (L + P - 1) // P].long()
        pos = torch.arange(L)
        causal = pos[None, :] <= (L - sq + torch.arange(sq) + causal_shift)[:, None]
        if drop is not None:
            for t in drop(L):
                causal[:, t] = False
        R = L if range_len is None else range_len
        nr = (L + R - 1) // R
        for g in range(Hkv):
            gk = g if kv_head_map is None else kv_head_map[g]
            hs = slice(g * G, (g + 1) * G)
            qf = qb[bi, :, hs].transpose(0, 1).float()
            kf = kvc[blk, 0, :P, gk].reshape(-1, D)[:L].float()
            vf = kvc[blk, 1, :P, gk].reshape(-1, D)[:L].float()
            p = qf @ kf.unsqueeze(0).expand(G, -1, -1).transpose(-1, -2) / math.sqrt(D)
            if fp8:
                p = p * qs[bi][:, hs].transpose(0, 1)[:, :, None]
                if inp["k_per_token"]:
                    p = p * ks[blk].contiguous().view(torch.float32)[:, :, gk].reshape(-1)[:L].float()[None, None, :]
                else:
                    p = p * ks
            p = p.masked_fill(~causal.unsqueeze(0), float("-inf"))
            pad = nr * R - L
            pr = torch.nn.functional.pad(p, (0, pad), value=float("-inf")).reshape(G, sq, nr, R)
            vr = torch.nn.functional.pad(vf, (0, 0, 0, pad)).reshape(nr, R, D)
            m = pr.amax(-1)
            ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            w = torch.exp(pr - ms[..., None])
            lsum = w.sum(-1)
            wq = (w * 256.0).to(F8).float() if fp8 else w.to(torch.bfloat16).float()
            o = torch.einsum("gsrt,rtd->gsrd", wq, vr)
            M = m.amax(-1, keepdim=True)
            a = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - M))
            if range_mult is not None and -nr <= range_mult[0] < nr:
                a[..., range_mult[0]] *= range_mult[1]
            if range_len is None:  # the oracle's operation order
                y = o[:, :, 0] / lsum
                y = y * (vs[gk] / 256.0 if inp["k_per_token"] else vs / 256.0) if fp8 else y
            else:
                y = (a[..., None] * o).sum(2) / (a * lsum).sum(-1, keepdim=True)
                y = y * (vs[gk] / 256.0 if inp["k_per_token"] else vs / 256.0) if fp8 else y
            out[oi, :, hs] = y.transpose(0, 1).to(torch.bfloat16)
    return out
