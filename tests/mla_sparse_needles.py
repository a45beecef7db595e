"""Lists on top of the dense needle inputs (tests/mla_needles.py, imported, not edited), and a CPU model of the split-list
arithmetic, for hpc.attention_decode_mla_sparse_bf16 / _fp8.  The statement is tests/mla_sparse_ref.py.

Lists.  For q row (b, s) the candidate needle positions of mla_needles.needle_inputs (one of them holds the needle of every head)
sit at the EDGE slots of the list - 63, 64, the last valid slot, 0, 65, the piece ends of 2, 3 and 8 splits of topk and their
neighbours - each position once; the heads' own needles are placed first, so a lost edge slot loses a head's needle.  The rest of
the list is a random sample of other visible positions, and between them, in interior slots, the TRAPS, each of which dominates
the row or faults if it is read:
  -1, other negatives, INT32_MIN;
  vis(b, s) - row s + 1's new token, which holds poison in row s's columns (for the last row: the first slot of the page tail);
  positions in the last page's tail (poison);
  positions >= max_blocks * P, 2^30 + 3 and INT32_MAX;
  for one request a page in the middle of its table whose block_ids entry is overwritten with the -999999 padding, and for
  another one whose entry is num_blocks + 7: the positions on those pages are listed and must contribute nothing.
A list shorter than topk (a request with few visible tokens) ends in -1 padding.

Split model: mla_needles.split_model's arithmetic over the list's slots - invalid slots kept as -inf (and zero rows) so that the
tiles of 64 slots and the pieces fall where the kernel's do.

Bars: mla_needles.TAU_NEEDLE on `out` and mla_needles.LSE_BAR_NEEDLE on `lse`.  Measured with this model on the calibration cases
of tests/test_attention_decode_mla_sparse.py over piece lengths 64 .. 2048: see test_split_model_within_bars, which measures
them again on every run, prints them and asserts model <= bar."""
import math

import torch

import mla_needles as mn
import mla_sparse_ref as sr

DIM, DIM_V = sr.DIM, sr.DIM_V
PAD_PAGE = -999999
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
PIECE_LENS = (64, 128, 256, 512, 1024, 2048)


def list_piece_len(topk, splits):
    """slots per piece: ceil(topk / splits) rounded up to the kernel's tile of 64 slots"""
    return (-(-topk // splits) + mn.KV_TILE - 1) // mn.KV_TILE * mn.KV_TILE


def effective_splits(topk, splits):
    return -(-topk // list_piece_len(topk, splits))


def candidates(lb, s, sq, P):
    """the `cands` of mla_needles.needle_inputs for row s of a request with lb tokens before the step"""
    L, vis = lb + sq, lb + s + 1
    cands = [0, P - 1, P, P + 1, 63, 64, 65, lb - 1, lb + s]
    for splits in (2, 3, 8):
        bd = mn.piece_len(L, splits)
        cands += [bd - 1, bd, bd + 1, 2 * bd - 1, 2 * bd]
    return sorted({p for p in cands if 0 <= p < vis})


def edge_slots(topk, n):
    """the edge slots of a list whose first n slots are in use, most telling first"""
    slots = [63, 64, n - 1, 0, 65]
    for splits in (2, 3, 8):
        pl = list_piece_len(topk, splits)
        slots += [pl - 1, pl, pl + 1, 2 * pl - 1, 2 * pl]
    seen, out = set(), []
    for k in slots:
        if 0 <= k < n and k not in seen:
            seen.add(k)
            out.append(k)
    return out


def sparse_needle_inputs(lens_before, num_seq_q, P, H, topk, seed=0):
    """mla_needles.needle_inputs plus `indices` int32 [B * Sq, topk], `topk`, and block_ids with two poisoned entries (module
    docstring)."""
    inp = mn.needle_inputs(lens_before, num_seq_q, P, H, seed)
    sq = num_seq_q
    B = len(inp["lens_total"])
    gen = torch.Generator().manual_seed(seed + 7919)
    block_ids = inp["block_ids"].clone()
    max_blocks, pool = block_ids.shape[1], inp["ckv"].shape[0]
    # poisoned page ids: the two requests with the most pages, a page in the middle that holds no candidate of any row
    all_cands = [set().union(*(candidates(int(inp["lens_before"][b]), s, sq, P) for s in range(sq))) for b in range(B)]
    dead = {}
    for b, bad in zip(sorted(range(B), key=lambda i: -int(inp["nblocks"][i]))[:2], (PAD_PAGE, pool + 7)):
        nb = int(inp["nblocks"][b])
        free = [pg for pg in range(1, nb - 1) if not any(c // P == pg for c in all_cands[b])]
        if free:
            dead[b] = free[len(free) // 2]
            block_ids[b, dead[b]] = bad
    indices = torch.full((B * sq, topk), -1, dtype=torch.int32)
    for b in range(B):
        lb, L = int(inp["lens_before"][b]), int(inp["lens_total"][b])
        tail_end = -(-L // P) * P
        for s in range(sq):
            vis = lb + s + 1
            cands = candidates(lb, s, sq, P)
            own = sorted({cands[(h + 3 * s + 7 * b) % len(cands)] for h in range(H)})
            traps = [-1, -7, INT32_MIN, vis, max_blocks * P, max_blocks * P + 5, 2 ** 30 + 3, INT32_MAX, -1]
            traps += [t for t in (L, tail_end - 1) if L <= t < tail_end]
            if b in dead:
                traps += [dead[b] * P, dead[b] * P + P - 1]
            taken = set(cands)
            others = [p for p in torch.randperm(vis, generator=gen).tolist() if p not in taken]
            needles = own + [c for c in cands if c not in own]  # the heads' own needles take the most telling slots
            assert len(needles) + len(traps) <= topk, "every candidate and every trap must fit the list"
            n = min(topk, len(needles) + len(traps) + len(others))
            row = [None] * n
            edges = edge_slots(topk, n)
            for k, pos in zip(edges, needles):
                row[k] = pos
            interior = [k for k in range(n) if row[k] is None]
            fill = (needles[len(edges):] + traps + others)[: len(interior)]
            for j, pos in zip(torch.randperm(len(interior), generator=gen).tolist(), fill):
                row[interior[j]] = pos
            assert None not in row and all(p in row for p in needles), (b, s)
            indices[b * sq + s, :n] = torch.tensor(row, dtype=torch.int64).to(torch.int32)
    return dict(inp, block_ids=block_ids, indices=indices, topk=topk, dead_pages=dead)


def statement(inp, **mutation):
    """(out bf16, lse float64) of the float64 statement on `inp`; keyword arguments are mla_sparse_ref.sparse_statement's mutations"""
    out, lse = sr.sparse_statement(inp["q"], inp["ckv"], inp["block_ids"], inp["lens_total"], inp["indices"], inp["num_seq_q"],
                                   inp["scale"], **mutation)
    return out.to(torch.bfloat16), lse


def split_model(inp, plen):
    """(out bf16 [B * Sq, H, 512], lse float32 [B * Sq, H]) of the split model of mla_needles over each row's list, cut into
    pieces of `plen` slots.  Invalid slots are zero rows with a score of -inf, in place."""
    sq, H, topk = inp["num_seq_q"], inp["H"], inp["topk"]
    R = inp["indices"].shape[0]
    out = torch.zeros(R, H, DIM_V, dtype=torch.bfloat16)
    lse = torch.full((R, H), float("-inf"), dtype=torch.float32)
    k2 = torch.tensor(inp["scale"], dtype=torch.float32) * torch.tensor(math.log2(math.e), dtype=torch.float32)
    ln2 = torch.tensor(math.log(2.0), dtype=torch.float32)
    n = -(-topk // plen)
    pad = n * plen - topk
    for r in range(R):
        b, s = divmod(r, sq)
        c, valid = sr.gather_list(inp["ckv"], inp["block_ids"][b], inp["indices"][r], sr.vis_of(inp["lens_total"], sq, b, s))
        c = c.float()
        qf = inp["q"][r].float()
        t = torch.zeros(H, topk, dtype=torch.float32)
        for k in range(DIM):  # the column-ordered chain of fp32 multiply-adds of mla_needles.split_model
            t = t + qf[:, k, None] * c[None, :, k]
        t = (t * k2).masked_fill(~valid[None, :], float("-inf"))
        tr = torch.nn.functional.pad(t, (0, pad), value=float("-inf")).reshape(H, n, plen)
        vr = torch.nn.functional.pad(c[:, :DIM_V], (0, 0, 0, pad)).reshape(n, plen, DIM_V)
        m = tr.amax(-1)
        ms = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        w = torch.exp2(tr - ms[..., None])
        lsum = w.sum(-1)
        o = torch.einsum("hnt,ntd->hnd", w.to(torch.bfloat16).float(), vr)
        M = m.amax(-1, keepdim=True)
        if bool(torch.isinf(M).all()):
            continue  # no valid entry: zeros and -inf
        a = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - M))
        den = (a * lsum).sum(-1, keepdim=True)
        out[r] = ((a[..., None] * o).sum(1) / den).to(torch.bfloat16)
        lse[r] = ((M + torch.log2(den)) * ln2)[..., 0]
    return out, lse


def lse_err(ref64, got):
    """worst |got - ref| of an lse; -inf where the reference has -inf is no error, NaN counts as infinite"""
    g = got.double().cpu()
    same_inf = torch.isinf(ref64) & (g == ref64)
    d = torch.where(same_inf, torch.zeros_like(g), (g - ref64).abs())
    return float(d.nan_to_num(nan=float("inf")).max())
