"""The statement of the DSA prefill ops (hpc.mla_indexer_logits_prefill_fp8 / mla_indexer_topk_prefill / mla_indexer_topk_prefill_fp8
and hpc.attention_prefill_mla_sparse_bf16 / _fp8): the existing float64 statements applied to the EXPANDED FORM of a ragged chunk,
the mutants of the row rule, and the one small case the CPU and GPU tests share.

The row rule (the writers', csrc/mla_indexer_dev.h::locate_row): row r of the chunk belongs to the last request b with
q_index[b] <= r, at pos = num_seqlen_per_req[b] - (q_index[b + 1] - r); lengths are totals including the chunk's tokens.  A row at
or past q_index[num_req] or with pos < 0 is a row of no request.  A live row sees vis(r) = min(pos + 1, max_blocks * P) tokens.

The expanded form: B' = R one-row requests, row r's page-table row that of its request, its length pos + 1 (0 for a row of no
request), mtp = 0, lengths included.  On it the statements are tests/mla_indexer_ref.py::logits_statement / topk_statement and
tests/mla_sparse_ref.py::sparse_statement, imported, not restated."""
import torch

import mla_indexer_ref as ir
import mla_sparse_ref as sr

# the case: the smallest that reaches every edge.  New rows and cached context per request; the last request's total length is 2
# for its 4 rows, so its first two rows are rows of no request; three pad rows follow q_index[-1].
CASE_NEW = [1, 2, 15, 16, 17, 33, 70, 0, 4]
CASE_CTX = [0, 5, 63, 300, 2100, 0, 17, 40, -2]
PAD_ROWS = 3
CONFIGS = [(16, 16), (64, 16), (16, 64), (64, 64)]  # (Hi, P)


def row_rule(lens_total, q_index, row, *, pos_delta=0, prev_row=False, pad_live=False):
    """(request, pos, live) of row `row`.  Mutations, all off by default: pos_delta moves the position; prev_row gives the row
    the request and position of the row before it; pad_live treats the rows past q_index[-1] as rows of the last request."""
    if prev_row and row > 0:
        row -= 1
    num_req = len(lens_total)
    live = row < int(q_index[num_req]) or pad_live
    b = 0
    while b + 1 < num_req and int(q_index[b + 1]) <= row:
        b += 1
    pos = int(lens_total[b]) - (int(q_index[b + 1]) - row) + pos_delta
    return b, pos, live and pos >= 0


def expand(block_ids, lens_total, q_index, num_rows, row_begin=0, *, ignore_row_begin=False, **mutation):
    """the expanded form of rows row_begin .. row_begin + num_rows - 1: (block_ids [R, max_blocks], lengths int32 [R], the
    request of every row).  ignore_row_begin (a mutant): the rows are taken as rows 0 .. of the chunk."""
    rows = [row_rule(lens_total, q_index, (0 if ignore_row_begin else row_begin) + r, **mutation) for r in range(num_rows)]
    req = torch.tensor([b for b, _, _ in rows], dtype=torch.long)
    lens = torch.tensor([pos + 1 if live else 0 for _, pos, live in rows], dtype=torch.int32)
    return block_ids[req].contiguous(), lens, req


def logits_statement(inp, row_begin=0, num_rows=None, **mutation):
    """float64 [R, max_blocks * P] of rows row_begin .. of the chunk; NaN marks a column the op does not write"""
    R = inp["T"] - row_begin if num_rows is None else num_rows
    bid, lens, _ = expand(inp["block_ids"], inp["lens_total"], inp["q_index"], R, row_begin, **mutation)
    return ir.logits_statement(inp["q"][row_begin: row_begin + R], inp["weights"][row_begin: row_begin + R], inp["k_cache"], bid,
                               lens, 1)


def topk_statement(logits, inp, topk, row_begin=0, **mutation):
    """int32 [R, topk] for the logits of rows row_begin .. of the chunk"""
    _, lens, _ = expand(inp["block_ids"], inp["lens_total"], inp["q_index"], logits.shape[0], row_begin, **mutation)
    return ir.topk_statement(logits, lens, 1, topk)


def sparse_statement(q, ckv, inp, indices, scale):
    """(out float64 [T, H, 512], lse float64 [T, H]) of the token-sparse attention of the chunk"""
    bid, lens, _ = expand(inp["block_ids"], inp["lens_total"], inp["q_index"], q.shape[0])
    return sr.sparse_statement(q, ckv, bid, lens, indices, 1, scale)


ROW_RULE_MUTANTS = {
    "pos off by one": dict(pos_delta=1),
    "the previous row's request": dict(prev_row=True),
    "row_begin ignored": dict(ignore_row_begin=True),
    "pad rows treated as live": dict(pad_live=True),
}


def chunk_of(new, ctx, pad_rows):
    """(total lengths int32 [num_req], q_index int32 [num_req + 1], rows of the chunk with its pad rows)"""
    lens_total = torch.tensor([c + n for c, n in zip(ctx, new)], dtype=torch.int32)
    q_index = torch.tensor([0] + torch.tensor(new).cumsum(0).tolist(), dtype=torch.int32)
    return lens_total, q_index, int(q_index[-1]) + pad_rows


def inputs(Hi, P, *, exact, new=CASE_NEW, ctx=CASE_CTX, pad_rows=PAD_ROWS, seed=0):
    """The case: the cache, the page table (one column wider than the longest request, one poisoned page id per request) and
    the value ranges of mla_indexer_ref.inputs(exact=...), with q and weights for every row of the chunk."""
    lens_total, q_index, T = chunk_of(new, ctx, pad_rows)
    base = ir.inputs(Hi, 0, P, exact=exact, lens_total=lens_total.tolist(), seed=seed)
    gen = torch.Generator().manual_seed(seed + 7 + 1000 * Hi + P)
    if exact:
        q = torch.randint(-8, 9, (T, Hi, ir.DIM), generator=gen).float().to(ir.F8)
        weights = torch.randint(-8, 9, (T, Hi), generator=gen).float()
    else:
        raw = torch.randint(0, 256, (T, Hi, ir.DIM), generator=gen, dtype=torch.int32)
        raw[(raw & 0x7F) == 0x7F] = 0x38  # the two NaN codes -> 1.0
        q = raw.to(torch.uint8).view(ir.F8)
        weights = torch.randn(T, Hi, generator=gen)
    return dict(q=q, weights=weights, k_cache=base["k_cache"], block_ids=base["block_ids"], lens_total=lens_total, q_index=q_index,
                T=T, P=P, Hi=Hi, dead=base["dead"])


def absolute_statement(inp):
    """A of the logits bar (mla_indexer_ref: absolute values everywhere, no ReLU) on the expanded form"""
    bid, lens, _ = expand(inp["block_ids"], inp["lens_total"], inp["q_index"], inp["T"])
    return ir.logits_statement(inp["q"], inp["weights"], inp["k_cache"], bid, lens, 1, absolute=True)
