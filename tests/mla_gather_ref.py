"""The statement of hpc.mla_gather_ckv / hpc.mla_gather_ckv_fp8 on CPU tensors, the knobs the tests turn to make mutants of it,
and the builder of the cases the GPU tests run (tests/test_mla_gather.py checks on the CPU that those cases tell every mutant
from the statement).

    request b owns output rows cu_seqlens[b] <= r < cu_seqlens[b + 1]; row r is the token at
    pos = seq_starts[b] + (r - cu_seqlens[b])                                            (seq_starts None: zeros)

    bf16 cache [num_blocks, P, 576]:   out[r, :]    = cache[block_ids[b, pos // P], pos % P, :]        the bits, untouched
    FP8 cache  [num_blocks, P, 656]:   out[r, :]    = mla_fp8_ref.dequantise(cache[block_ids[b, pos // P], pos % P, :])
                                       i.e. out[r, d] = bf16_rne(fp32(code[d]) * scale[d // 128]) for d < 512 and
                                       out[r, 512:] = the 64 bf16 at byte offset 528, untouched

    rows of no request are not written; a row of a request with pos < 0, pos // P >= max_blocks or a page id outside
    [0, num_blocks) is written as 576 zeros.

The gather itself holds no float: rows are addressed with integers and moved as int16 / uint8.  The only arithmetic is
mla_fp8_ref.dequantise on the fetched FP8 row.  Everything is compared as int16."""
from types import SimpleNamespace

import torch

import mla_fp8_ref as f8

WIDTH = 576
ZERO, UNWRITTEN = "zero", None
INT32_MAX = 2 ** 31 - 1
SENTINEL = 0x7B3D  # int16 pattern of the output buffer before the call (a finite bf16)


def sources(block_ids, cu_seqlens, seq_starts, num_rows, P, num_blocks, *, ignore_starts=False, page_edge_off_by_one=False,
            slot_is_row_offset=False, next_table_row=False):
    """per output row: (page id, slot), ZERO or UNWRITTEN.  Mutations, all off by default: ignore_starts takes seq_starts for
    zeros; page_edge_off_by_one takes the table column (pos + 1) // P (wrong on a page's last slot only); slot_is_row_offset takes
    the row's offset within its request for pos in pos % P; next_table_row reads request (b + 1) % B's row of block_ids."""
    B, max_blocks = block_ids.shape
    cu = [int(x) for x in cu_seqlens]
    st = [0] * B if (seq_starts is None or ignore_starts) else [int(x) for x in seq_starts]
    src = [UNWRITTEN] * num_rows
    for b in range(B):
        for r in range(max(cu[b], 0), min(cu[b + 1], num_rows)):
            pos = st[b] + (r - cu[b])
            col = ((pos + 1) if page_edge_off_by_one else pos) // P
            if pos < 0 or col >= max_blocks:
                src[r] = ZERO
                continue
            page = int(block_ids[(b + 1) % B if next_table_row else b, col])
            src[r] = (page, ((r - cu[b]) if slot_is_row_offset else pos) % P) if 0 <= page < num_blocks else ZERO
    return src


def dequantise_mutant(row_u8, *, scale_shift=0, truncate=False, rope_at=f8.ROPE_AT):
    """mla_fp8_ref.dequantise of uint8 [..., 656] with knobs: scale_shift takes the scale of group (d // 128 + shift) % 4,
    truncate cuts the product to bf16 instead of rounding to nearest even, rope_at reads k_pe from another byte offset.  With
    the defaults it IS mla_fp8_ref.dequantise (asserted by the tests)."""
    codes, scales, _ = f8.unpack(row_u8)
    scales = torch.roll(scales, -scale_shift, -1)
    prod = codes.float().view(*codes.shape[:-1], f8.GROUPS, 128) * scales.unsqueeze(-1)
    if truncate:
        lat = (prod.contiguous().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
    else:
        lat = prod.to(torch.bfloat16)
    rope = row_u8.contiguous()[..., rope_at: rope_at + 2 * f8.ROPE].contiguous().view(torch.bfloat16)
    return torch.cat([lat.view(*codes.shape[:-1], f8.LAT), rope], -1)


def gather_statement(cache, block_ids, cu_seqlens, seq_starts=None, *, out_bits, guard_unwritten=False, scale_shift=0,
                     truncate=False, rope_at=f8.ROPE_AT, **addressing):
    """The op on CPU tensors.  cache: bf16 [num_blocks, P, 576] or uint8 [num_blocks, P, 656] (any strides); out_bits: int16
    [T, 576], the output as it is before the call.  Returns the int16 [T, 576] it is afterwards.  Mutations: those of sources()
    and dequantise_mutant(), and guard_unwritten, which leaves a ZERO row as it was."""
    fp8 = cache.dtype == torch.uint8
    num_blocks, P = cache.shape[0], cache.shape[1]
    out = out_bits.clone()
    src = sources(block_ids, cu_seqlens, seq_starts, out.shape[0], P, num_blocks, **addressing)
    rows = [r for r, s in enumerate(src) if s not in (ZERO, UNWRITTEN)]
    if rows:
        cells = cache[torch.tensor([src[r][0] for r in rows]), torch.tensor([src[r][1] for r in rows])]
        if fp8:
            plain = scale_shift == 0 and not truncate and rope_at == f8.ROPE_AT
            cells = f8.dequantise(cells) if plain else dequantise_mutant(cells, scale_shift=scale_shift, truncate=truncate,
                                                                         rope_at=rope_at)
        out[torch.tensor(rows)] = cells.contiguous().view(torch.int16)
    if not guard_unwritten:
        zeros = [r for r, s in enumerate(src) if s == ZERO]
        if zeros:
            out[torch.tensor(zeros)] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
LAYOUTS = ("plain", "padded", "pool")  # contiguous / padded token stride / a view into a larger pool
FILL = 0x5A
LEAD, TRAIL = 2, 2  # output rows of no request in front of cu_seqlens[0] and behind cu_seqlens[B]


def requests_for(P):
    """(start, count) of the GPU cases: an empty request, one row, pieces that start inside a page and cross page edges, and
    one of exactly 2 P rows"""
    return [(0, 0), (0, 1), (5, 27), (16, 17), (130, 300), (3, 2 * P)]


def alloc_shape(nblocks, P, layout, fp8):
    row, wide = (f8.ROW, 704) if fp8 else (WIDTH, 640)
    return {"plain": (nblocks, P, row), "padded": (nblocks, P, wide), "pool": (nblocks + 2, P + 3, wide)}[layout]


def cache_view(alloc, P, layout, fp8):
    """the op's cache argument as a view of the allocation"""
    row = f8.ROW if fp8 else WIDTH
    return {"plain": alloc, "padded": alloc[:, :, :row], "pool": alloc[1:-1, 2: 2 + P, :row]}[layout]


def build_case(P, layout, fp8, requests=None, seed=0, max_blocks=None):
    """One case on the CPU: .alloc (the cache allocation: int16 bit patterns for the bf16 cache, uint8 for FP8), .cache (the
    op's view of it, bf16 / uint8), .block_ids (padded with -1), .cu_seqlens (cu[0] = LEAD), .seq_starts, .T (output rows,
    TRAIL of them behind the last request), .requests, .P, .num_blocks."""
    requests = requests_for(P) if requests is None else requests
    g = torch.Generator().manual_seed(1000 * P + 10 * LAYOUTS.index(layout) + int(fp8) + 7919 * seed)
    pages = [-(-(max(s, 0) + n) // P) if n > 0 else 0 for s, n in requests]
    nblocks = sum(pages) + 3  # three pages no table lists
    width = max_blocks if max_blocks is not None else max(pages) + 2
    perm = torch.randperm(nblocks, generator=g).tolist()
    block_ids = torch.full((len(requests), width), -1, dtype=torch.int32)
    listed, o = [], 0
    for b, n in enumerate(pages):
        n = min(n, width)
        block_ids[b, :n] = torch.tensor(perm[o: o + n], dtype=torch.int32)
        listed += perm[o: o + n]
        o += pages[b]
    shape = alloc_shape(nblocks, P, layout, fp8)
    if not fp8:
        # every 16-bit pattern may occur, NaN and Inf encodings among them: the bf16 path must do no arithmetic
        alloc = torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int32).to(torch.int16)
        cache = cache_view(alloc, P, layout, False)
        special = torch.tensor([0x7FC0, 0x7F80, 0xFF80, 0x7FFF, 0xFFC1, 0x0001, 0x8000], dtype=torch.int32).to(torch.int16)
        cache[:, :, : len(special)] = special  # in every row, whatever the draw
        cache = cache.view(torch.bfloat16)
    else:
        alloc = torch.full(shape, FILL, dtype=torch.uint8)
        cache = cache_view(alloc, P, layout, True)
        rows = torch.randn(nblocks, P, WIDTH, generator=g).to(torch.bfloat16)
        q = f8.quantise(rows, vary_seed=seed + 11)
        zero_scale = torch.rand(nblocks, P, f8.GROUPS, generator=g) < 0.03  # a few groups with scale 0
        sc = q[..., f8.SCALES_AT: f8.ROPE_AT].contiguous().view(torch.float32)
        sc[zero_scale] = 0.0
        q[..., f8.SCALES_AT: f8.ROPE_AT] = sc.view(torch.uint8)
        cache.copy_(q)
        # page tails and pages no table lists: FILL
        for p in set(range(nblocks)) - set(listed):
            cache[p] = FILL
        for b, (s, n) in enumerate(requests):
            if n > 0 and (max(s, 0) + n) % P and pages[b] <= width:
                cache[int(block_ids[b, pages[b] - 1]), (max(s, 0) + n) % P:] = FILL
    cu = [LEAD]
    for _, n in requests:
        cu.append(cu[-1] + n)
    return SimpleNamespace(alloc=alloc, cache=cache, block_ids=block_ids, cu_seqlens=torch.tensor(cu, dtype=torch.int32),
                           seq_starts=torch.tensor([s for s, _ in requests], dtype=torch.int32), T=cu[-1] + TRAIL,
                           requests=requests, P=P, num_blocks=nblocks, layout=layout, fp8=fp8)


def build_guard_case(P, fp8, bad):
    """Rows that cannot be fetched, among rows that can: request 0 has the page id `bad` in its second table slot; request 1
    starts 3 tokens before the end of the table, so that pos // P >= max_blocks from its fourth row on; request 2 starts at -5.
    Returns (case, zero_rows): the output rows that must come back as zeros."""
    width = 4
    reqs = [(0, 2 * P + 8), (width * P - 3, 8), (-5, 12)]
    c = build_case(P, "plain", fp8, requests=reqs, seed=3, max_blocks=width)
    # request 1's context fills the whole table; request 2's positions 0 .. 6 lie in its first page
    c.block_ids[0, 1] = bad
    cu = c.cu_seqlens.tolist()
    zero_rows = list(range(cu[0] + P, cu[0] + 2 * P)) + list(range(cu[1] + 3, cu[2])) + list(range(cu[2], cu[2] + 5))
    return c, zero_rows
