"""The DSA lightning indexer of a DeepSeek-V3.2 decode step: the paged FP8 index-key cache, its writer, the FP8 MQA logits over it
and the top-k that yields the `indices` of hpc.attention_decode_mla_sparse_bf16 / _fp8 (csrc/mla_indexer.hip), and the front end
in front of them (csrc/mla_indexer_prep.hip).

No reference counterpart: the ops are registered under torch.ops.hpc_mla.* and pinned to the float64 PyTorch statements
tests/mla_indexer_ref.py and tests/mla_indexer_prep_ref.py.  The index key's LayerNorm, RoPE and rotation in front of the store,
the queries' RoPE, rotation and quantisation and the fold of the head weights are mla_indexer_prep_fp8; mla_indexer_store_k_fp8
remains for a caller that runs them itself.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the libraries that register torch.ops.hpc_mla.*)


def mla_indexer_store_k_fp8(k_cache: Tensor, k: Tensor, num_seqlen_per_req: Tensor, q_index: Tensor, block_ids: Tensor) -> None:
    """Quantise the index keys of the new tokens and store them in the paged index-key cache.  Returns None.

    The index-key cache: every token of every request has ONE index key of 128 columns, shared by all index heads, stored
    as 128 float8_e4m3fn codes and one float32 scale; a column is fp32(code[d]) * scale.  k_cache is a torch.uint8 tensor,
    logically [num_blocks, P * 132], addressed through the same block_ids page table as the latent cache.  Within a page
    the codes of its P tokens come first ([P, 128] at byte 0), the P float32 scales follow at byte P * 128, so every
    16-byte access is aligned without padding a row to 144 bytes.  P in {16, 32, 64, 128}; the block stride
    (k_cache.stride(0)) is at least P * 132 and a multiple of 16 bytes; the base is 16-byte aligned.  The readers take any
    finite non-negative scale, so a cache written by another producer of this layout works.

    k                 bf16 [T, 128]: the index key after the caller's own norm, RoPE and rotation.  The last dim is
                      contiguous, the row stride a multiple of 8 elements, the base 16-byte aligned.
    quantisation      the convention of hpc.blockwise_fp8_quant, a row being exactly one 128-block, every step in fp32:
                      scale = amax / 448, code = e4m3fn(x * (1 / (scale + 1e-8))) - bit-identical to
                      tests/blockwise_quant_ref.py::quant(k).
    destination       as hpc.mla_rope_norm_store_kv: row r belongs to the last request b with q_index[b] <= r, at position
                      num_seqlen_per_req[b] - (q_index[b + 1] - r).  num_seqlen_per_req int32 [num_req] (total lengths
                      including the new tokens), q_index int32 [num_req + 1], block_ids int32 [num_req, max_blocks].  Rows
                      of no request store nothing, a page id outside [0, num_blocks) stores nothing, a position beyond the
                      table stores nothing; only the 128 + 4 bytes of a new token are written, page tails are not cleared.

    Everything is read on the device: the call allocates nothing and captures into a hipGraph.  T == 0 or num_req == 0
    returns without a launch."""
    torch.ops.hpc_mla.mla_indexer_store_k_fp8(k_cache, k, num_seqlen_per_req, q_index, block_ids)


@torch.library.register_fake("hpc_mla::mla_indexer_store_k_fp8")
def _mla_indexer_store_k_fp8_fake(k_cache, k, num_seqlen_per_req, q_index, block_ids):
    return None


def mla_indexer_logits_fp8(q: Tensor, weights: Tensor, k_cache: Tensor, block_ids: Tensor, num_seq_kvcache: Tensor, mtp: int = 0,
                           new_kv_included: bool = False, *, output: Tensor = None) -> Tensor:
    """The indexer's FP8 MQA logits over the paged index-key cache.  Returns float32 [B * Sq, max_blocks * P].

    Semantics = the PyTorch statement tests/mla_indexer_ref.py, in float64.  With Sq = mtp + 1, L_b the tokens of request b
    including the Sq new ones (the new_kv_included convention of attention_decode_mla_sparse_bf16) and
    vis(b, s) = L_b - Sq + s + 1, for 0 <= j < min(vis(b, s), max_blocks * P):

        logit[b*Sq+s, j] = kscale_b[j] * sum_h weights[b*Sq+s, h] * relu( sum_{d<128} q[b*Sq+s, h, d] * kcode_b[j, d] )

    q                float8_e4m3fn [B * Sq, Hi, 128], contiguous, Hi in {16, 32, 64}.
    weights          float32 [B * Sq, Hi].  The caller folds the q scales, the softmax scale and Hi ** -0.5 into it, as
                     DeepSeek's reference does; weights may be negative (in the model they are):
                         q8, q_scale = hpc.blockwise_fp8_quant(q_idx.view(T * Hi, 128))      # codes, per-(token, head) scales
                         weights = head_weights * q_scale.view(T, Hi) * softmax_scale * Hi ** -0.5
                         logits = hpc.mla_indexer_logits_fp8(q8.view(T, Hi, 128), weights, k_cache, block_ids, lens)
    k_cache          the cache of mla_indexer_store_k_fp8: torch.uint8 [num_blocks, P * 132], P in {16, 32, 64, 128}.
    poisoned pages   a position whose page id lies outside [0, num_blocks) gets -inf, and its page is never loaded.
    unwritten        columns at or past min(vis, max_blocks * P) are NOT written (mla_indexer_topk never reads them): a
                     fresh output holds whatever the allocator left there.
    limits           mtp 0..3; max_blocks * P <= 2^30; B == 0 returns an empty tensor without a launch.

    Nothing on the host reads lengths or pages and every address is checked against a host value: with output given
    nothing is allocated and the call captures into a hipGraph.  No float atomics, and the head sum has a fixed order:
    the result is bit-identical from call to call."""
    return torch.ops.hpc_mla.mla_indexer_logits_fp8(q, weights, k_cache, block_ids, num_seq_kvcache, int(mtp), bool(new_kv_included),
                                                    output)


@torch.library.register_fake("hpc_mla::mla_indexer_logits_fp8")
def _mla_indexer_logits_fp8_fake(q, weights, k_cache, block_ids, num_seq_kvcache, mtp, new_kv_included, output=None):
    if output is not None:
        return output
    return q.new_empty((q.shape[0], block_ids.shape[1] * (k_cache.shape[1] // 132)), dtype=torch.float32)


def mla_indexer_topk(logits: Tensor, num_seq_kvcache: Tensor, topk: int, mtp: int = 0, new_kv_included: bool = False, *,
                     output: Tensor = None) -> Tensor:
    """The indexer's top-k: the positions of the topk best logits per q row.  Returns int32 [B * Sq, topk] - the `indices`
    of attention_decode_mla_sparse_bf16 / _fp8.

    Semantics = tests/mla_indexer_ref.py::topk_statement.  A pure selection over row r's columns [0, n_r), with
    n_r = clamp(vis(b, s), 0, logits.shape[1]) and vis(b, s) = L_b - Sq + s + 1 as in mla_indexer_logits_fp8.

    selection        the min(topk, n_r) best positions under (logit descending, position ascending): ties go to the
                     smaller position.  Values are ordered as torch.topk orders them: -0.0 == +0.0, NaN ranks above +inf;
                     -inf is an ordinary lowest value (the attention drops unreadable positions itself).
    output           the positions in ASCENDING position order, then -1 to the end of the row: the list is deterministic
                     (the sparse attention sums in list order) and page-local.  When n_r <= topk the list is exactly
                     0 .. n_r - 1 then -1 - the identity list on which the sparse op is bit-equal to the dense op - and
                     the logits are not read at all.  Columns at or past n_r are never read.
    logits           float32 [B * Sq, columns], last dim contiguous, row stride >= columns <= 2^30.
    limits           topk 1..65536, any value; mtp 0..3; B == 0 returns an empty tensor without a launch.

    Nothing on the host reads lengths or logits: with output given nothing is allocated and the call captures into a
    hipGraph.  Integer arithmetic only: the result is bit-identical from call to call."""
    return torch.ops.hpc_mla.mla_indexer_topk(logits, num_seq_kvcache, int(topk), int(mtp), bool(new_kv_included), output)


@torch.library.register_fake("hpc_mla::mla_indexer_topk")
def _mla_indexer_topk_fake(logits, num_seq_kvcache, topk, mtp, new_kv_included, output=None):
    return output if output is not None else logits.new_empty((logits.shape[0], topk), dtype=torch.int32)


def mla_indexer_topk_fp8(q: Tensor, weights: Tensor, k_cache: Tensor, block_ids: Tensor, num_seq_kvcache: Tensor, topk: int,
                         mtp: int = 0, new_kv_included: bool = False, *, output: Tensor = None) -> Tensor:
    """mla_indexer_logits_fp8 then mla_indexer_topk in one call.  Returns int32 [B * Sq, topk]: what goes into
    attention_decode_mla_sparse_bf16 / _fp8 as `indices`.

    The logits go through a cached scratch buffer of float32 [B * Sq, max_blocks * P] per (device, stream, hipGraph
    capture) that hpc.release_decode_workspaces() drops; it is never zeroed, the top-k reads only the columns the logits
    wrote.  Arguments, limits and rules are those of the two ops; the result is bit-identical to calling them one after
    the other, and from call to call.  With output given nothing is allocated beyond the scratch and the call captures
    into a hipGraph, which replayed after lengths, page table, cache contents and q changed in place gives the new result.
    Two launches: nothing is fused between them."""
    return torch.ops.hpc_mla.mla_indexer_topk_fp8(q, weights, k_cache, block_ids, num_seq_kvcache, int(topk), int(mtp),
                                                  bool(new_kv_included), output)


@torch.library.register_fake("hpc_mla::mla_indexer_topk_fp8")
def _mla_indexer_topk_fp8_fake(q, weights, k_cache, block_ids, num_seq_kvcache, topk, mtp, new_kv_included, output=None):
    return output if output is not None else q.new_empty((q.shape[0], topk), dtype=torch.int32)


def mla_indexer_logits_prefill_fp8(q: Tensor, weights: Tensor, k_cache: Tensor, block_ids: Tensor, num_seqlen_per_req: Tensor,
                                   q_index: Tensor, *, row_begin: int = 0, output: Tensor = None) -> Tensor:
    """The indexer's FP8 MQA logits of a ragged PREFILL chunk over the paged index-key cache.  Returns float32
    [R, max_blocks * P].

    mla_indexer_logits_fp8 with the writers' row rule in the place of mtp; semantics = tests/mla_indexer_ref.py applied to
    the expanded form of tests/mla_indexer_prefill_ref.py (every row its own one-row request of length pos + 1).

    row rule         that of mla_indexer_prep_fp8 / mla_indexer_store_k_fp8: row r of the chunk belongs to the last request b
                     with q_index[b] <= r, at pos = num_seqlen_per_req[b] - (q_index[b + 1] - r).  num_seqlen_per_req int32
                     [num_req] (total lengths INCLUDING the chunk's tokens), q_index int32 [num_req + 1], block_ids int32
                     [num_req, max_blocks]: on the device, never read on the host.  A row at or past q_index[-1] or with
                     pos < 0 is a row of no request.  A live row sees vis(r) = min(pos + 1, max_blocks * P) tokens: causal
                     inside the chunk, all of the cached context before it (chunked prefill, prefix caching).
    q, weights       float8_e4m3fn [R, Hi, 128] and float32 [R, Hi], Hi in {16, 32, 64}, exactly what mla_indexer_prep_fp8
                     returns: the chunk's rows row_begin .. row_begin + R - 1, so a caller can bound the logits' memory by
                     row slabs (mla_indexer_topk_prefill_fp8 does).
    result           for j < vis(r): logit[r - row_begin, j] by the formula of mla_indexer_logits_fp8, with the same bits as
                     that op gives on the expanded form (one head sum, csrc/mla_indexer_dev.h).  Columns at or past vis(r)
                     and rows of no request are NOT written.  A position whose page id lies outside [0, num_blocks) gets
                     -inf, and its page is never loaded.
    k_cache          the cache of mla_indexer_store_k_fp8: torch.uint8 [num_blocks, P * 132], P in {16, 32, 64, 128}.

    Key-stationary: a workgroup stages 16 rows of q in LDS and runs them against each 64-key step of its chunk of columns,
    so a key is loaded once per 16 rows, not once per mtp + 1 <= 4 rows as through the decode op.  R == 0 or num_req == 0
    returns without a launch.  With output given nothing is allocated and the call captures into a hipGraph.  No float
    atomics: the result is bit-identical from call to call."""
    return torch.ops.hpc_mla.mla_indexer_logits_prefill_fp8(q, weights, k_cache, block_ids, num_seqlen_per_req, q_index,
                                                            int(row_begin), output)


@torch.library.register_fake("hpc_mla::mla_indexer_logits_prefill_fp8")
def _mla_indexer_logits_prefill_fp8_fake(q, weights, k_cache, block_ids, num_seqlen_per_req, q_index, row_begin, output=None):
    if output is not None:
        return output
    return q.new_empty((q.shape[0], block_ids.shape[1] * (k_cache.shape[1] // 132)), dtype=torch.float32)


def mla_indexer_topk_prefill(logits: Tensor, num_seqlen_per_req: Tensor, q_index: Tensor, topk: int, *, row_begin: int = 0,
                             output: Tensor = None) -> Tensor:
    """The indexer's top-k of a ragged PREFILL chunk.  Returns int32 [R, topk] - the `indices` of
    attention_prefill_mla_sparse_bf16 / _fp8.

    mla_indexer_topk (the same kernel): its selection, its tie rule (ties go to the smaller position), its ASCENDING
    position output with -1 padding and the identity list 0 .. n_r - 1 without reading a logit when n_r <= topk.  Only
    n_r differs: n_r = min(vis(row_begin + r), logits.shape[1]) from the row rule of mla_indexer_logits_prefill_fp8
    (num_seqlen_per_req, q_index on the device).  A row of no request gets all -1.  logits float32 [R, columns] holds the
    chunk's rows row_begin ..; columns at or past n_r are never read.  topk 1..65536.  With output given nothing is
    allocated and the call captures into a hipGraph."""
    return torch.ops.hpc_mla.mla_indexer_topk_prefill(logits, num_seqlen_per_req, q_index, int(topk), int(row_begin), output)


@torch.library.register_fake("hpc_mla::mla_indexer_topk_prefill")
def _mla_indexer_topk_prefill_fake(logits, num_seqlen_per_req, q_index, topk, row_begin, output=None):
    return output if output is not None else logits.new_empty((logits.shape[0], topk), dtype=torch.int32)


def mla_indexer_topk_prefill_fp8(q: Tensor, weights: Tensor, k_cache: Tensor, block_ids: Tensor, num_seqlen_per_req: Tensor,
                                 q_index: Tensor, topk: int, *, scratch_rows: int = 0, output: Tensor = None) -> Tensor:
    """mla_indexer_logits_prefill_fp8 then mla_indexer_topk_prefill over the whole chunk, in slabs of rows.  Returns int32
    [T, topk]: what goes into attention_prefill_mla_sparse_bf16 / _fp8 as `indices`.

    The logits of a slab go through a cached scratch buffer of float32 [slab_rows, max_blocks * P] per (device, stream,
    hipGraph capture) that hpc.release_decode_workspaces() drops; it is never zeroed, the top-k reads only the columns the
    logits wrote, and it does not grow with T.  scratch_rows > 0 fixes the slab; 0 lets the library take what fits a
    256 MiB budget (a resource cap, csrc/mla_indexer_route.h).  The number of slabs is a host value: with output given
    nothing is allocated beyond the scratch and the call captures into a hipGraph.  The result is bit-identical to the two
    ops run over the whole chunk, whatever the slab, and from call to call.  Two launches per slab."""
    return torch.ops.hpc_mla.mla_indexer_topk_prefill_fp8(q, weights, k_cache, block_ids, num_seqlen_per_req, q_index, int(topk),
                                                          int(scratch_rows), output)


@torch.library.register_fake("hpc_mla::mla_indexer_topk_prefill_fp8")
def _mla_indexer_topk_prefill_fp8_fake(q, weights, k_cache, block_ids, num_seqlen_per_req, q_index, topk, scratch_rows, output=None):
    return output if output is not None else q.new_empty((q.shape[0], topk), dtype=torch.int32)


def mla_indexer_prep_fp8(k_cache: Optional[Tensor], k: Tensor, k_norm_weight: Tensor, k_norm_bias: Tensor, cos_sin: Tensor,
                         num_seqlen_per_req: Tensor, q_index: Tensor, block_ids: Tensor, *, q: Optional[Tensor] = None,
                         head_weights: Optional[Tensor] = None, softmax_scale: Optional[float] = None, eps: float = 1e-6,
                         interleaved: bool = False, rotate_scale: float = 128 ** -0.5, pow2_scale: bool = False,
                         out_k: Optional[Tensor] = None, out_q: Optional[Tensor] = None, out_weights: Optional[Tensor] = None,
                         out_q_rot: Optional[Tensor] = None) -> Optional[Tuple[Tensor, Tensor]]:
    """The indexer's front end in one launch: everything between a layer's wq_b / wk / weights_proj GEMMs and
    mla_indexer_topk_fp8.  Returns (q8, weights) when q is given, else None.

    Semantics = the PyTorch statement tests/mla_indexer_prep_ref.py, in float64.  Row r is one new token.  Its request b is
    the last one with q_index[b] <= r and its position pos = num_seqlen_per_req[b] - (q_index[b + 1] - r), the rule of
    mla_rope_norm_store_kv / mla_indexer_store_k_fp8; rows past q_index[-1] or with pos < 0 belong to no request.
    Everything is computed in fp32 with ONE rounding to bfloat16 per path, after the rotation.

    key, x = k[r] (bfloat16 [T, 128], the wk output):
        n      = (x - mean(x)) / sqrt(var(x) + eps) * k_norm_weight + k_norm_bias      (biased variance over the 128 columns)
        n[:64] = rot(n[:64], cos_sin[pos])                                             (RoPE on the FIRST 64 columns)
        kr     = bf16( H128(n) * rotate_scale )
      kr goes into k_cache exactly as mla_indexer_store_k_fp8(kr) would write it (bit for bit), and into out_k (bfloat16
      [T, 128], contiguous) when given.  k_cache may be None when out_k is given; at least one of the two is required.
    queries, x = q[r, h] (bfloat16 [T, Hi, 128], Hi in {16, 32, 64}), when q is given:
        x[:64]        = rot(x[:64], cos_sin[pos])
        qr            = bf16( H128(x) * rotate_scale )                    -> out_q_rot (bfloat16 [T, Hi, 128]) when given
        (code, scale) = the 128-block quantiser on qr                     -> q8 float8_e4m3fn [T, Hi, 128]
        weights[r, h] = fp32( fp32( head_weights[r, h] * scale ) * c ),   c = float32(softmax_scale * Hi ** -0.5)
      (q8, weights) are exactly the q / weights arguments of mla_indexer_logits_fp8 / mla_indexer_topk_fp8.  q needs
      head_weights (float32 or bfloat16 [T, Hi], contiguous: the weights_proj output) and softmax_scale.

    rot, cos_sin     those of mla_rope_norm_store_kv: cos_sin float32 [max_pos, 64] contiguous, cos[0..31] then sin[0..31];
                     rot turns each pair (a, b) into (a cos_i - b sin_i, b cos_i + a sin_i).  interleaved=False pairs column
                     i with i + 32 (neox: what the V3.2 indexer uses), True pairs (2i, 2i + 1).
    H128             the Walsh-Hadamard transform in Sylvester order, y[i] = sum_j (-1)^popcount(i & j) x[j]; H128 . H128 =
                     128 I, so with the default rotate_scale = 128 ** -0.5 the rotation is orthonormal and q . k is kept.
    quantiser        the project's (hpc.blockwise_fp8_quant, tests/blockwise_quant_ref.py::quant): scale = amax / 448,
                     code = e4m3fn(x * (1 / (scale + 1e-8))).  pow2_scale=True (DeepSeek's ue8m0 format), for key and
                     queries alike: the scale is the smallest power of two at or above amax / 448 - of its float32 bits
                     the exponent field goes up by one when the mantissa is non-zero and is clamped to [1, 254] - and
                     code = e4m3fn(x / scale), which is exact and cannot saturate.  The readers take any finite
                     non-negative scale.
    k_norm_weight,   float32 [128] each.
    k_norm_bias
    layouts          k and q may be views with padded strides: last dim contiguous, row (and head) strides multiples of 8
                     elements, base 16-byte aligned.  q8, weights (float32), out_k and out_q_rot are contiguous.
    rows of no       store nothing in the cache and are written as zeros in out_k, out_q, out_weights and out_q_rot.
    request
    cache guards     as mla_indexer_store_k_fp8: a page id outside [0, num_blocks) stores nothing, a position beyond the table
                     stores nothing, the cos_sin index is clamped to max_pos - 1 (the result of such a row is unspecified);
                     only the 128 + 4 bytes of a new token are written, page tails are not cleared.
    limits           T * (1 + Hi) vectors must fit int32.

    Nothing on the host reads device values.  With out_q and out_weights given (or without q) nothing is allocated and the
    call captures into a hipGraph.  T == 0 or num_req == 0 returns without a launch.  A fixed butterfly order and no
    atomics: the result is bit-identical from call to call."""
    q8, weights = torch.ops.hpc_mla.mla_indexer_prep_fp8(
        k_cache, k, k_norm_weight, k_norm_bias, cos_sin, num_seqlen_per_req, q_index, block_ids, q, head_weights,
        None if softmax_scale is None else float(softmax_scale), float(eps), bool(interleaved), float(rotate_scale), bool(pow2_scale),
        out_k, out_q, out_weights, out_q_rot)
    if q is None:
        return None
    return (q8 if out_q is None else out_q), (weights if out_weights is None else out_weights)


@torch.library.register_fake("hpc_mla::mla_indexer_prep_fp8")
def _mla_indexer_prep_fp8_fake(k_cache, k, k_norm_weight, k_norm_bias, cos_sin, num_seqlen_per_req, q_index, block_ids, q,
                               head_weights, softmax_scale, eps, interleaved, rotate_scale, pow2_scale, out_k, out_q, out_weights,
                               out_q_rot):
    """the entry's return (csrc/torch_mla_indexer.cpp::prep_fp8): out_q / out_weights, fresh ones, or two empty tensors"""
    if q is None:
        return (torch.empty((0,), dtype=torch.float8_e4m3fn, device=k.device), torch.empty((0,), dtype=torch.float32, device=k.device))
    q8 = out_q if out_q is not None else torch.empty(q.shape, dtype=torch.float8_e4m3fn, device=k.device)
    w = out_weights if out_weights is not None else torch.empty(q.shape[:2], dtype=torch.float32, device=k.device)
    return q8, w
