"""hpc.rope — RoPE + QK-norm + paged KV store (reference hpc/rope.py:7-234), and the MLA latent-cache writer (ours)."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the libraries that register torch.ops.hpc.*)


def rope_norm_store_kv(
    key_cache: Tensor,
    value_cache: Tensor,
    qkv: Tensor,
    cos_sin: Tensor,
    num_seqlen_per_req: Tensor,
    q_index: Tensor,
    kvcache_indices: Tensor,
    is_prefill: bool,
    q_norm_weight: Optional[Tensor] = None,
    k_norm_weight: Optional[Tensor] = None,
    out_q: Optional[Tensor] = None,
    out_k: Optional[Tensor] = None,
    out_v: Optional[Tensor] = None,
    qk_norm_policy: int = 0,
) -> Tensor:
    """RoPE on Q/K (neox pairing), optional QK RMSNorm (policy 1: after RoPE, 2: before), K/V written
    into the paged bf16 KV cache (or out_k / out_v), tail of each request's last page zeroed.
    Shapes as in the reference (hpc/rope.py:7-104); head dims 128.  Returns Q [rows, Hq, 128] bf16."""
    return torch.ops.hpc.rope_norm_store_kv(
        key_cache, value_cache, qkv, cos_sin, num_seqlen_per_req, q_index, kvcache_indices, is_prefill,
        q_norm_weight, k_norm_weight, out_q, out_k, out_v, qk_norm_policy,
    )


def rope_norm_store_kv_fp8(
    key_cache: Tensor,
    value_cache: Tensor,
    qkv: Tensor,
    cos_sin: Tensor,
    num_seqlen_per_req: Tensor,
    q_index: Tensor,
    kvcache_indices: Tensor,
    is_prefill: bool,
    k_scale: Tensor,
    v_scale: Tensor,
    quant_policy: int,
    max_seqlens: int = 0,
    upper_max: Optional[float] = None,
    q_scale_inv: Optional[Tensor] = None,
    q_norm_weight: Optional[Tensor] = None,
    k_norm_weight: Optional[Tensor] = None,
    out_q: Optional[Tensor] = None,
    out_k: Optional[Tensor] = None,
    out_v: Optional[Tensor] = None,
    qk_norm_policy: int = 0,
) -> Tuple[Tensor, Tensor, Tensor]:
    """FP8 variant (reference hpc/rope.py:107-234): Q quantised per token per head (quant_policy 1,
    scale = amax/upper_max returned in q_scale: decode [rows, Hq], prefill [num_req, Hq, pad128]) or
    statically (quant_policy 2, q_scale_inv); K/V divided by the static k_scale / v_scale into the
    e4m3 paged cache.  Returns (q e4m3, q_scale or None, split_k_flag int32 [num_req, Hkv] zeroed)."""
    return torch.ops.hpc.rope_norm_store_kv_fp8(
        key_cache, value_cache, qkv, cos_sin, num_seqlen_per_req, q_index, kvcache_indices, is_prefill,
        k_scale, v_scale, quant_policy, max_seqlens, upper_max, q_scale_inv, q_norm_weight, k_norm_weight,
        out_q, out_k, out_v, qk_norm_policy,
    )


def _rope_q_heads(key_cache, value_cache, qkv):
    kv_heads, qk_dim, v_dim = key_cache.size(-2), key_cache.size(-1), value_cache.size(-1)
    return (qkv.size(-1) - kv_heads * qk_dim - kv_heads * v_dim) // qk_dim, kv_heads, qk_dim


@torch.library.register_fake("hpc::rope_norm_store_kv")
def _rope_norm_store_kv_fake(key_cache, value_cache, qkv, cos_sin, num_seqlen_per_req, q_index, kvcache_indices, is_prefill,
                             q_norm_weight, k_norm_weight, out_q=None, out_k=None, out_v=None, qk_norm_policy=0):
    if out_q is not None:
        return out_q
    q_heads, _, qk_dim = _rope_q_heads(key_cache, value_cache, qkv)
    return torch.empty((qkv.size(0), q_heads, qk_dim), dtype=qkv.dtype, device=qkv.device)


@torch.library.register_fake("hpc::rope_norm_store_kv_fp8")
def _rope_norm_store_kv_fp8_fake(key_cache, value_cache, qkv, cos_sin, num_seqlen_per_req, q_index, kvcache_indices, is_prefill,
                                 k_scale, v_scale, quant_policy, max_seqlens, upper_max, q_scale_inv, q_norm_weight,
                                 k_norm_weight, out_q=None, out_k=None, out_v=None, qk_norm_policy=0):
    """(q e4m3, q_scale, split_k_flag) with the entry's shapes (csrc/torch_misc.cpp::rope_norm_store_kv_fp8): dynamic q
    scales are [rows, Hq] in decode and [num_req, Hq, pad128(max_seqlens)] in prefill; with static q scales
    (quant_policy 2) the real op returns an undefined tensor there - a fake must return a tensor: an empty one"""
    q_heads, kv_heads, qk_dim = _rope_q_heads(key_cache, value_cache, qkv)
    rows, num_req, dev = qkv.size(0), num_seqlen_per_req.size(0), qkv.device
    q = out_q if out_q is not None else torch.empty((rows, q_heads, qk_dim), dtype=torch.float8_e4m3fn, device=dev)
    if quant_policy == 1:
        shape = (num_req, q_heads, (max_seqlens + 127) // 128 * 128) if is_prefill else (rows, q_heads)
    else:
        shape = (0,)
    return q, torch.empty(shape, dtype=torch.float32, device=dev), torch.empty((num_req, kv_heads), dtype=torch.int32, device=dev)


def mla_rope_norm_store_kv(ckv_cache: Optional[Tensor], kv_a: Tensor, cos_sin: Tensor, kv_norm_weight: Tensor,
                           num_seqlen_per_req: Tensor, q_index: Tensor, block_ids: Tensor, *, q_pe: Optional[Tensor] = None,
                           out_q_pe: Optional[Tensor] = None, out_ckv: Optional[Tensor] = None, eps: float = 1e-6,
                           interleaved: bool = True) -> Optional[Tensor]:
    """Writer of the paged MLA latent cache (DeepSeek-V3 / R1, Kimi-K2): kv_a_layernorm over the 512 compressed-KV columns,
    RoPE on the shared k_pe head and on every q head, the 576-column latent row stored into its page.  The step between the
    kv_a / q_b projections and attention_decode_mla_bf16, whose cache and q RoPE columns it produces, in one launch.

    No reference counterpart; semantics = the PyTorch statement tests/mla_store_ref.py, in float64.  Row r of kv_a is one
    new token.  Its request b is the last one with q_index[b] <= r and its position
    pos = num_seqlen_per_req[b] - (q_index[b + 1] - r), the rule of rope_norm_store_kv; rows at or past q_index[-1] and rows
    with pos < 0 belong to no request.  Computed in fp32 with one rounding to bfloat16:

        c         = kv_a[r, :512]
        lat[:512] = bf16( c / sqrt(mean(c^2) + eps) * kv_norm_weight )
        lat[512:] = bf16( rot(kv_a[r, 512:576], cos_sin[pos]) )
        ckv_cache[block_ids[b, pos // P], pos % P, :576] = lat        and / or        out_ckv[r] = lat
        out_q_pe[r, h, :] = bf16( rot(q_pe[r, h, :], cos_sin[pos]) )

    rot turns each pair (a, b) into (a cos_i - b sin_i, b cos_i + a sin_i) with cos_i = cos_sin[pos, i] and
    sin_i = cos_sin[pos, 32 + i], i < 32.  interleaved=True pairs elements (2i, 2i + 1) in place (GPT-J style, how vLLM and
    SGLang run DeepSeek); interleaved=False pairs i with i + 32 (neox, as rope_norm_store_kv does at width 128).  A YaRN
    mscale belongs in the table.

    Layouts (all on one device):
      ckv_cache           bfloat16, logical [num_blocks, P, 576], P in {16, 32, 64, 128}; the stride rules of
                          attention_decode_mla_bf16: block and token strides multiples of 8 elements, token stride >= 576,
                          last dim contiguous, base 16-byte aligned (padded rows, views into a larger pool).  None when
                          out_ckv is given;
      kv_a                bfloat16 [rows, 576], last dim contiguous, row stride a multiple of 8, base 16-byte aligned -
                          typically y[:, 1536:2112] of the fused q_a + kv_a projection;
      cos_sin             float32 [max_pos, 64] contiguous: cos[0..31] then sin[0..31];
      kv_norm_weight      float32 [512];
      num_seqlen_per_req  int32 [num_req], total lengths including the new tokens; q_index int32 [num_req + 1];
                          block_ids int32 [num_req, max_blocks].  Nothing on the host reads their values: a captured
                          hipGraph replayed after the lengths changed follows the new lengths;
      q_pe                optional bfloat16 [rows, H, 64], 1 <= H <= 128, last dim contiguous, row and head strides
                          multiples of 8, base 16-byte aligned - typically q[..., 128:] of the q_b projection;
      out_q_pe            optional, like q_pe - typically q_abs[..., 512:] of the [rows, H, 576] buffer the decode op
                          takes, so no concat runs.  May be q_pe itself (in place);
      out_ckv             optional bfloat16 [rows, 576], row stride a multiple of 8.
    Refused as well, because written rows or heads would overlap: row strides below 576 (kv_a, out_ckv), head / row
    strides below 64 (q_pe, out_q_pe), an out_q_pe row stride below (H - 1) * its head stride + 64, and an out_q_pe
    that shares memory with q_pe without being q_pe itself (same pointer, same strides).

    Each of ckv_cache and out_ckv that is given is written; at least one is required.  Returns out_q_pe (the same object
    when given, else a fresh contiguous tensor), or None without q_pe.  With caller-provided outputs nothing is allocated
    per call.  rows == 0 or num_req == 0 returns without a launch.

    Only the 576 columns of the new tokens' cache cells are written: page tails, padding columns, pages no table lists and
    the columns :512 of a q_abs buffer stay byte-identical (no tail is cleared: the decode op ignores finite values in
    page tails).  Rows of no request store nothing into the cache and are written as zeros in out_q_pe and out_ckv.

    Memory safety does not depend on the device values: the table index is clamped to max_pos - 1 (the result of such a
    row is unspecified), and a token is not stored when pos // P >= max_blocks or when its page id is outside
    [0, num_blocks) - frameworks pad tables with -1."""
    out = torch.ops.hpc_mla.rope_norm_store_kv(ckv_cache, kv_a, cos_sin, kv_norm_weight, num_seqlen_per_req, q_index, block_ids,
                                               q_pe, out_q_pe, out_ckv, float(eps), bool(interleaved))
    if q_pe is None:
        return None
    return out if out_q_pe is None else out_q_pe


@torch.library.register_fake("hpc_mla::rope_norm_store_kv")
def _mla_rope_norm_store_kv_fake(ckv_cache, kv_a, cos_sin, kv_norm_weight, num_seqlen_per_req, q_index, block_ids, q_pe,
                                 out_q_pe, out_ckv, eps, interleaved):
    """the entry's return (csrc/torch_mla.cpp::rope_norm_store_kv): out_q_pe, a fresh [rows, H, 64], or an empty tensor"""
    if q_pe is None:
        return torch.empty((0,), dtype=kv_a.dtype, device=kv_a.device)
    if out_q_pe is not None:
        return out_q_pe
    return torch.empty(q_pe.shape, dtype=kv_a.dtype, device=kv_a.device)


def mla_rope_norm_store_kv_fp8(ckv_cache: Optional[Tensor], kv_a: Tensor, cos_sin: Tensor, kv_norm_weight: Tensor,
                               num_seqlen_per_req: Tensor, q_index: Tensor, block_ids: Tensor, *,
                               q_pe: Optional[Tensor] = None, out_q_pe: Optional[Tensor] = None,
                               out_ckv: Optional[Tensor] = None, eps: float = 1e-6,
                               interleaved: bool = True) -> Optional[Tensor]:
    """mla_rope_norm_store_kv into the FP8 latent KV cache that attention_decode_mla_fp8 reads.  Arguments, the
    row-to-position rule, the guards (a page id outside [0, num_blocks) is not stored, neither is a token with
    pos // P >= max_blocks, the table index is clamped) and the return value are those of mla_rope_norm_store_kv; out_ckv
    and out_q_pe stay bfloat16 and are bit-identical to what mla_rope_norm_store_kv writes.

    ckv_cache is a torch.uint8 tensor, logical [num_blocks, P, 656], P in {16, 32, 64, 128}, or None when out_ckv is
    given: last dim contiguous, token stride >= 656 bytes and a multiple of 16, block stride a multiple of 16, base
    16-byte aligned.  With lat the bfloat16-ROUNDED row mla_rope_norm_store_kv stores, the written row is

        bytes   0 .. 511 (offset 0)    code[d] = e4m3fn_sat( lat[d] * (1 / (scale[d // 128] + 1e-8)) ),  d < 512
        bytes 512 .. 527 (offset 512)  scale[g] = amax / 448 of lat[128 g .. 128 g + 127], float32, g < 4
        bytes 528 .. 655 (offset 528)  lat[512:], the RoPE'd k_pe in bfloat16

    every step in float32 - tests/blockwise_quant_ref.py::quant on the 512 columns, the quantiser of
    fused_rmsnorm_blockwise_quant.  Quantising the rounded row makes the FP8 cache an exact function of the bf16 cache.
    A reader recovers c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] ).  Only those 656 bytes of a new token's cell are
    written: token-stride padding, page tails and unlisted pages stay byte-identical."""
    out = torch.ops.hpc_mla.rope_norm_store_kv_fp8(ckv_cache, kv_a, cos_sin, kv_norm_weight, num_seqlen_per_req, q_index,
                                                   block_ids, q_pe, out_q_pe, out_ckv, float(eps), bool(interleaved))
    if q_pe is None:
        return None
    return out if out_q_pe is None else out_q_pe


torch.library.register_fake("hpc_mla::rope_norm_store_kv_fp8")(_mla_rope_norm_store_kv_fake)
