"""hpc.stem — Stem block-sparse mask generation (reference hpc/stem.py).

The pipeline that feeds `hpc.attention_with_kvcache_blocksparse_prefill_fp8`: score every (q block, kv block) pair of
128-token stem blocks cheaply, then keep a per-row top-k plus fixed patterns.

    stem_oam_prep_paged_kv  paged FP8 K / V  -> kflat bf16 [B, Hkv, max_Kb, 2048], vbias f32 [B, Hkv, max_Kb]
    stem_oam_prep_varlen_q  packed FP8 Q     -> qflat bf16 [B, Hq, max_Qb, 2048]
    stem_oam_gemm           qflat, kflat     -> block_logits bf16 [B, Hq, max_Qb, max_Kb] (-inf where masked)
    stem_tpd                block_logits     -> mask uint8 [B, Hq, max_Qb, max_Kb] (1 = attend)
    stem_paged_kv           the four in sequence

Same function names, argument order and defaults as the reference; the kernels are the gfx950 ones of csrc/stem.hip.
The ops are registered as torch.ops.hpc_stem.* (not torch.ops.hpc.*).  Only stem_block_size 128
with stem_stride 16 and head dim 128 are supported.  The prep ops read kv_seq_lens.max() / q_seq_lens.max() on the
host to size their outputs, as the reference does.
"""
from typing import Tuple

import torch
from torch import Tensor

from . import _C  # noqa: F401  (loads the library that registers torch.ops.hpc_stem.*)
from .attention import QuantType


def stem_oam_prep_paged_kv(
    kcache: Tensor,
    vcache: Tensor,
    kscale: Tensor,
    vscale: Tensor,
    kv_indices: Tensor,
    kv_seq_lens: Tensor,
    lambda_mag: float = 0.3,
    stem_block_size: int = 128,
    stem_stride: int = 16,
    quant_type: QuantType = QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR,
) -> Tuple[Tensor, Tensor]:
    """K group sums and V-norm block bias of a paged FP8 KV cache.

    kcache / vcache: float8_e4m3fn [num_pages, 32 | 64, Hkv, 128]; kv_indices int32 [B, max_pages] (page table);
    kv_seq_lens int32 [B].  quant_type QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR: kscale / vscale float32 [1];
    QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD: kscale per token, [num_pages, page / 32, Hkv, 32] float32 or the fp8
    view of that storage ([num_pages, page / 32, Hkv, 128], the cache's tail rows), vscale float32 [Hkv].

    Returns kflat bf16 [B, Hkv, max_Kb, 16 * 128]: for block b and group g the sum of kscale * K over tokens
    128 b + g + 16 s (s < 8) at columns (15 - g) * 128 (reversed group order); and vbias float32 [B, Hkv, max_Kb]:
    lambda_mag times the mean over the block's eight 16-token windows of relu of the standardised log window norm.
    Blocks past a request's length are zero.
    """
    return torch.ops.hpc_stem.stem_oam_prep_paged_kv(
        kcache, vcache, kscale, vscale, kv_indices, kv_seq_lens, lambda_mag, stem_block_size, stem_stride,
        quant_type.value,
    )


def stem_oam_prep_varlen_q(
    q_fp8: Tensor,
    qscale: Tensor,
    q_seq_lens: Tensor,
    cu_seqlens_q: Tensor,
    stem_block_size: int = 128,
    stem_stride: int = 16,
) -> Tensor:
    """Q group sums of packed FP8 queries.

    q_fp8 float8_e4m3fn [total_tokens, Hq, 128]; qscale float32 [B, Hq, max_seq_q_pad] (per token and head);
    q_seq_lens int32 [B]; cu_seqlens_q int32 [B + 1].  Returns qflat bf16 [B, Hq, max_Qb, 16 * 128] with the sum of
    qscale * Q over tokens 128 b + g + 16 s (s < 8) at columns g * 128 (natural group order); zeros past a request.
    """
    return torch.ops.hpc_stem.stem_oam_prep_varlen_q(q_fp8, qscale, q_seq_lens, cu_seqlens_q, stem_block_size, stem_stride)


def stem_oam_gemm(
    qflat: Tensor,
    kflat: Tensor,
    vbias: Tensor,
    q_seq_lens: Tensor,
    kv_seq_lens: Tensor,
    stem_block_size: int = 128,
    stem_stride: int = 16,
    causal: bool = True,
) -> Tensor:
    """Block logits qflat . kflat^T / 64 + vbias (GQA: q head h reads kv head h / (Hq / Hkv)).

    Returns bf16 [B, Hq, qflat.size(2), kflat.size(2)]; -inf past a request's q or kv blocks and, when causal, where
    qb + (kv_len - q_len + 127) // 128 < kb.
    """
    return torch.ops.hpc_stem.stem_oam_gemm(qflat, kflat, vbias, q_seq_lens, kv_seq_lens, stem_block_size, stem_stride,
                                            causal)


def stem_tpd(
    block_logits: Tensor,
    q_seq_lens: Tensor,
    kv_seq_lens: Tensor,
    num_prompt_tokens: Tensor,
    block_size: int = 128,
    alpha: float = 1.0,
    initial_blocks: int = 4,
    window_size: int = 4,
    k_block_num_rate_medium: float = 0.2,
    k_block_num_bias_medium: int = 30,
    k_block_num_rate_large: float = 0.1,
    k_block_num_bias_large: int = 30,
) -> Tensor:
    """Block mask from block logits: per row the top-`budget` blocks plus fixed patterns.

    block_logits bf16 contiguous [B, H, max_Qb, max_Kb <= 32768]; q_seq_lens / kv_seq_lens / num_prompt_tokens int32
    [B] (num_prompt_tokens: the whole prompt's kv tokens - the same for every chunk of a chunked prefill; kv_seq_lens
    for a plain prefill).  The budget follows from P = ceil(num_prompt_tokens / block_size) (P below 56: P; below 160:
    int(P * rate_medium) + bias_medium; else int(P * rate_large) + bias_large), decaying linearly towards k * alpha
    over the later rows.  Selected besides the top-budget blocks (ties included): the first initial_blocks blocks, the
    window_size blocks ending at the row's diagonal block, and the diagonal block.  Returns uint8 of the logits' shape.
    """
    return torch.ops.hpc_stem.stem_tpd(
        block_logits, q_seq_lens, kv_seq_lens, num_prompt_tokens, block_size, alpha, initial_blocks, window_size,
        k_block_num_rate_medium, k_block_num_bias_medium, k_block_num_rate_large, k_block_num_bias_large,
    )


def stem_paged_kv(
    q_fp8: Tensor,
    kcache: Tensor,
    vcache: Tensor,
    qscale: Tensor,
    kscale: Tensor,
    vscale: Tensor,
    kv_indices: Tensor,
    cu_seqlens_q: Tensor,
    kv_seq_lens: Tensor,
    num_prompt_tokens: Tensor,
    lambda_mag: float = 0.3,
    alpha: float = 1.0,
    stem_block_size: int = 128,
    stem_stride: int = 16,
    causal: bool = True,
    initial_blocks: int = 4,
    window_size: int = 4,
    k_block_num_rate_medium: float = 0.2,
    k_block_num_bias_medium: int = 30,
    k_block_num_rate_large: float = 0.1,
    k_block_num_bias_large: int = 30,
    quant_type: QuantType = QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR,
) -> Tensor:
    """End-to-end Stem mask for a paged FP8 prefill: prep_paged_kv, prep_varlen_q, oam_gemm, tpd.

    Arguments as in the four stages; kv_seq_lens counts the cached tokens including this chunk's q tokens.  The
    returned uint8 [B, Hq, ceil(max q_len / 128), ceil(max kv_len / 128)] is the `block_mask` of
    hpc.attention_with_kvcache_blocksparse_prefill_fp8.
    """
    q_seq_lens = (cu_seqlens_q[1:] - cu_seqlens_q[:-1]).to(torch.int32)
    kflat, vbias = stem_oam_prep_paged_kv(kcache, vcache, kscale, vscale, kv_indices, kv_seq_lens, lambda_mag,
                                          stem_block_size, stem_stride, quant_type)
    qflat = stem_oam_prep_varlen_q(q_fp8, qscale, q_seq_lens, cu_seqlens_q, stem_block_size, stem_stride)
    block_logits = stem_oam_gemm(qflat, kflat, vbias, q_seq_lens, kv_seq_lens, stem_block_size, stem_stride, causal)
    return stem_tpd(block_logits, q_seq_lens, kv_seq_lens, num_prompt_tokens, stem_block_size, alpha, initial_blocks,
                    window_size, k_block_num_rate_medium, k_block_num_bias_medium, k_block_num_rate_large,
                    k_block_num_bias_large)


# Fakes: the output sizes of the prep ops depend on the data (the longest request), so the fakes give the upper bounds
# the reference's fakes give - every page of the page table in use, every token of qscale's padded length.
@torch.library.register_fake("hpc_stem::stem_oam_prep_paged_kv")
def _stem_oam_prep_paged_kv_fake(kcache, vcache, kscale, vscale, kv_indices, kv_seq_lens, lambda_mag, stem_block_size,
                                 stem_stride, quant_type):
    max_kb = (kv_indices.size(1) * kcache.size(1) + stem_block_size - 1) // stem_block_size
    b, hkv = kv_seq_lens.size(0), kcache.size(2)
    return (kcache.new_empty((b, hkv, max_kb, stem_stride * kcache.size(3)), dtype=torch.bfloat16),
            kcache.new_empty((b, hkv, max_kb), dtype=torch.float32))


@torch.library.register_fake("hpc_stem::stem_oam_prep_varlen_q")
def _stem_oam_prep_varlen_q_fake(q_fp8, qscale, q_seq_lens, cu_seqlens_q, stem_block_size, stem_stride):
    max_qb = (qscale.size(2) + stem_block_size - 1) // stem_block_size
    return q_fp8.new_empty((q_seq_lens.size(0), q_fp8.size(1), max_qb, stem_stride * q_fp8.size(2)), dtype=torch.bfloat16)


@torch.library.register_fake("hpc_stem::stem_oam_gemm")
def _stem_oam_gemm_fake(qflat, kflat, vbias, q_seq_lens, kv_seq_lens, stem_block_size, stem_stride, causal):
    return qflat.new_empty((qflat.size(0), qflat.size(1), qflat.size(2), kflat.size(2)), dtype=torch.bfloat16)


@torch.library.register_fake("hpc_stem::stem_tpd")
def _stem_tpd_fake(block_logits, q_seq_lens, kv_seq_lens, num_prompt_tokens, block_size, alpha, initial_blocks,
                   window_size, k_block_num_rate_medium, k_block_num_bias_medium, k_block_num_rate_large,
                   k_block_num_bias_large):
    return torch.empty_like(block_logits, dtype=torch.uint8)
