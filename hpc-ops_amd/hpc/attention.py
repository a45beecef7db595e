"""hpc.attention — decode-attention surface of the reference (hpc/attention.py:8-12, :336-696).

Same function names, argument names/defaults and semantics; the kernels behind torch.ops.hpc.* are
the gfx950 ones of libhpc_amd.so.  Prefill / block-sparse entry points of the reference are out of
scope of this hot path and intentionally absent.
"""
import ctypes
from enum import Enum

import torch
from torch import Tensor

from . import _C


class QuantType(Enum):
    QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD = 0
    QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR = 1
    QPERTENSOR_KPERTENSOR_VPERTENSOR = 2
    QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD_QKHADAMARD = 3


def attention_decode_bf16(
    q: Tensor,
    kcache: Tensor,
    vcache: Tensor,
    block_ids: Tensor,
    num_seq_kvcache: Tensor,
    mtp: int = 0,
    new_kv_included: bool = False,
    splitk: bool = True,
    task_map: Tensor = None,
    split_flag: Tensor = None,
    output: Tensor = None,
) -> Tensor:
    """Paged decode attention in bfloat16 (reference hpc/attention.py:336-417).

    Args:
        q: [num_batch * num_seq_q, num_head_q, 128] bfloat16 (num_seq_q = mtp + 1).  num_head_q / num_head_kv must be
            1, 2, 4, 8 or 16 (the ratios the prefill ops take); every ratio takes mtp 0..4.  Ratio 16 at mtp 3 / 4 (64 / 80 q
            rows per kv head) is served as 2 slices of the kv head's q heads - its K / V are read once per slice: 1.4-1.5 x
            the time of one pass at mtp 3 (2 x with num_seq_kvcache on the host), 2 x at mtp 4.
        kcache / vcache: paged caches, logical [num_blocks, block_size, num_head_kv, 128] bfloat16;
            any block/token/head strides (NHD-contiguous and HND-backed views both work).  Unused
            slots of a request's last block should be zero (they are masked anyway).
        block_ids: [num_batch, max_blocks] int32 page table.
        num_seq_kvcache: [num_batch] int32; tokens in the cache before this step, or including the
            num_seq_q new ones when new_kv_included.
        splitk: accepted for API compatibility; the schedule is always the dynamic tile schedule.
        task_map: workspace from get_attention_decode_task_workspace filled by
            assign_attention_decode_task (scheduled on the fly when None).
        split_flag: unused on MI355X (the reference's static path spins on it).
        output: optional preallocated [num_batch * num_seq_q, num_head_q, 128] bfloat16.
    """
    return torch.ops.hpc.attention_decode_bf16(
        q, kcache, vcache, block_ids, num_seq_kvcache, mtp, new_kv_included, splitk, task_map,
        split_flag, output,
    )


def attention_decode_fp8(
    q: Tensor,
    kcache: Tensor,
    vcache: Tensor,
    block_ids: Tensor,
    num_seq_kvcache: Tensor,
    qscale: Tensor,
    kscale: Tensor,
    vscale: Tensor,
    mtp: int = 0,
    new_kv_included: bool = False,
    quant_type: QuantType = QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR,
    splitk: bool = True,
    task_map: Tensor = None,
    split_flag: Tensor = None,
    output: Tensor = None,
) -> Tensor:
    """Paged decode attention with FP8 (e4m3) Q/K/V (reference hpc/attention.py:420-517):
    softmax(Q K^T * qscale * kscale / sqrt(head_dim)) V * vscale, bfloat16 output.

    Args (beyond attention_decode_bf16):
        q: [num_batch * num_seq_q, num_head_q, 128] float8_e4m3fn.  num_head_q / num_head_kv must be 1, 2, 4, 8 or 16;
            every ratio takes mtp 0..3.  Ratio 16 at mtp 2 / 3 (48 / 64 q rows per kv head) is served as 2 slices of the kv
            head's q heads - its K / V are read twice: 1.4-1.6 x the time of one pass on pages of 32 / 64 tokens, 2 x on
            pages of 16.
        kcache / vcache: paged caches of 1-byte elements (float8_e4m3fn).
        qscale: float32 [num_batch * num_seq_q, num_head_q] per-token per-head Q scale.
        kscale: float32 [1] (QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR) or the view of the K-cache
            tail rows `kcache_full[:, block_size:]` holding per-token per-head fp32 scales
            (QPERTOKEN_PERHEAD_KPERTOKEN_PERHEAD_VPERHEAD).
        vscale: float32 [1] or [num_head_kv].
    """
    return torch.ops.hpc.attention_decode_fp8(
        q, kcache, vcache, block_ids, num_seq_kvcache, qscale, kscale, vscale, mtp,
        new_kv_included, quant_type.value, splitk, task_map, split_flag, output,
    )


def get_attention_decode_task_workspace(
    max_num_batch: int, max_seqlen: int, num_head_kv: int, min_process_len: int = 512
):
    """Allocate the task-map workspace (reference hpc/attention.py:520-582; same byte layout).

    Returns int8 [task_map_byte_size] on the current device with header ints 2..4 pre-filled
    (num_head_kv, max_num_batch, scheduler byte size).
    """
    dev = torch.device("cuda", torch.cuda.current_device())
    num_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    total, sched = task_workspace_bytes(num_cu, max_num_batch, max_seqlen, num_head_kv, min_process_len)
    ws = torch.zeros(total, dtype=torch.int8, device=dev)
    hdr = ws.view(torch.int32)
    hdr[2] = num_head_kv
    hdr[3] = max_num_batch
    hdr[4] = sched
    return ws


def task_workspace_bytes(num_cu, max_num_batch, max_seqlen, num_head_kv, min_process_len):
    """Byte size + scheduler byte size of the task-map workspace (hpc_attention_decode_task_workspace_bytes: the sizes of
    reference hpc/attention.py:540-571, for up to 4 bins per CU, so any gfx950 bin count fits)."""
    sched = ctypes.c_int64(0)
    total = _C.lib.hpc_attention_decode_task_workspace_bytes(num_cu, max_num_batch, max_seqlen, num_head_kv, min_process_len,
                                                             ctypes.byref(sched))
    _C.require(total > 0, "task_workspace_bytes: invalid arguments")
    return total, sched.value


def release_decode_workspaces():
    """Drop EVERY zero-once scratch buffer the host library caches per (purpose, device, stream, hipGraph capture) - the
    decode workspaces, the router GEMM's split-K ticket buffers, the MLA decode's split-KV partials and the MLA indexer's
    logits (a decode step's and a prefill slab's) alike (csrc/torch_common.h::release_cached_scratch) -
    e.g. after the streams / graphs that used them are gone.  Buffers of captures that have ended are dropped on the
    next call on their stream anyway."""
    torch.ops.hpc._release_decode_workspaces()


def assign_attention_decode_task(
    num_seq_kvcache: Tensor,
    task_map: Tensor,
    num_head_kv: int,
    mtp: int,
    new_kv_included: bool,
    min_process_len: int = 512,
) -> Tensor:
    """Fill `task_map` for one decode step (reference hpc/attention.py:585-626).

    NOTE: as in the reference, the 4th argument is passed to the op as num_seq_q (callers pass
    num_seq_q = mtp + 1 here, tests/test_attention_decode_bf16.py:105-121 of the reference).
    `num_seq_kvcache` may live on the GPU (device scheduler) or on the CPU (host scheduler, then
    three byte ranges are copied into the device workspace); both give byte-identical maps.

    `min_process_len` (KV tokens one workgroup processes at least) shapes the map's bins for the kernels that consume
    the map (<= 16 q rows per kv head on HND pages or with an odd kv-head count).  The head-pair kernels (NHD pages, even
    kv-head count; 17-32 q rows per kv head on any layout: csrc/attention_decode_v2.hip) plan their ranges in closed form inside the launch - the map's bins and split
    decisions do not apply there - and honour this lower bound through header int 6 of the map, where the scheduler
    records it (csrc/sched_task_info.h)."""
    if num_seq_kvcache.device.type == "cpu":
        task_map_host = torch.ops.hpc.assign_attention_decode_task(
            num_seq_kvcache, num_head_kv, mtp, new_kv_included, min_process_len, None
        )
        flat = task_map_host.reshape(-1)
        task_map[:8].copy_(flat[:8], non_blocking=True)
        task_map[20:28].copy_(flat[20:28], non_blocking=True)  # max chunks per request, min_process_len (header int 6)
        task_map[48 : flat.numel()].copy_(flat[48:], non_blocking=True)
        return task_map
    return torch.ops.hpc.assign_attention_decode_task(
        num_seq_kvcache, num_head_kv, mtp, new_kv_included, min_process_len, task_map
    )


def print_attention_decode_task(task_map: Tensor) -> None:
    """Pretty-print a task map (reference hpc/attention.py:629-696)."""
    stride = 12
    task = task_map.view(torch.int32).reshape(-1)
    task = task[: task.numel() // stride * stride].reshape(-1, stride).cpu()
    per1, bins = int(task[0][0]), int(task[0][1])
    num_head_kv, max_num_batch = int(task[0][2]), int(task[0][3])
    chunk_row = 1 + bins * per1
    chunks = task[chunk_row:].reshape(-1)[: num_head_kv * max_num_batch]
    print(
        f"\n[Dynamic Decode Attn Task Map] num_tile_per_cta={per1 - 1}, num_head_kv={num_head_kv}, "
        f"max_num_batch={max_num_batch}, num_total_ctas={bins}"
    )
    print(f"num_chunks[ihead_kv, ibatch]:\n{chunks.reshape(num_head_kv, max_num_batch)}\n")
    idx, empty = 0, 0
    for icta in range(bins):
        rows = task[1 + icta * per1 : 1 + (icta + 1) * per1]
        if int(rows[0][0]) < 0 or int(rows[0][1]) < 0:
            empty += 1
            continue
        print(f"#######CTA{icta}########")
        ntask, seqkv = 0, 0
        for row in rows[: per1 - 1]:
            r = [int(v) for v in row]
            if r[0] < 0 or r[1] < 0:
                break
            print(
                f"task:{idx}, ihead_kv:{r[0]}, ibatch:{r[1]}, ichunk:{r[2]}, iseq_start:{r[3]}, "
                f"num_seqkv:{r[4]}, num_seqkvcache:{r[5]}, num_tile_kv:{r[6]}, "
                f"num_tile_full:{r[7]}, is_casual_chunk:{r[8]}"
            )
            idx += 1
            ntask += 1
            seqkv += r[4]
        print(f"CTA:{icta}, num_tasks:{ntask}, total_seqkv:{seqkv}")
    print(f"[idle] {empty}/{bins} bins were empty")


@torch.library.register_fake("hpc::attention_decode_bf16")
def attention_decode_bf16_fake(
    q, kcache, vcache, block_ids, num_seq_kvcache, mtp, new_kv_included, splitk,
    task_map=None, split_flag=None, output=None,
):
    return torch.empty_like(q)


@torch.library.register_fake("hpc::attention_decode_fp8")
def attention_decode_fp8_fake(
    q, kcache, vcache, block_ids, num_seq_kvcache, qscale, kscale, vscale, mtp, new_kv_included,
    quant_type, splitk, task_map=None, split_flag=None, output=None,
):
    return torch.empty_like(q, dtype=torch.bfloat16)


def attention_with_kvcache_prefill_fp8(
    q: Tensor,
    kcache: Tensor,
    vcache: Tensor,
    qscale: Tensor,
    kscale: Tensor,
    vscale: Tensor,
    cu_seqlens_q: Tensor,
    block_ids: Tensor,
    seqlens_kvcache: Tensor,
    max_seqlens_q: int,
    quant_type: QuantType = QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR,
    output: Tensor = None,
) -> Tensor:
    """Causal paged-KV prefill attention with FP8 q/k/v (reference hpc/attention.py:148-251).

    q e4m3 [total_seq, Hq, 128]; kcache / vcache e4m3 logical [num_blocks, block_size, Hkv, 128] (NHD or
    HND-backed strides); qscale f32 [num_batch, Hq, max_seqlens_q_pad] (per token, per head);
    kscale f32 [1] / vscale f32 [1] (per tensor) or the K-scale tail rows + vscale [Hkv];
    cu_seqlens_q int32 [num_batch+1]; block_ids int32 [num_batch, max_blocks]; seqlens_kvcache int32
    [num_batch]: tokens of each request in the cache, the request's q tokens being the last ones (q row s
    attends keys j <= L - Sq + s, as in the reference tests' oracle).  Returns bf16 [total_seq, Hq, 128]."""
    return torch.ops.hpc.attention_with_kvcache_prefill_fp8(
        q, kcache, vcache, qscale, kscale, vscale, cu_seqlens_q, block_ids, seqlens_kvcache, int(max_seqlens_q),
        quant_type.value, output)


@torch.library.register_fake("hpc::attention_with_kvcache_prefill_fp8")
def _attention_with_kvcache_prefill_fp8_fake(q, kcache, vcache, qscale, kscale, vscale, cu_seqlens_q, block_ids,
                                             seqlens_kvcache, max_seqlens_q, quant_type, output=None):
    if output is not None:
        return output
    return torch.empty((q.shape[0], q.shape[1], vcache.shape[-1]), dtype=torch.bfloat16, device=q.device)


def attention_with_kvcache_blocksparse_prefill_fp8(
    q: Tensor,
    kcache: Tensor,
    vcache: Tensor,
    qscale: Tensor,
    kscale: Tensor,
    vscale: Tensor,
    cu_seqlens_q: Tensor,
    block_ids: Tensor,
    seqlens_kvcache: Tensor,
    max_seqlens_q: int,
    quant_type: QuantType = QuantType.QPERTOKEN_PERHEAD_KPERTENSOR_VPERTENSOR,
    block_mask: Tensor = None,
    output: Tensor = None,
) -> Tensor:
    """Dense / block-sparse causal prefill over the paged FP8 cache (reference hpc/attention.py:253-339).
    Arguments as attention_with_kvcache_prefill_fp8 plus block_mask uint8
    [num_batch, num_head_q, ceil(max_seqlens_q/128), Kb]: only 128 x 128 (q positions x kv tokens) tiles marked
    non-zero are attended (None = dense).  Keep the causal diagonal tile of every q tile set: a q row with no
    active key yields zeros here (NaN in the reference's PyTorch model)."""
    return torch.ops.hpc.attention_with_kvcache_blocksparse_prefill_fp8(
        q, kcache, vcache, qscale, kscale, vscale, cu_seqlens_q, block_ids, seqlens_kvcache, int(max_seqlens_q),
        quant_type.value, block_mask, output)


@torch.library.register_fake("hpc::attention_with_kvcache_blocksparse_prefill_fp8")
def _attention_blocksparse_prefill_fp8_fake(q, kcache, vcache, qscale, kscale, vscale, cu_seqlens_q, block_ids,
                                            seqlens_kvcache, max_seqlens_q, quant_type, block_mask=None, output=None):
    if output is not None:
        return output
    return torch.empty((q.shape[0], q.shape[1], vcache.shape[-1]), dtype=torch.bfloat16, device=q.device)


def attention_prefill_bf16(q: Tensor, k: Tensor, v: Tensor, seqlens_q: Tensor, cu_seqlens_q: Tensor,
                           max_seqlens_q: int, output: Tensor = None) -> Tensor:
    """Causal varlen prefill attention in bf16 over contiguous K/V (reference hpc/attention.py:15-68).
    q [total_seq, Hq, 128], k / v [total_seq, Hkv, 128] bf16; seqlens_q int32 [B]; cu_seqlens_q int32 [B+1];
    token s of a request attends tokens 0..s of the same request.  Returns bf16 [total_seq, Hq, 128]."""
    return torch.ops.hpc.attention_prefill_bf16(q, k, v, seqlens_q, cu_seqlens_q, int(max_seqlens_q), output)


def attention_with_kvcache_prefill_bf16(q: Tensor, kcache: Tensor, vcache: Tensor, cu_seqlens_q: Tensor,
                                        block_ids: Tensor, seqlens_kvcache: Tensor, max_seqlens_q: int,
                                        output: Tensor = None) -> Tensor:
    """Causal prefill attention in bf16 over the paged KV cache (reference hpc/attention.py:70-146).
    q [total_seq, Hq, 128]; kcache / vcache logical [num_blocks, block_size, Hkv, 128] (NHD or HND-backed
    strides); cu_seqlens_q int32 [B+1]; block_ids int32 [B, max_blocks]; seqlens_kvcache int32 [B] = cached
    tokens of each request, its q tokens being the last ones (q row s attends keys j <= L - Sq + s).
    Returns bf16 [total_seq, Hq, 128]."""
    return torch.ops.hpc.attention_with_kvcache_prefill_bf16(q, kcache, vcache, cu_seqlens_q, block_ids,
                                                             seqlens_kvcache, int(max_seqlens_q), output)


@torch.library.register_fake("hpc::attention_prefill_bf16")
def _attention_prefill_bf16_fake(q, k, v, seqlens_q, cu_seqlens_q, max_seqlens_q, output=None):
    return output if output is not None else torch.empty((q.shape[0], q.shape[1], v.shape[-1]), dtype=q.dtype,
                                                         device=q.device)


@torch.library.register_fake("hpc::attention_with_kvcache_prefill_bf16")
def _attention_with_kvcache_prefill_bf16_fake(q, kcache, vcache, cu_seqlens_q, block_ids, num_seq_kvcache,
                                              max_seqlens_q, output=None):
    return output if output is not None else torch.empty((q.shape[0], q.shape[1], vcache.shape[-1]), dtype=q.dtype,
                                                         device=q.device)


def _decode_mla_result(out, lse, output, output_lse, return_lse):
    out = out if output is None else output
    if not (return_lse or output_lse is not None):
        return out
    return out, (lse if output_lse is None else output_lse)


def attention_decode_mla_bf16(q: Tensor, ckv_cache: Tensor, block_ids: Tensor, num_seq_kvcache: Tensor,
                              softmax_scale: float, mtp: int = 0, new_kv_included: bool = False, *, output: Tensor = None,
                              output_lse: Tensor = None, return_lse: bool = False, splits: int = 0):
    """Multi-head latent attention (MLA) decode in its weight-absorbed form over the paged latent KV cache, bfloat16
    (DeepSeek-V3 / R1, Kimi-K2 decode steps).  Returns out bf16 [B * Sq, H, 512], or (out, lse) with return_lse or
    output_lse.

    No reference counterpart; semantics = the PyTorch statement tests/mla_ref.py, in float64.  One latent row per token
    is the key of every head (all 576 columns) and its value (the first 512).  With Sq = mtp + 1 and L_b the tokens of
    request b including the Sq new ones, row (b, s, h) sees tokens j < L_b - Sq + s + 1 (causal among the new tokens):

        z_j = softmax_scale * sum_{d < 576} q[b * Sq + s, h, d] * c_b[j, d]
        out[b * Sq + s, h, :] = bf16( sum_j softmax(z)_j * c_b[j, :512] )
        lse[b * Sq + s, h]    = log sum_j exp(z_j)                      (float32, natural log)

    Layouts:
      q                bfloat16 [B * Sq, H, 576], contiguous: columns 0..511 are q_nope already multiplied by W_UK
                       (latent space), columns 512..575 the RoPE part;
      ckv_cache        bfloat16, logical [num_blocks, P, 576]: one latent row per token, 512 compressed KV + 64 RoPE'd
                       k_pe.  Any block stride that is a multiple of 8 elements, token stride >= 576 and a multiple of 8,
                       last dim contiguous, base 16-byte aligned: padded rows and a view into a larger pool both work;
      block_ids        int32 [B, max_blocks] page table; entries past a request's pages are never dereferenced;
      num_seq_kvcache  int32 [B] on the device: the tokens before this step, or including the Sq new ones with
                       new_kv_included (the convention of attention_decode_bf16; the new tokens' rows are in the cache).
                       Nothing on the host depends on its values: a captured hipGraph replayed after the lengths
                       changed gives the new lengths' result;
      softmax_scale    explicit: 1 / sqrt(128 + 64) times the model's YaRN factor - it is not guessed from 576;
      output           bfloat16 [B * Sq, H, 512] and output_lse float32 [B * Sq, H], contiguous.  When given they are
                       written and returned (the same objects) and nothing is allocated per call beyond the cached
                       scratch, so the call captures into a hipGraph.

    Limits: H % 16 == 0, 16 <= H <= 128; mtp 0..3; P in {16, 32, 64, 128}.  B == 0 returns empty tensors without a
    launch.  Every row must see at least one token.  NaN / Inf inputs: unspecified.  Finite values in page tails, in
    pages no block table lists and in later new tokens of the same request do not influence the result.

    splits: the number of pieces each request's token range is cut into, each piece a workgroup of its own per 64 q
    rows (r = s * H + h).  0 = the library chooses (one piece when the batch fills the CUs, else about two workgroups
    per CU); 1 .. max = the caller's count, max = 64; beyond it the call is refused.  The piece length of request b is
    ceil(L_b / splits) rounded up to the kernel's KV tile of 64 tokens, computed on the device; a piece that starts at
    or past L_b is empty, writes nothing and is never read.  With splits == 1 the kernel writes out directly; otherwise
    the pieces go through a cached scratch buffer per (device, stream, hipGraph capture), which
    hpc.release_decode_workspaces() drops, and a second launch merges them.

    Determinism: for given shapes, splits and CU count the result is bit-identical from call to call - the merge sums
    the pieces in piece order and no float atomics are used."""
    out, lse = torch.ops.hpc_mla.attention_decode_mla_bf16(q, ckv_cache, block_ids, num_seq_kvcache, float(softmax_scale),
                                                           int(mtp), bool(new_kv_included), output, output_lse,
                                                           bool(return_lse), int(splits))
    return _decode_mla_result(out, lse, output, output_lse, return_lse)


@torch.library.register_fake("hpc_mla::attention_decode_mla_bf16")
def _attention_decode_mla_bf16_fake(q, ckv_cache, block_ids, num_seq_kvcache, softmax_scale, mtp, new_kv_included,
                                    output=None, output_lse=None, return_lse=False, splits=0):
    out = output if output is not None else torch.empty((q.shape[0], q.shape[1], 512), dtype=torch.bfloat16, device=q.device)
    if output_lse is not None:
        lse = output_lse
    elif return_lse:
        lse = torch.empty((q.shape[0], q.shape[1]), dtype=torch.float32, device=q.device)
    else:
        lse = torch.empty((0,), dtype=torch.float32, device=q.device)
    return out, lse


def attention_decode_mla_fp8(q: Tensor, ckv_cache: Tensor, block_ids: Tensor, num_seq_kvcache: Tensor,
                             softmax_scale: float, mtp: int = 0, new_kv_included: bool = False, *, output: Tensor = None,
                             output_lse: Tensor = None, return_lse: bool = False, splits: int = 0):
    """attention_decode_mla_bf16 over an FP8 latent KV cache: 656 bytes per token where the bf16 cache has 1,152, so the
    same memory holds 1.76 x the tokens.  Returns out bf16 [B * Sq, H, 512], or (out, lse) with return_lse or output_lse.
    Only the cache is FP8: q, out and lse are those of attention_decode_mla_bf16, and so is every other argument, limit
    (H % 16 == 0, 16 <= H <= 128; mtp 0..3; P in {16, 32, 64, 128}), the splits rule (0 .. 64), the cached scratch that
    hpc.release_decode_workspaces() drops (shared with the bf16 op), hipGraph capture with caller-provided outputs and
    the determinism statement; num_seq_kvcache is never read on the host.

    ckv_cache is a torch.uint8 tensor, logical [num_blocks, P, 656].  The row of one token:

        bytes   0 .. 511   512 float8_e4m3fn codes: the normalised compressed KV, column d at byte d (offset 0)
        bytes 512 .. 527   four little-endian float32 scales (offset 512); scale g belongs to columns 128 g .. 128 g + 127
        bytes 528 .. 655   64 bfloat16 (offset 528): the RoPE'd k_pe, unquantised

    Last dim contiguous, token stride >= 656 bytes and a multiple of 16, block stride a multiple of 16, base 16-byte
    aligned: padded rows and views into a larger pool work.  Allocate it as torch.empty(num_blocks, P, 656,
    dtype=torch.uint8) and fill it with hpc.mla_rope_norm_store_kv_fp8.

    Semantics = attention_decode_mla_bf16 (tests/mla_ref.py::mla_statement in float64) applied to the dequantised cache,
    whose latent column d < 512 of a token is

        c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] )

    with one float32 multiply and one round-to-nearest-even to bfloat16; columns 512..575 are the bf16 k_pe.  The scales
    may be any finite non-negative float32 (hpc.mla_rope_norm_store_kv_fp8 writes amax / 448 per group and codes
    e4m3fn(lat * (1 / (scale + 1e-8)))); a scale of 0 makes its group zeros.  NaN codes (0x7f / 0xff) and non-finite
    scales in tokens a row can see: unspecified.  The kernel is attention_decode_mla_bf16's behind the gather, which
    dequantises into the same on-chip image: for given shapes, splits and CU count the result is bit-identical to
    attention_decode_mla_bf16 on the dequantised cache, and bit-identical from call to call."""
    out, lse = torch.ops.hpc_mla.attention_decode_mla_fp8(q, ckv_cache, block_ids, num_seq_kvcache, float(softmax_scale),
                                                          int(mtp), bool(new_kv_included), output, output_lse,
                                                          bool(return_lse), int(splits))
    return _decode_mla_result(out, lse, output, output_lse, return_lse)


torch.library.register_fake("hpc_mla::attention_decode_mla_fp8")(_attention_decode_mla_bf16_fake)


def attention_decode_mla_sparse_bf16(q: Tensor, ckv_cache: Tensor, block_ids: Tensor, num_seq_kvcache: Tensor,
                                     indices: Tensor, softmax_scale: float, mtp: int = 0, new_kv_included: bool = False, *,
                                     output: Tensor = None, output_lse: Tensor = None, return_lse: bool = False,
                                     splits: int = 0):
    """Token-sparse MLA decode over the paged latent KV cache, bfloat16: every q row attends to the cache tokens its list
    names, not to the whole context (the attention of a DeepSeek-V3.2 / DSA decode step, whose indexer picks topk = 2048
    tokens per query token).  Returns out bf16 [B * Sq, H, 512], or (out, lse) with return_lse or output_lse - what
    attention_decode_mla_bf16 returns.  The indexer is not part of this op: the indices are taken as given.

    No reference counterpart; semantics = the PyTorch statement tests/mla_sparse_ref.py, in float64.  With Sq = mtp + 1,
    L_b the tokens of request b including the Sq new ones (the new_kv_included convention of attention_decode_mla_bf16)
    and vis(b, s) = L_b - Sq + s + 1, the list of row (b, s) is indices[b * Sq + s, :], shared by all H heads:

        z_k = softmax_scale * sum_{d < 576} q[b * Sq + s, h, d] * c_b[idx_k, d]      over valid k
        out[b * Sq + s, h, :] = bf16( sum_k softmax(z)_k * c_b[idx_k, :512] )
        lse[b * Sq + s, h]    = log sum_k exp(z_k)                                   (float32, natural log)

    indices          int32 [B * Sq, topk], contiguous, on q's device: LOGICAL token positions in the request - what an
                     indexer's top-k yields.  The kernel translates pages through block_ids; no conversion kernel is
                     needed.  topk = indices.shape[1] is a host value, 1 <= topk <= 65536, and need not be a multiple
                     of 64.
    valid entry      0 <= idx_k < vis(b, s), idx_k // P < max_blocks, and its page id in [0, num_blocks).  Every other
                     entry contributes nothing and causes no memory access: -1 padding, any other negative, positions
                     at or past vis (later new tokens included), positions beyond the page table, poisoned page ids.
                     Every address is checked against a host value.
    duplicates       a position listed twice counts twice: the sum runs over entries.
    empty row        a row with no valid entry writes out = 0 and lse = -inf (the convention of
                     attention_prefill_mla_bf16; hpc.merge_attn_states passes the other side through for it).

    q, ckv_cache, block_ids, num_seq_kvcache, softmax_scale (explicit), output and output_lse are those of
    attention_decode_mla_bf16, with its limits: H % 16 == 0, 16 <= H <= 128; mtp 0..3; P in {16, 32, 64, 128}; B == 0
    returns empty tensors without a launch.  Nothing on the host reads num_seq_kvcache, block_ids or indices: with
    output (and output_lse) given nothing is allocated beyond the cached scratch and the call captures into a hipGraph,
    which replayed after lengths, pages, cache and indices changed in place gives the new result.

    splits cuts the LIST, not the context: piece p covers slots [p * plen, min(topk, (p + 1) * plen)) with
    plen = ceil(topk / splits) rounded up to the kernel's tile of 64 slots, computed on the host.  Pieces that would
    start at or past topk are not launched.  0 = the library chooses (one piece when B * Sq * ceil(H / 64) workgroups
    fill the CUs, else about two workgroups per CU, never more pieces than the list has tiles); 1 .. max = the caller's
    count, max = 64; beyond it the call is refused.  More than one piece goes through the cached scratch buffer that
    attention_decode_mla_bf16 uses (hpc.release_decode_workspaces() drops it) and a merge launch that sums the pieces
    in piece order, skipping a piece that saw no token.

    Determinism: no float atomics; for given shapes, splits and CU count the result is bit-identical from call to call.
    Behind the gather the kernel is attention_decode_mla_bf16's: with mtp = 0, splits = 1 and the list 0 .. L_b - 1
    (then -1) the result is bit-identical to attention_decode_mla_bf16 at splits = 1."""
    out, lse = torch.ops.hpc_mla.attention_decode_mla_sparse_bf16(q, ckv_cache, block_ids, num_seq_kvcache, indices,
                                                                  float(softmax_scale), int(mtp), bool(new_kv_included),
                                                                  output, output_lse, bool(return_lse), int(splits))
    return _decode_mla_result(out, lse, output, output_lse, return_lse)


@torch.library.register_fake("hpc_mla::attention_decode_mla_sparse_bf16")
def _attention_decode_mla_sparse_fake(q, ckv_cache, block_ids, num_seq_kvcache, indices, softmax_scale, mtp, new_kv_included,
                                      output=None, output_lse=None, return_lse=False, splits=0):
    return _attention_decode_mla_bf16_fake(q, ckv_cache, block_ids, num_seq_kvcache, softmax_scale, mtp, new_kv_included,
                                           output, output_lse, return_lse, splits)


def attention_decode_mla_sparse_fp8(q: Tensor, ckv_cache: Tensor, block_ids: Tensor, num_seq_kvcache: Tensor,
                                    indices: Tensor, softmax_scale: float, mtp: int = 0, new_kv_included: bool = False, *,
                                    output: Tensor = None, output_lse: Tensor = None, return_lse: bool = False,
                                    splits: int = 0):
    """attention_decode_mla_sparse_bf16 over the FP8 latent KV cache of attention_decode_mla_fp8: a torch.uint8 tensor,
    logical [num_blocks, P, 656] (512 e4m3 codes, four float32 scales, 64 bf16 RoPE columns per token) - the row
    DeepSeek-V3.2's sparse attention reads.  Returns out bf16 [B * Sq, H, 512], or (out, lse) with return_lse or
    output_lse.

    Semantics = the statement of attention_decode_mla_sparse_bf16 (tests/mla_sparse_ref.py) applied to the dequantised
    cache exactly as attention_decode_mla_fp8 does it: c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] ).  indices
    (int32 [B * Sq, topk] logical token positions, 1 <= topk <= 65536), the valid-entry rule (0 <= idx_k < vis(b, s),
    inside the page table, page id in [0, num_blocks); -1 padding and every other invalid entry contribute nothing and
    cause no memory access), the duplicate rule (a position listed twice counts twice), the empty row (out = 0,
    lse = -inf), the limits (H % 16 == 0,
    16 <= H <= 128; mtp 0..3; P in {16, 32, 64, 128}), the splits rule over the list (0 .. 64), the cached scratch that
    hpc.release_decode_workspaces() drops and hipGraph capture with caller-provided outputs are all those of
    attention_decode_mla_sparse_bf16; the cache's stride rule is attention_decode_mla_fp8's.  Only the gather differs:
    for given shapes, splits and CU count the result is bit-identical to attention_decode_mla_sparse_bf16 on the
    dequantised cache, and bit-identical from call to call."""
    out, lse = torch.ops.hpc_mla.attention_decode_mla_sparse_fp8(q, ckv_cache, block_ids, num_seq_kvcache, indices,
                                                                 float(softmax_scale), int(mtp), bool(new_kv_included),
                                                                 output, output_lse, bool(return_lse), int(splits))
    return _decode_mla_result(out, lse, output, output_lse, return_lse)


torch.library.register_fake("hpc_mla::attention_decode_mla_sparse_fp8")(_attention_decode_mla_sparse_fake)


def attention_prefill_mla_sparse_bf16(q: Tensor, ckv_cache: Tensor, block_ids: Tensor, num_seqlen_per_req: Tensor,
                                      q_index: Tensor, indices: Tensor, softmax_scale: float, *, output: Tensor = None,
                                      output_lse: Tensor = None, return_lse: bool = False, splits: int = 0):
    """Token-sparse MLA attention of a ragged PREFILL chunk over the paged latent KV cache, bfloat16: every prompt token
    attends to the cache tokens its list names (DeepSeek-V3.2 / DSA: the top-2048 of hpc.mla_indexer_topk_prefill_fp8).
    Returns out bf16 [T, H, 512], or (out, lse) with return_lse or output_lse - what hpc.mla_unabsorb_o and
    hpc.merge_attn_states take.

    attention_decode_mla_sparse_bf16 with the writers' row rule in the place of mtp; semantics = tests/mla_sparse_ref.py on
    the expanded form (tests/mla_indexer_prefill_ref.py: every row its own one-row request).

    row rule         that of mla_rope_norm_store_kv / mla_indexer_prep_fp8: row r of the chunk belongs to the last request
                     b with q_index[b] <= r, at pos = num_seqlen_per_req[b] - (q_index[b + 1] - r).  num_seqlen_per_req
                     int32 [num_req] (total lengths INCLUDING the chunk's tokens, whose rows are in the cache), q_index
                     int32 [num_req + 1], block_ids int32 [num_req, max_blocks]; all on the device, never read on the
                     host.  A live row sees vis(r) = min(pos + 1, max_blocks * P) tokens: causal inside the chunk, all
                     of the cached context before it - chunked prefill and prefix caching need nothing extra.
    row of no        a row at or past q_index[-1] or with pos < 0: an empty row.
    request
    q, indices       bf16 [T, H, 576] and int32 [T, topk]: row r's list names LOGICAL positions of its request.

    The valid-entry rule (0 <= idx_k < vis(r), inside the page table, page id in [0, num_blocks)), the duplicate rule, the
    empty row (out = 0, lse = -inf), the splits rule over the list (0 .. 64), the limits (H % 16 == 0, 16 <= H <= 128;
    P in {16, 32, 64, 128}; 1 <= topk <= 65536), the cached scratch that hpc.release_decode_workspaces() drops and
    hipGraph capture with caller-provided outputs are attention_decode_mla_sparse_bf16's: the same kernel, one workgroup
    per row, 64 heads and piece.  With q_index = [0, Sq, 2 Sq, ...] the result is bit-identical to that op at mtp = Sq - 1
    and the same splits, and on any chunk to that op on the expanded form.  T == 0 returns empty tensors without a
    launch; num_req == 0 makes every row an empty row."""
    out, lse = torch.ops.hpc_mla.attention_prefill_mla_sparse_bf16(q, ckv_cache, block_ids, num_seqlen_per_req, q_index, indices,
                                                                   float(softmax_scale), output, output_lse, bool(return_lse),
                                                                   int(splits))
    return _decode_mla_result(out, lse, output, output_lse, return_lse)


@torch.library.register_fake("hpc_mla::attention_prefill_mla_sparse_bf16")
def _attention_prefill_mla_sparse_fake(q, ckv_cache, block_ids, num_seqlen_per_req, q_index, indices, softmax_scale, output=None,
                                       output_lse=None, return_lse=False, splits=0):
    return _attention_decode_mla_bf16_fake(q, ckv_cache, block_ids, num_seqlen_per_req, softmax_scale, 0, True, output, output_lse,
                                           return_lse, splits)


def attention_prefill_mla_sparse_fp8(q: Tensor, ckv_cache: Tensor, block_ids: Tensor, num_seqlen_per_req: Tensor,
                                     q_index: Tensor, indices: Tensor, softmax_scale: float, *, output: Tensor = None,
                                     output_lse: Tensor = None, return_lse: bool = False, splits: int = 0):
    """attention_prefill_mla_sparse_bf16 over the FP8 latent KV cache of attention_decode_mla_fp8 (torch.uint8, logical
    [num_blocks, P, 656]).  Returns out bf16 [T, H, 512], or (out, lse) with return_lse or output_lse.

    The row rule (num_seqlen_per_req, q_index, rows of no request), the lists and every other rule are those of
    attention_prefill_mla_sparse_bf16; the cache, its dequantisation c[d] = bf16_rne( fp32(code[d]) * scale[d // 128] ) and
    its stride rule are attention_decode_mla_sparse_fp8's.  For given shapes, splits and CU count the result is
    bit-identical to attention_decode_mla_sparse_fp8 on the expanded form, and bit-identical from call to call; the call
    captures into a hipGraph with caller-provided outputs."""
    out, lse = torch.ops.hpc_mla.attention_prefill_mla_sparse_fp8(q, ckv_cache, block_ids, num_seqlen_per_req, q_index, indices,
                                                                  float(softmax_scale), output, output_lse, bool(return_lse),
                                                                  int(splits))
    return _decode_mla_result(out, lse, output, output_lse, return_lse)


torch.library.register_fake("hpc_mla::attention_prefill_mla_sparse_fp8")(_attention_prefill_mla_sparse_fake)


def attention_prefill_mla_bf16(q: Tensor, k_nope: Tensor, k_pe: Tensor, v: Tensor, cu_seqlens_q: Tensor, max_seqlens_q: int,
                               softmax_scale: float, *, cu_seqlens_k: Tensor = None, max_seqlens_k: int = None,
                               causal: bool = True, output: Tensor = None, output_lse: Tensor = None,
                               return_lse: bool = False):
    """Multi-head latent attention (MLA) prefill in its non-absorbed form, bfloat16: q / k heads of 192 columns (128 "nope" +
    64 RoPE), v heads of 128 (DeepSeek-V3 / R1, Kimi-K2 prompts and prompt chunks).  Returns out bf16 [Tq, H, 128], or
    (out, lse) with return_lse or output_lse.

    No reference counterpart; semantics = the PyTorch statement tests/mla_prefill_ref.py, in float64.  Request b has
    Sq = cu_seqlens_q[b + 1] - cu_seqlens_q[b] q rows and Lk = cu_seqlens_k[b + 1] - cu_seqlens_k[b] keys.  With causal, row s
    sees keys j <= Lk - Sq + s (bottom-right aligned, the convention of attention_with_kvcache_prefill_bf16); without it
    every j < Lk:

        z_j = softmax_scale * (q[s, h, :128] . k_nope[j, h] + q[s, h, 128:] . k_pe[j])
        out[s, h, :] = bf16( sum_j softmax(z)_j * v[j, h, :] )
        lse[s, h]    = log sum_j exp(z_j)                                (float32, natural log)

    A row that sees no key - Lk == 0 (a request without a prefix in the context pass), or Lk - Sq + s < 0 - writes out = 0
    and lse = -inf.  Such a row is legal: merge_attn_states passes the other side through for it.

    Layouts (no concat or copy between the producers and this call):
      q              bfloat16 [Tq, H, 192]: columns 0..127 nope, 128..191 with RoPE already applied -
                     hpc.mla_rope_norm_store_kv(..., q_pe=q[..., 128:], out_q_pe=q[..., 128:]) does that in place.  Last dim
                     contiguous, row and head strides multiples of 8 elements and >= 192, base 16-byte aligned;
      k_nope, v      bfloat16 [Tk, H, 128], any row / head strides that are multiples of 8 and >= 128: the two halves
                     kv[..., :128] and kv[..., 128:] of the kv_b projection's [Tk, H, 256] output, passed as views;
      k_pe           bfloat16 [Tk, 64], ONE RoPE'd head shared by all H heads, row stride a multiple of 8 and >= 64:
                     out_ckv[:, 512:] of hpc.mla_rope_norm_store_kv (row stride 576).  The kernel reads it once per KV tile of a
                     workgroup; no [Tk, H, 192] tensor is ever materialised;
      cu_seqlens_q   int32 [B + 1] on the device; cu_seqlens_k int32 [B + 1], or None meaning the same tensor as cu_seqlens_q
                     (self-attention of the chunk); given, it needs max_seqlens_k.  Only the two max_* ints are read on the
                     host: a captured hipGraph replayed after the device lengths changed (same maxima) follows the new lengths;
      softmax_scale  explicit: 1 / sqrt(192) times the model's YaRN factor; positive and finite;
      output         bfloat16 [Tq, H, 128] and output_lse float32 [Tq, H], contiguous.  When given they are written and
                     returned (the same objects) and nothing is allocated per call, so the call captures into a hipGraph.

    Limits: 1 <= H <= 65535, any value (group 1: nothing needs a power of two); B <= 65535; row strides <= 2^25 elements.
    B == 0 or Tq == 0 returns without a launch.  Refused: misaligned bases or strides, strides under 192 / 128 / 64,
    cu_seqlens_k without max_seqlens_k, negative counts.  NaN / Inf inputs: unspecified.  Reads are bounded by the rows of the
    request that exist: finite values in rows of other requests, in rows past cu_seqlens[-1] and in the columns around the
    views do not influence the result.  No float atomics: bit-identical from call to call."""
    out, lse = torch.ops.hpc_mla.attention_prefill_mla_bf16(
        q, k_nope, k_pe, v, cu_seqlens_q, int(max_seqlens_q), float(softmax_scale), cu_seqlens_k,
        None if max_seqlens_k is None else int(max_seqlens_k), bool(causal), output, output_lse, bool(return_lse))
    out = out if output is None else output
    if not (return_lse or output_lse is not None):
        return out
    return out, (lse if output_lse is None else output_lse)


@torch.library.register_fake("hpc_mla::attention_prefill_mla_bf16")
def _attention_prefill_mla_bf16_fake(q, k_nope, k_pe, v, cu_seqlens_q, max_seqlens_q, softmax_scale, cu_seqlens_k=None,
                                     max_seqlens_k=None, causal=True, output=None, output_lse=None, return_lse=False):
    out = output if output is not None else torch.empty((q.shape[0], q.shape[1], 128), dtype=torch.bfloat16, device=q.device)
    if output_lse is not None:
        lse = output_lse
    elif return_lse:
        lse = torch.empty((q.shape[0], q.shape[1]), dtype=torch.float32, device=q.device)
    else:
        lse = torch.empty((0,), dtype=torch.float32, device=q.device)
    return out, lse


def merge_attn_states(out_a: Tensor, lse_a: Tensor, out_b: Tensor, lse_b: Tensor, *, output: Tensor = None,
                      output_lse: Tensor = None):
    """Merge two attention results over disjoint key sets by their log-sum-exps into the result over the union: the step
    that comes with chunked prefill and prefix caching (a chunk's causal self pass and its non-causal pass over the cached
    context, both from attention_prefill_mla_bf16 with return_lse).  Returns (out, lse).

    No reference counterpart; semantics = tests/mla_prefill_ref.py::merge_statement.  In float32 with one rounding to bf16, per
    (row, head):

        m = max(la, lb)    wa = exp(la - m)    wb = exp(lb - m)
        out = (wa a + wb b) / (wa + wb)        lse = m + log(wa + wb)

    A side whose lse is -inf (it saw no key) passes the other side through bit for bit; both -inf give zeros and -inf.

    out_a, out_b   bfloat16 [T, H, D], D % 8 == 0, D <= 512, last dim contiguous, row / head strides multiples of 8 and >= D,
                   base 16-byte aligned;
    lse_a, lse_b   float32 [T, H], contiguous, natural log;
    output         bfloat16 [T, H, D] under the rules of out_a, output_lse float32 [T, H]: written and returned (the same
                   objects), nothing allocated.  output may be out_a itself and output_lse may be lse_a (merge in place); any
                   other overlap of an output with an input is refused.
    T == 0 or H == 0 returns without a launch.  NaN / +Inf lse: unspecified.  A small streaming kernel (16-byte loads and
    stores, one lane group per row of one head); bit-identical from call to call."""
    out, lse = torch.ops.hpc_mla.merge_attn_states(out_a, lse_a, out_b, lse_b, output, output_lse)
    return (out if output is None else output), (lse if output_lse is None else output_lse)


@torch.library.register_fake("hpc_mla::merge_attn_states")
def _merge_attn_states_fake(out_a, lse_a, out_b, lse_b, output=None, output_lse=None):
    out = output if output is not None else torch.empty(out_a.shape, dtype=torch.bfloat16, device=out_a.device)
    lse = output_lse if output_lse is not None else torch.empty(lse_a.shape, dtype=torch.float32, device=lse_a.device)
    return out, lse


def mla_gather_ckv(ckv_cache: Tensor, block_ids: Tensor, cu_seqlens: Tensor, *, seq_starts: Tensor = None,
                   output: Tensor = None, num_rows: int = None) -> Tensor:
    """Gather rows of the paged MLA latent cache (bfloat16) into one contiguous tensor: the step between the cache and the
    kv_b projection in the context pass of chunked prefill and prefix caching.  Returns bfloat16 [T, 576] with the shape
    and meaning of mla_rope_norm_store_kv's out_ckv: out[:, :512] feeds kv_b, out[:, 512:] is the k_pe operand of
    attention_prefill_mla_bf16 (row stride 576).

    No reference counterpart; semantics = the PyTorch statement tests/mla_gather_ref.py, which holds no float.  Request b
    owns the output rows cu_seqlens[b] <= r < cu_seqlens[b + 1]; row r is the token at position
    pos = seq_starts[b] + (r - cu_seqlens[b]), seq_starts = 0 when it is not given:

        out[r, :] = ckv_cache[block_ids[b, pos // P], pos % P, :576]          (the bits, untouched: no arithmetic)

    Layouts (all on one device):
      ckv_cache   bfloat16, logical [num_blocks, P, 576], P in {16, 32, 64, 128}; the stride rules of
                  attention_decode_mla_bf16: block and token strides multiples of 8 elements, token stride >= 576, last dim
                  contiguous, base 16-byte aligned (padded rows, views into a larger pool).  Cache offsets are 64-bit;
      block_ids   int32 [B, max_blocks] page table; cu_seqlens int32 [B + 1]; seq_starts int32 [B], the first context
                  position of each request in this pass (hpc.mla_context_chunks plans the passes);
      output      bfloat16 [T, 576], last dim contiguous, row stride a multiple of 8 and >= 576, base 16-byte aligned.
                  Given, it is written and returned (the same object), nothing is allocated and the call captures into a
                  hipGraph; otherwise num_rows (a host int) sizes a fresh contiguous tensor.  The call is refused when
                  both are absent, or when they disagree.
    Nothing on the host reads cu_seqlens, seq_starts or block_ids: T is output.shape[0] or num_rows, and a captured
    hipGraph replayed after the device lengths changed follows the new lengths.  T == 0 or B == 0 returns without a launch.

    Guards: rows that belong to no request (r < cu_seqlens[0], r >= cu_seqlens[B]) are not written and stay byte-identical,
    and so do the bytes between the 576 columns and a wider row stride.  A row of a request whose token cannot be fetched
    is written as 576 zeros: pos < 0, pos // P >= max_blocks, or a page id outside [0, num_blocks) - frameworks pad tables
    with -1.  Memory safety does not depend on any device value: every index is checked against a host value, and with a
    cu_seqlens that does not ascend a negative count is an empty request."""
    out = torch.ops.hpc_mla.gather_ckv(ckv_cache, block_ids, cu_seqlens, seq_starts, output,
                                       None if num_rows is None else int(num_rows))
    return out if output is None else output


@torch.library.register_fake("hpc_mla::gather_ckv")
def _mla_gather_ckv_fake(ckv_cache, block_ids, cu_seqlens, seq_starts=None, output=None, num_rows=None):
    if output is not None:
        return output
    if num_rows is None:
        raise RuntimeError("one of output and num_rows must be given: the row count is a host value")
    return torch.empty((num_rows, 576), dtype=torch.bfloat16, device=ckv_cache.device)


def mla_gather_ckv_fp8(ckv_cache: Tensor, block_ids: Tensor, cu_seqlens: Tensor, *, seq_starts: Tensor = None,
                       output: Tensor = None, num_rows: int = None) -> Tensor:
    """mla_gather_ckv over the FP8 latent KV cache that hpc.mla_rope_norm_store_kv_fp8 writes and attention_decode_mla_fp8
    reads: the gather and the dequantisation in one pass.  Returns bfloat16 [T, 576].  Arguments, the row-to-position rule
    (request b owns rows cu_seqlens[b] <= r < cu_seqlens[b + 1], pos = seq_starts[b] + (r - cu_seqlens[b])), output /
    num_rows, the guards (rows of no request are not written; pos < 0, pos // P >= max_blocks or a page id outside
    [0, num_blocks) give 576 zeros; no device value is trusted with an address) and the hipGraph statement are those of
    mla_gather_ckv; nothing on the host reads cu_seqlens, seq_starts or block_ids.

    ckv_cache is a torch.uint8 tensor, logical [num_blocks, P, 656], P in {16, 32, 64, 128}: last dim contiguous, token
    stride >= 656 bytes and a multiple of 16, block stride a multiple of 16, base 16-byte aligned.  With code, scale and the
    RoPE part read from the 656-byte row of the token (bytes 0 .. 511, 512 .. 527, 528 .. 655):

        out[r, d]    = bf16_rne( fp32(code[d]) * scale[d // 128] ),  d < 512     one float32 multiply, one rounding
        out[r, 512:] = the 64 bfloat16 at byte offset 528                        (the bits, untouched)

    That is tests/mla_fp8_ref.py::dequantise of the row, the dequantisation attention_decode_mla_fp8 applies
    (csrc/mla_fp8_format.h): a prompt chunk and a decode step read the same keys from the same cache, bit for bit.  A scale
    of 0 makes its group zeros.  NaN codes (0x7f / 0xff) and non-finite scales: unspecified."""
    out = torch.ops.hpc_mla.gather_ckv_fp8(ckv_cache, block_ids, cu_seqlens, seq_starts, output,
                                           None if num_rows is None else int(num_rows))
    return out if output is None else output


torch.library.register_fake("hpc_mla::gather_ckv_fp8")(_mla_gather_ckv_fake)


def mla_absorb_q(q_nope: Tensor, w_uk: Tensor, *, output: Tensor = None) -> Tensor:
    """The first absorb matmul of an MLA decode step: W_UK folded into the query, per head.  Returns bfloat16 [T, H, 512],
    the first 512 columns of the q that attention_decode_mla_bf16 / _fp8 take.

    No reference counterpart; semantics = tests/mla_absorb_ref.py::absorb_q_statement.  With fp32 accumulation and one rounding:

        out[t, h, c] = bf16( sum_{d < 128} float(q_nope[t, h, d]) * float(w_uk[h, d, c]) ),   c < 512

    q_nope   bfloat16 [T, H, 128], last dim contiguous, row and head strides multiples of 8 elements, base 16-byte aligned:
             q[..., :128] of the q_b output [T, H, 192] is taken as it stands, columns 128 .. 191 are never read;
    w_uk     bfloat16 [H, 128, 512], last dim contiguous, head and d strides multiples of 8 elements: the view
             w_kv_b.view(H, 256, 512)[:, :128] of the dequantised kv_b_proj weight [H * 256, 512], without a copy (the
             kernel transposes on chip);
    output   bfloat16 [T, H, 512] under q_nope's stride rules, heads and rows not overlapping: q_abs[..., :512] of the
             [T, H, 576] buffer is written in place and its columns 512 .. 575 - where mla_rope_norm_store_kv(out_q_pe=)
             puts q_pe - are never touched, in either call order.  Given, it is written and returned (the same object),
             nothing is allocated, nothing is read on the host and the call captures into a hipGraph; otherwise a contiguous
             tensor is returned.  An output that shares bytes with an input is refused.
    1 <= H <= 128 (no multiple-of-16 rule); T == 0 returns without a launch; offsets are 64-bit.  No split-K, no atomics, no
    workspace: bit-identical from call to call."""
    out = torch.ops.hpc_mla.absorb_q(q_nope, w_uk, output)
    return out if output is None else output


@torch.library.register_fake("hpc_mla::absorb_q")
def _mla_absorb_q_fake(q_nope, w_uk, output=None):
    if output is not None:
        return output
    return torch.empty((q_nope.shape[0], q_nope.shape[1], 512), dtype=torch.bfloat16, device=q_nope.device)


def mla_unabsorb_o(o_lat: Tensor, w_uv: Tensor, *, output: Tensor = None, quant: bool = False, output_scale: Tensor = None):
    """The second absorb matmul of an MLA decode step: W_UV applied to the latent attention output, per head, laid out for
    the output projection.  quant=False returns bfloat16 [T, H * 128]; quant=True returns the (x, x_scale) pair of
    gemm_blockwise_fp8: (codes float8_e4m3fn [T, H * 128], scale float32 [T, H]) - a head's 128 columns are one block.

    No reference counterpart; semantics = tests/mla_absorb_ref.py::unabsorb_o_statement.  fp32 accumulation, one rounding:

        o[t, h * 128 + v] = bf16( sum_{c < 512} float(o_lat[t, h, c]) * float(w_uv[h, v, c]) ),   v < 128
        quant:  scale[t, h] = amax_v |o| / 448      codes = e4m3fn( o * (1 / (scale + 1e-8)) )     on the bf16-rounded o

    The quantised pair is bit-identical to hpc.blockwise_fp8_quant(hpc.mla_unabsorb_o(..., quant=False)), and the bf16 values
    behind it are the same bits in both modes (the same accumulation order).

    o_lat    bfloat16 [T, H, 512], the decode op's output; last dim contiguous, row and head strides multiples of 8 elements,
             base 16-byte aligned;
    w_uv     bfloat16 [H, 128, 512], last dim contiguous, head and row strides multiples of 8: the view
             w_kv_b.view(H, 256, 512)[:, 128:] of the same kv_b weight, without a copy;
    output   quant=False: bfloat16 [T, H * 128], last dim contiguous, row stride a multiple of 8 and >= H * 128;
             quant=True: float8_e4m3fn [T, H * 128] and output_scale float32 [T, H], both contiguous.  Given, they are written
             and returned (the same objects), nothing is allocated or read on the host and the call captures into a hipGraph.
    1 <= H <= 128; T == 0 returns empty tensors without a launch; offsets are 64-bit.  No split-K, no atomics, no workspace:
    bit-identical from call to call."""
    o, s = torch.ops.hpc_mla.unabsorb_o(o_lat, w_uv, output, bool(quant), output_scale)
    o = o if output is None else output
    if not quant:
        return o
    return o, (s if output_scale is None else output_scale)


@torch.library.register_fake("hpc_mla::unabsorb_o")
def _mla_unabsorb_o_fake(o_lat, w_uv, output=None, quant=False, output_scale=None):
    t, h = o_lat.shape[0], o_lat.shape[1]
    if output_scale is not None and not quant:
        raise RuntimeError("output_scale needs quant=True")
    o = output if output is not None else torch.empty(
        (t, h * 128), dtype=torch.float8_e4m3fn if quant else torch.bfloat16, device=o_lat.device)
    if not quant:
        return o, torch.empty((0,), dtype=torch.float32, device=o_lat.device)
    s = output_scale if output_scale is not None else torch.empty((t, h), dtype=torch.float32, device=o_lat.device)
    return o, s


def mla_context_chunks(context_lens, workspace_rows: int):
    """Plan the context passes of chunked prefill on the host: cut every request's cached context [0, L_b) into passes so
    that one pass gathers at most workspace_rows rows in all (the bound of the mla_gather_ckv output and of the kv_b
    projection behind it).  context_lens is a sequence of B host ints - schedulers hold them on the host - and no device
    memory is read.

    Every pass gives each request the same share = workspace_rows // B rounded down to a multiple of 128 rows; a
    workspace_rows below 128 * B is refused.  Pass p covers positions [p * share, min((p + 1) * share, L_b)) of request b;
    a request whose context is exhausted contributes 0 rows.  There are ceil(max_b L_b / share) passes, none with all
    lengths 0.

    Returns a list with one tuple per pass:
      seq_starts  CPU int32 tensor [B], for mla_gather_ckv(seq_starts=...);
      cu_seqlens  CPU int32 tensor [B + 1], for mla_gather_ckv and attention_prefill_mla_bf16(cu_seqlens_k=...);
      max_len     int, the longest piece of the pass, for max_seqlens_k."""
    lens = [int(n) for n in context_lens]
    workspace_rows = int(workspace_rows)
    if any(n < 0 for n in lens):
        raise ValueError("context_lens must not be negative")
    if not lens or max(lens) == 0:
        return []
    share = workspace_rows // len(lens) // 128 * 128
    if share < 128:
        raise ValueError(f"workspace_rows = {workspace_rows} is below 128 rows for each of the {len(lens)} requests")
    passes = []
    for first in range(0, max(lens), share):
        counts = [min(share, max(n - first, 0)) for n in lens]
        cu = [0]
        for c in counts:
            cu.append(cu[-1] + c)
        passes.append((torch.tensor([min(first, n) for n in lens], dtype=torch.int32), torch.tensor(cu, dtype=torch.int32),
                       max(counts)))
    return passes
