// MLA prefill attention in the non-absorbed form (attention_prefill_mla.hip: q / k heads of 128 nope + 64 RoPE columns, v heads of
// 128, k_pe one head shared by all): on which grid a call runs, or why it is refused - mla_prefill_route() is the one statement of
// it.  Internal header, host only, no HIP calls: a pure function of the call's addresses (their alignment only), strides and
// counts.  Nothing here depends on the lengths of the requests: they stay on the device.
#pragma once
#include <stdint.h>

#include "hpc_common.h"
#include "mla_cache.h"

namespace hpc {

constexpr int kMlaPrefillDimNope = 128;  // q / k columns without RoPE, and the v head
constexpr int kMlaPrefillDimPe = kMlaRope;  // RoPE columns: behind the nope columns in q, one shared head in k_pe
constexpr int kMlaPrefillDimQk = kMlaPrefillDimNope + kMlaPrefillDimPe;
constexpr int kMlaPrefillRowTile = 128;  // q positions of one head per workgroup: four waves x 32 rows
constexpr int kMlaPrefillKvTile = 64;    // tokens per LDS image
constexpr int kMlaPrefillThreads = 256;
// the kernel forms a tile's row offsets and its buffer limits in 32 bits: 16 rows x stride x 2 bytes must stay below 2^31
constexpr int64_t kMlaPrefillMaxRowStride = int64_t{1} << 25;

struct MlaPrefillCall {  // what the call is; strides in ELEMENTS (bf16)
  uintptr_t out, q, k_nope, k_pe, v, cu_seqlens_q;  // addresses: looked at for null and alignment, never dereferenced
  uintptr_t lse;                                    // may be null: no lse wanted
  uintptr_t cu_seqlens_k;                           // null: the same array as cu_seqlens_q
  int num_batch, num_head, max_seqlens_q, max_seqlens_k;  // max_seqlens_k < 0: not given
  int64_t q_row_stride, q_head_stride, k_row_stride, k_head_stride, k_pe_row_stride, v_row_stride, v_head_stride;
  float softmax_scale;
};

struct MlaPrefillRoute {
  int code;   // HPC_OK or the refusal; nothing below is set on a refusal
  int empty;  // no request or no q token: HPC_OK with nothing launched (and nothing below set)
  int grid_x, grid_y, grid_z, threads;  // (128-position q tiles of the longest request, heads, requests)
};

// Refusals in this order (a call with two faults gets the code of the earlier one):
//   1. a null out, q, k_nope, k_pe, v or cu_seqlens_q                                       HPC_ERR_INVALID
//   2. a base that is not 16-byte aligned (lse, the cu arrays: 4), a stride that is no multiple of 8    HPC_ERR_UNSUPPORTED
//   3. q row / head stride under 192, k_nope / v row / head stride under 128, k_pe row stride under 64  HPC_ERR_UNSUPPORTED
//   4. cu_seqlens_k given without max_seqlens_k                                              HPC_ERR_INVALID
//   5. a negative num_batch or max_seqlens_q, num_head <= 0, a softmax_scale that is not a positive finite number  HPC_ERR_INVALID
//   6. num_head or num_batch beyond 65535 (grid y, z), a row stride beyond 2^25 elements     HPC_ERR_UNSUPPORTED
// then the empty call.  (static: the product and the development library may sit in one process, and each must call its own)
static inline MlaPrefillRoute mla_prefill_route(const MlaPrefillCall& c) {
  MlaPrefillRoute r{};
  auto refuse = [&r](int code) { return r.code = code, r; };
  if (!c.out || !c.q || !c.k_nope || !c.k_pe || !c.v || !c.cu_seqlens_q) return refuse(HPC_ERR_INVALID);
  if (((c.out | c.q | c.k_nope | c.k_pe | c.v) & 15) || ((c.lse | c.cu_seqlens_q | c.cu_seqlens_k) & 3) ||
      ((c.q_row_stride | c.q_head_stride | c.k_row_stride | c.k_head_stride | c.k_pe_row_stride | c.v_row_stride | c.v_head_stride) & 7))
    return refuse(HPC_ERR_UNSUPPORTED);
  if (c.q_row_stride < kMlaPrefillDimQk || c.q_head_stride < kMlaPrefillDimQk || c.k_row_stride < kMlaPrefillDimNope ||
      c.k_head_stride < kMlaPrefillDimNope || c.v_row_stride < kMlaPrefillDimNope || c.v_head_stride < kMlaPrefillDimNope ||
      c.k_pe_row_stride < kMlaPrefillDimPe)
    return refuse(HPC_ERR_UNSUPPORTED);
  if (c.cu_seqlens_k && c.max_seqlens_k < 0) return refuse(HPC_ERR_INVALID);
  if (c.num_batch < 0 || c.max_seqlens_q < 0 || c.num_head <= 0 || !(c.softmax_scale > 0.f) || !(c.softmax_scale < __builtin_inff()))
    return refuse(HPC_ERR_INVALID);
  if (c.num_head > 65535 || c.num_batch > 65535 || c.q_row_stride > kMlaPrefillMaxRowStride || c.k_row_stride > kMlaPrefillMaxRowStride ||
      c.v_row_stride > kMlaPrefillMaxRowStride || c.k_pe_row_stride > kMlaPrefillMaxRowStride)
    return refuse(HPC_ERR_UNSUPPORTED);
  if (c.num_batch == 0 || c.max_seqlens_q == 0) return r.empty = 1, r;
  r.grid_x = (c.max_seqlens_q + kMlaPrefillRowTile - 1) / kMlaPrefillRowTile;
  r.grid_y = c.num_head;
  r.grid_z = c.num_batch;
  r.threads = kMlaPrefillThreads;
  return r;
}

// merge_attn_states (merge_attn_states.hip): one lane group of D / 8 lanes per (row, head), kMergeThreads lanes a workgroup.
constexpr int kMergeThreads = 256;
constexpr int kMergeMaxDim = 512;

struct MergeRoute {
  int code, empty;
  int lanes_per_row;  // D / 8: each lane moves 16 bytes of a and of b
  int rows_per_wg;    // kMergeThreads / lanes_per_row (a lane group never straddles a workgroup; spare lanes idle)
  int64_t grid;
};

// out / out_a / out_b bf16 [T, H, D] with row and head strides (elements), lse arrays fp32 [T, H] contiguous.  HPC_ERR_INVALID:
// null pointers, negative counts; HPC_ERR_UNSUPPORTED: D % 8, D > 512 or D <= 0, misaligned bases or strides, strides under D,
// more than 2^31 - 1 (row, head) pairs.  T == 0 or H == 0 launches nothing.
static inline MergeRoute merge_route(uintptr_t out, uintptr_t lse, uintptr_t out_a, uintptr_t lse_a, uintptr_t out_b, uintptr_t lse_b,
                                     int64_t num_rows, int num_head, int dim, const int64_t (&strides)[6]) {
  MergeRoute r{};
  auto refuse = [&r](int code) { return r.code = code, r; };
  if (!out || !lse || !out_a || !lse_a || !out_b || !lse_b) return refuse(HPC_ERR_INVALID);
  if (num_rows < 0 || num_head < 0) return refuse(HPC_ERR_INVALID);
  if (dim <= 0 || (dim & 7) || dim > kMergeMaxDim) return refuse(HPC_ERR_UNSUPPORTED);
  if (((out | out_a | out_b) & 15) || ((lse | lse_a | lse_b) & 3)) return refuse(HPC_ERR_UNSUPPORTED);
  for (int64_t s : strides)
    if ((s & 7) || s < dim) return refuse(HPC_ERR_UNSUPPORTED);
  if (num_rows * num_head > 0x7fffffffll) return refuse(HPC_ERR_UNSUPPORTED);
  if (num_rows == 0 || num_head == 0) return r.empty = 1, r;
  r.lanes_per_row = dim / 8;
  r.rows_per_wg = kMergeThreads / r.lanes_per_row;
  r.grid = (num_rows * num_head + r.rows_per_wg - 1) / r.rows_per_wg;
  return r;
}

}  // namespace hpc
