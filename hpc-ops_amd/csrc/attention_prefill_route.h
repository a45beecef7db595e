// Prefill attention (attention_prefill.hip: FP8 on the paged cache, dense and block-sparse; attention_prefill_bf16.hip: bf16 on the
// paged cache and on contiguous K / V): which kernel form a call runs, with which shifts and on which grid, or why it is refused -
// prefill_route() is the one statement of it.  Internal header, host only, no HIP calls: a pure function of the call's
// shapes and - in the development build - of keys kDevPrefillRowMap (7) and kDevPrefillBf16Perm (46), read here and nowhere else.
#pragma once
#include <stdint.h>

#include "hpc_common.h"
#include "hpc_dev.h"

namespace hpc {

constexpr int kPrefillRowTile = 128;   // (position, q head) rows per workgroup: four waves x 32 rows
constexpr int kPrefillThreads = 256;
constexpr int kPrefillMaskCols = 512;  // block-sparse: mask columns (128-token tiles) a workgroup caches per q head (64k tokens)
constexpr float kPrefillScaleLog2 = 1.4426950408889634f / 11.313708498984761f;  // log2(e) / sqrt(128)

// the four C entries: ..._with_kvcache_prefill_fp8, ..._with_kvcache_blocksparse_prefill_fp8, ..._with_kvcache_prefill_bf16 and
// ..._prefill_bf16 (contiguous K / V, no pages: block_size and the block strides are 0)
enum PrefillEntry : int { kPrefillFp8 = 0, kPrefillFp8Sparse = 1, kPrefillBf16Paged = 2, kPrefillBf16 = 3 };

struct PrefillCall {  // what the call is; K / V strides in ELEMENTS (fp8: = bytes)
  int entry;       // PrefillEntry
  int quant_type;  // fp8: 1 = q per token and head, K / V per tensor; 0 = K per token (page tail rows), V per head
  bool has_mask;   // block-sparse entry: a mask was given (none = dense)
  int mask_tiles_m, mask_tiles_kv;
  int num_batch, max_seqlens_q;
  int num_dim_qk, num_dim_v, num_head_q, num_head_kv;
  int block_size;
  int ldQ, ldY;
  int64_t k_block_stride, k_token_stride, k_head_stride;
  int64_t v_block_stride, v_token_stride, v_head_stride;
};

struct PrefillRoute {  // what runs
  int code;                 // HPC_OK or the refusal; nothing below is set on a refusal
  int empty;                // no request or no q token: HPC_OK with nothing launched (and nothing below set)
  int g_shift, page_shift;  // log2 of the q heads per kv head and of the page size (contiguous K / V: 6, never used for a lookup)
  int quant, sparse;        // fp8: the kernel's kQuant and kSparse
  int by_head;              // fp8 row map: every 16-row block is one q head (else 128 / group positions x all heads, head fastest)
  int v_perm;               // bf16, development key kDevPrefillBf16Perm = 1: V^T operands built with v_perm_b32 (rounds 3-4)
  int grid_x, grid_y, grid_z, threads;  // (q row tiles of the longest request, kv heads, requests)
};

// The block-sparse entry refuses a page that does not divide a 128-token mask tile before it looks at anything else, its operands
// included: the entry asks this first, the route states it first.
static inline bool prefill_mask_page_ok(int block_size) { return block_size > 0 && 128 % block_size == 0; }

// Refusals come in the order the entries always had (the table of DESIGN 3.9) - it is observable, a call with two faults gets the
// code of the earlier one, and fp8 and paged bf16 differ in it: bf16 asks for the stride limits BEFORE the head counts.
// Alignment (16-byte vector accesses) is NOT symmetric for fp8: ldQ and the K strides to 16 elements, ldY and the V strides to 8
// (8 bf16 of y are 16 bytes; the V strides of an fp8 cache get the same 8: recorded as it always was, not to be changed in passing).
// Stride limits: the kernels form page offsets as unsigned 32 x 32 -> 64 products of what their Args hold.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline PrefillRoute prefill_route(const PrefillCall& c) {
  PrefillRoute r{};
  auto refuse = [&r](int code) { return r.code = code, r; };
  const bool fp8 = c.entry == kPrefillFp8 || c.entry == kPrefillFp8Sparse, paged = c.entry != kPrefillBf16;
  const bool sparse = c.entry == kPrefillFp8Sparse && c.has_mask;
  const auto strides_below = [&c](int64_t lim) {
    return c.k_block_stride > 0 && c.v_block_stride > 0 && c.k_token_stride > 0 && c.v_token_stride > 0 && c.k_block_stride < lim &&
           c.v_block_stride < lim && c.k_token_stride * c.block_size < lim && c.v_token_stride * c.block_size < lim;
  };
  if (c.entry == kPrefillFp8Sparse && !prefill_mask_page_ok(c.block_size)) return refuse(HPC_ERR_UNSUPPORTED);
  if (fp8 && c.quant_type != 0 && c.quant_type != 1) return refuse(HPC_ERR_INVALID);
  if (c.num_batch < 0 || c.max_seqlens_q < 0) return refuse(HPC_ERR_INVALID);
  if (c.num_batch == 0 || c.max_seqlens_q == 0) return r.empty = 1, r;
  if (c.num_dim_qk != 128 || c.num_dim_v != 128) return refuse(HPC_ERR_UNSUPPORTED);
  if (paged && c.block_size != 16 && c.block_size != 32 && c.block_size != 64) return refuse(HPC_ERR_UNSUPPORTED);
  if (fp8 && c.quant_type == 0 && c.block_size < 32) return refuse(HPC_ERR_UNSUPPORTED);  // scale rows hold 32 tokens
  if (c.entry == kPrefillBf16Paged && !strides_below(1ll << 31)) return refuse(HPC_ERR_UNSUPPORTED);
  if (c.num_head_kv <= 0 || c.num_head_q % c.num_head_kv) return refuse(HPC_ERR_INVALID);
  const int group = c.num_head_q / c.num_head_kv;
  // powers of two up to 16: q rows are addressed by shift and mask
  if (group != 1 && group != 2 && group != 4 && group != 8 && group != 16) return refuse(HPC_ERR_UNSUPPORTED);
  if (((c.ldQ | c.k_token_stride | c.k_head_stride | c.k_block_stride) & (fp8 ? 15 : 7)) ||
      ((c.ldY | c.v_token_stride | c.v_head_stride | c.v_block_stride) & 7))
    return refuse(HPC_ERR_UNSUPPORTED);
  if (sparse && (c.mask_tiles_m <= 0 || c.mask_tiles_kv <= 0)) return refuse(HPC_ERR_INVALID);
  if (sparse && c.mask_tiles_kv > kPrefillMaskCols) return refuse(HPC_ERR_UNSUPPORTED);
  if (fp8 && !strides_below(1ll << 32)) return refuse(HPC_ERR_UNSUPPORTED);
  if (c.num_head_kv > 65535 || c.num_batch > 65535) return refuse(HPC_ERR_UNSUPPORTED);  // grid.y, grid.z

  r.g_shift = __builtin_ctz(static_cast<unsigned>(group));
  r.page_shift = paged ? __builtin_ctz(static_cast<unsigned>(c.block_size)) : 6;
  r.quant = fp8 ? c.quant_type : 0;
  r.sparse = sparse;
  // head-major 16-row blocks let a block skip masked-out tiles (block-sparse); dense attention measured ~8 % faster with every
  // wave holding all heads of a few positions.  Development key kDevPrefillRowMap overrides: 1 = by head, 2 = by position.
  // Group 16 has no head-major form (8 positions x 16 heads per block).
  const int row_map = hpc_dev_tuning_get(kDevPrefillRowMap);
  r.by_head = fp8 && group <= 8 && (row_map ? row_map == 1 : sparse);
  r.v_perm = !fp8 && hpc_dev_tuning_get(kDevPrefillBf16Perm) == 1;
  r.grid_x = static_cast<int>((static_cast<int64_t>(c.max_seqlens_q) * group + kPrefillRowTile - 1) / kPrefillRowTile);
  r.grid_y = c.num_head_kv;
  r.grid_z = c.num_batch;
  r.threads = kPrefillThreads;
  return r;
}

}  // namespace hpc
