// The paged latent KV cache of the MLA ops, stated once: the row's dimensions, the two forms of a cache cell and the host rule
// for a cache a launcher accepts.  Internal header, plain C++17, no HIP header: the launchers of mla_store.hip,
// attention_decode_mla.hip and mla_gather.hip and the torch shim (torch_mla.cpp) all read it.
// A cache is [num_blocks, block_size, row]: token t of page p at base + p * block_stride + t * token_stride, the row contiguous.
//   bf16   576 bf16 per token (the 512 latent columns, then the 64 RoPE columns); strides in ELEMENTS
//   FP8    the 656-byte row of mla_fp8_format.h; strides in BYTES
// Either way every 16-byte access of a row is aligned: both strides and the base are multiples of 16 bytes.
#pragma once
#include <stdint.h>

#include "hpc_status.h"
#include "mla_fp8_format.h"

namespace hpc {

constexpr int kMlaLatent = 512;                 // the normalised compressed KV: K and V of every head
constexpr int kMlaRope = 64;                    // the RoPE'd k_pe: K only
constexpr int kMlaRow = kMlaLatent + kMlaRope;  // 576: one token, and one absorbed q row
static_assert(kMlaLatent == 4 * kMlaFp8Group && kMlaFp8ScalesAt == kMlaLatent && kMlaFp8RopeAt + 2 * kMlaRope == kMlaFp8RowBytes,
              "the FP8 row holds the same columns");

struct MlaCacheKind {
  bool fp8;
  int unit;          // bytes in one unit of the cache's two strides
  int row;           // units a token takes: the least token stride
  int align;         // units both strides are multiples of: 16 bytes
  const char* rule;  // the stride rule in words
};
constexpr MlaCacheKind kMlaCacheBf16{false, 2, kMlaRow, 8,
                                     "ckv_cache token stride must be >= 576 and, like the block stride, a multiple of 8 elements"};
constexpr MlaCacheKind kMlaCacheFp8{true, 1, kMlaFp8RowBytes, kMlaFp8Align,
                                    "ckv_cache token stride must be >= 656 and, like the block stride, a multiple of 16 bytes"};

// log2 of a page size in {16, 32, 64, 128}: 4 .. 7; -1 for anything else
constexpr int mla_page_shift(int64_t block_size) {
  for (int s = 4; s <= 7; ++s)
    if (block_size == (int64_t{1} << s)) return s;
  return -1;
}

struct MlaCacheCheck {
  int code;         // HPC_OK or the refusal
  const char* why;  // the refusal in words (null when accepted)
};

// The one host check of a cache, for a call with or without work.  Refusals in this order: a negative block stride is
// HPC_ERR_INVALID and wins over everything behind it, which is HPC_ERR_UNSUPPORTED - the page size, a token stride below the row
// (a negative one included), a stride off the 16-byte grid, a misaligned base.  `base` is never dereferenced; null passes
// (whether a cache may be absent is the launcher's rule).  (static: product and development library may sit in one process)
static inline MlaCacheCheck mla_cache_check(const MlaCacheKind& kind, uintptr_t base, int64_t block_size, int64_t block_stride,
                                            int64_t token_stride) {
  if (block_stride < 0) return {HPC_ERR_INVALID, "ckv_cache block stride must not be negative"};
  if (mla_page_shift(block_size) < 0) return {HPC_ERR_UNSUPPORTED, "block_size must be 16, 32, 64 or 128"};
  if (token_stride < kind.row || token_stride % kind.align || block_stride % kind.align) return {HPC_ERR_UNSUPPORTED, kind.rule};
  if (base % 16) return {HPC_ERR_UNSUPPORTED, "ckv_cache must be 16-byte aligned"};
  return {HPC_OK, nullptr};
}

}  // namespace hpc
