// Dense FP8 linear with 128-block scales (gemm_blockwise_fp8.hip): which tile a workgroup owns, on which grid, with how many K
// splits, and what scratch goes with it - lgemm_route() is the one statement of it.  Internal header, host only, no HIP calls:
// a pure function of the call's shapes, the split count asked for and the CU count.  hpc_gemm_blockwise_fp8_plan (what the torch
// op sizes its scratch from) and the launcher hpc_gemm_blockwise_fp8_async both read it.
#pragma once
#include <stdint.h>

#include "hpc_common.h"

namespace hpc {

constexpr int kLgemmMaxM = 256;      // decode batches and speculative steps; prefill-sized calls belong to the grouped GEMM
constexpr int kLgemmTileN = 64;      // weight rows per workgroup: four waves x 16 rows
constexpr int kLgemmTileM = 64;      // tokens per workgroup at most: four 16-token MFMA column blocks
constexpr int kLgemmMaxSplits = 16;  // the last arriver sums at most 16 partial planes
constexpr int kLgemmMinBlocks = 4;   // k-blocks every split keeps when the library chooses the count

struct LgemmRoute {
  int code;        // HPC_OK or the refusal; the rest is set either way (zeros where it has no meaning)
  int mt;          // 16-token blocks per workgroup: 1 / 2 / 4 for m <= 16 / <= 32 / above
  int m_tiles;     // ceil(m / 64): token tiles are workgroups of their own (grid), each streams the weights again
  int n_tiles;     // n / 64
  int splits;      // the caller's count, or with splits_wanted == 0 what the library picks
  int max_splits;  // what a caller may ask for at most: min(16, k / 128) - every split keeps one k-block
  int grid;        // workgroups, one dimension: id = (m_tile * n_tiles + n_tile) * splits + split, so a tile's slices are
                   // neighbours in block id (dispatched together, they arrive together)
  int counters;    // zero-once int32 arrival counters, one per (m_tile, n_tile): m_tiles * n_tiles; 0 without a split
  int64_t workspace_bytes;  // fp32 partial planes [splits, m, n]; 0 without a split
};

// splits_wanted 0: as many splits as bring tiles x splits up to the CU count (between one and two workgroups per CU when the
// tiles alone are fewer than the CUs), never more than 16, never leaving a split fewer than 4 k-blocks.  cu_count <= 0: 256.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline LgemmRoute lgemm_route(int m, int n, int k, int splits_wanted, int cu_count) {
  LgemmRoute r{};
  r.splits = 1;
  if (m < 0 || n <= 0 || k <= 0 || splits_wanted < 0) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  // 128-wide k-blocks, 64-row tiles, decode-sized m, 32-bit buffer offsets into the weights and the activations
  if ((k & 127) || (n & (kLgemmTileN - 1)) || m > kLgemmMaxM || static_cast<int64_t>(n) * k > 0xfffffff0ll ||
      static_cast<int64_t>(m) * k > 0xfffffff0ll) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  const int kb = k >> 7;
  r.max_splits = kb < kLgemmMaxSplits ? kb : kLgemmMaxSplits;
  if (splits_wanted > r.max_splits) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  if (m == 0) return r;  // nothing to launch
  const int cus = cu_count > 0 ? cu_count : 256;
  r.mt = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
  r.m_tiles = (m + kLgemmTileM - 1) / kLgemmTileM;
  r.n_tiles = n / kLgemmTileN;
  const int64_t tiles = static_cast<int64_t>(r.m_tiles) * r.n_tiles;
  if (splits_wanted > 0) {
    r.splits = splits_wanted;
  } else {
    int64_t s = (cus + tiles - 1) / tiles;
    const int by_blocks = kb / kLgemmMinBlocks;
    if (s > by_blocks) s = by_blocks;
    if (s > kLgemmMaxSplits) s = kLgemmMaxSplits;
    r.splits = s < 1 ? 1 : static_cast<int>(s);
  }
  if (tiles * r.splits > 0x7fffffffll) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  r.grid = static_cast<int>(tiles * r.splits);
  if (r.splits > 1) {
    r.counters = static_cast<int>(tiles);
    r.workspace_bytes = static_cast<int64_t>(r.splits) * m * n * 4;
    if (r.workspace_bytes > 0xfffffff0ll) r.code = HPC_ERR_UNSUPPORTED;  // the planes are read through one 32-bit buffer
  }
  return r;
}

}  // namespace hpc
