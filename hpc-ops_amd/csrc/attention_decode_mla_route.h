// MLA decode attention over the paged latent cache (attention_decode_mla.hip): which rows a workgroup owns, on which grid, in
// how many pieces a request's tokens are cut, and what scratch goes with it - mla_route() is the one statement of it.  Internal
// header, host only, no HIP calls: a pure function of the call's shapes, the split count asked for and the CU count.
// hpc_attention_decode_mla_plan (what the torch op sizes its scratch from) and the launcher hpc_attention_decode_mla_bf16_async
// both read it.  Nothing here depends on the lengths of the requests: they stay on the device.
#pragma once
#include <stdint.h>

#include "hpc_common.h"
#include "mla_cache.h"

namespace hpc {

// the row's dimensions are mla_cache.h's: kMlaRow columns are K, the first kMlaLatent of them are also V
constexpr int kMlaRowTile = 64;     // q rows (r = s * num_head + h) per workgroup: four waves x 16 rows
constexpr int kMlaKvTile = 64;      // tokens per LDS image; piece lengths are multiples of it
constexpr int kMlaMaxSplits = 64;   // pieces the merge sums at most
constexpr int kMlaMaxSeqQ = 4;      // mtp 0 .. 3

struct MlaRoute {
  int code;        // HPC_OK or the refusal; the rest is set either way (zeros where it has no meaning)
  int rows;        // q rows per request: num_seq_q * num_head, a multiple of 16
  int narrow;      // 1 when a request has one 16-row block (num_head 16 at mtp 0): the four waves of the workgroup split each
                   // KV tile's tokens instead of the rows and merge at the end
  int row_tiles;   // ceil(rows / 64)
  int splits;      // the caller's count, or with splits_wanted == 0 what the library picks
  int max_splits;  // what a caller may ask for at most
  int grid;        // workgroups, one dimension: id = (batch * row_tiles + row_tile) * splits + piece
  int merge_grid;  // workgroups of the merge kernel: num_batch * rows (one per output row); 0 without a split
  int64_t ml_offset;        // byte offset of the (max, sum) pairs [splits, num_batch * rows, 2] fp32 behind the fp32 partial
                            // outputs [splits, num_batch * rows, 512]
  int64_t workspace_bytes;  // both arrays; 0 without a split.  Never zeroed, never read where a piece did not write
};

// splits_wanted 0, the starting rule (unmeasured when it was written; profiles/mla_decode.txt shows where it over- or
// under-splits): with W = num_batch * row_tiles workgroups before any split, one piece when W >= the CU count, otherwise
// min(max_splits, ceil(2 * CUs / W)).  cu_count <= 0: 256.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline MlaRoute mla_route(int num_batch, int num_seq_q, int num_head, int splits_wanted, int cu_count) {
  MlaRoute r{};
  r.splits = 1;
  r.max_splits = kMlaMaxSplits;
  if (num_batch < 0 || num_seq_q <= 0 || num_head <= 0 || splits_wanted < 0) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  if ((num_head & 15) || num_head > 128 || num_seq_q > kMlaMaxSeqQ) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  if (splits_wanted > r.max_splits) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  r.rows = num_seq_q * num_head;
  r.narrow = r.rows == 16;
  r.row_tiles = (r.rows + kMlaRowTile - 1) / kMlaRowTile;
  if (num_batch == 0) return r;  // nothing to launch
  const int cus = cu_count > 0 ? cu_count : 256;
  const int64_t w = static_cast<int64_t>(num_batch) * r.row_tiles;
  if (splits_wanted > 0) {
    r.splits = splits_wanted;
  } else if (w < cus) {
    const int64_t s = (2ll * cus + w - 1) / w;
    r.splits = static_cast<int>(s < r.max_splits ? s : r.max_splits);
  }
  const int64_t total_rows = static_cast<int64_t>(num_batch) * r.rows;
  if (w * r.splits > 0x7fffffffll || total_rows > 0x7fffffffll) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  r.grid = static_cast<int>(w * r.splits);
  if (r.splits > 1) {
    r.merge_grid = static_cast<int>(total_rows);
    r.ml_offset = static_cast<int64_t>(r.splits) * total_rows * kMlaLatent * 4;
    r.workspace_bytes = r.ml_offset + static_cast<int64_t>(r.splits) * total_rows * 2 * 4;
  }
  return r;
}

}  // namespace hpc
