// Token-sparse MLA decode attention over the paged latent cache (the kSparse form of attention_decode_mla.hip): which rows a
// workgroup owns, on which grid, in how many pieces a q row's list is cut, and what scratch goes with it - mla_sparse_route() is
// the one statement of it.  Internal header, host only, no HIP calls: a pure function of the call's shapes, the list length, the
// split count asked for and the CU count.  hpc_attention_decode_mla_sparse_plan (what the torch op sizes its scratch from) and the
// launchers hpc_attention_decode_mla_sparse_{bf16,fp8}_async read it.  Unlike the dense route the piece length is a host value,
// because topk is: nothing here or on the device depends on the lengths of the requests for it.
#pragma once
#include <stdint.h>

#include "attention_decode_mla_route.h"

namespace hpc {

constexpr int kMlaSparseMaxTopk = 65536;  // list entries per q row at most

struct MlaSparseRoute {
  int code;        // HPC_OK or the refusal; the rest is set either way (zeros where it has no meaning)
  int rows;        // rows a workgroup's tile is cut from: the num_head heads of ONE q row (b, s) - lists differ per s
  int narrow;      // 1 when num_head == 16: the four waves split each tile's slots instead of the heads and merge at the end
  int head_tiles;  // ceil(num_head / 64)
  int splits;      // the EFFECTIVE piece count: pieces that would start at or past topk are not launched
  int max_splits;  // what a caller may ask for at most
  int plen;        // list slots per piece: ceil(topk / splits asked or picked) rounded up to 64
  int grid;        // workgroups, one dimension: id = ((b * num_seq_q + s) * head_tiles + head_tile) * splits + piece
  int merge_grid;  // workgroups of the merge kernel: num_batch * num_seq_q * num_head (one per output row); 0 without a split
  int64_t ml_offset;        // byte offset of the (max, sum) pairs [splits, total rows, 2] fp32 behind the fp32 partial outputs
                            // [splits, total rows, 512]
  int64_t workspace_bytes;  // both arrays; 0 without a split.  Never zeroed: every launched piece writes all of its rows
};

// splits_wanted 0, the dense starting rule (unmeasured when it was written; profiles/mla_decode_sparse.txt shows where it over- or
// under-splits): with W = num_batch * num_seq_q * head_tiles workgroups before any split, one piece when W >= the CU count,
// otherwise min(max_splits, ceil(2 * CUs / W)), and never more pieces than the list has tiles of 64.  cu_count <= 0: 256.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline MlaSparseRoute mla_sparse_route(int num_batch, int num_seq_q, int num_head, int topk, int splits_wanted,
                                              int cu_count) {
  MlaSparseRoute r{};
  r.splits = 1;
  r.max_splits = kMlaMaxSplits;
  if (num_batch < 0 || num_seq_q <= 0 || num_head <= 0 || splits_wanted < 0 || topk <= 0) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  if ((num_head & 15) || num_head > 128 || num_seq_q > kMlaMaxSeqQ || topk > kMlaSparseMaxTopk) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  if (splits_wanted > r.max_splits) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  r.rows = num_head;
  r.narrow = num_head == 16;
  r.head_tiles = (num_head + kMlaRowTile - 1) / kMlaRowTile;
  const int list_tiles = (topk + kMlaKvTile - 1) / kMlaKvTile;
  r.plen = list_tiles * kMlaKvTile;
  if (num_batch == 0) return r;  // nothing to launch
  const int cus = cu_count > 0 ? cu_count : 256;
  const int64_t w = static_cast<int64_t>(num_batch) * num_seq_q * r.head_tiles;
  int64_t cut = 1;
  if (splits_wanted > 0) {
    cut = splits_wanted;
  } else if (w < cus) {
    cut = (2ll * cus + w - 1) / w;
    cut = cut < r.max_splits ? cut : r.max_splits;
    cut = cut < list_tiles ? cut : list_tiles;
  }
  r.plen = static_cast<int>(((topk + cut - 1) / cut + kMlaKvTile - 1) / kMlaKvTile) * kMlaKvTile;
  r.splits = (topk + r.plen - 1) / r.plen;  // <= cut
  const int64_t total_rows = w / r.head_tiles * num_head;
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
