// MLA decode attention over the paged latent cache (attention_decode_mla.hip), dense and token-sparse: which rows a workgroup
// owns, on which grid, in how many pieces a request's tokens or a q row's list are cut, and what scratch goes with it -
// mla_route() is the one statement of it.  Internal header, host only, no HIP calls: a pure function of the call's shapes, the
// form, the list length, the split count asked for and the CU count.  hpc_attention_decode_mla_plan and
// hpc_attention_decode_mla_sparse_plan (what the torch ops size their scratch from) and the four launchers
// hpc_attention_decode_mla{,_sparse}_{bf16,fp8}_async all read it.  Nothing here depends on the lengths of the requests: they
// stay on the device.  The sparse form's piece length is a host value, because topk is.
#pragma once
#include <stdint.h>

#include "hpc_status.h"
#include "mla_cache.h"

namespace hpc {

// the row's dimensions are mla_cache.h's: kMlaRow columns are K, the first kMlaLatent of them are also V
constexpr int kMlaRowTile = 64;     // q rows per workgroup: four waves x 16 rows
constexpr int kMlaKvTile = 64;      // tokens (list slots) per LDS image; piece lengths are multiples of it
constexpr int kMlaMaxSplits = 64;   // pieces the merge sums at most
constexpr int kMlaMaxSeqQ = 4;      // mtp 0 .. 3
constexpr int kMlaSparseMaxTopk = 65536;  // list entries per q row at most

// A unit is what a workgroup's row tile is cut from.  dense: a request, its rows r = s * num_head + h.  sparse: ONE q row
// (b, s), its rows the heads h - lists differ per s.
struct MlaRoute {
  int code;        // HPC_OK or the refusal; the rest is set either way (zeros where it has no meaning)
  int rows;        // rows per unit, a multiple of 16: num_seq_q * num_head (dense), num_head (sparse)
  int narrow;      // 1 when a unit has one 16-row block (16 heads; dense: at mtp 0 only): the four waves of the workgroup
                   // split each KV tile's tokens (slots) instead of the rows and merge at the end
  int row_tiles;   // ceil(rows / 64)
  int splits;      // the caller's count, or with splits_wanted == 0 what the library picks.  sparse: the EFFECTIVE piece
                   // count - pieces that would start at or past topk are not launched
  int max_splits;  // what a caller may ask for at most
  int plen;        // sparse: list slots per piece, ceil(topk / splits asked or picked) rounded up to 64.  dense: 0 (the piece
                   // length is the device's, from the request's length)
  int grid;        // workgroups, one dimension: id = (unit * row_tiles + row_tile) * splits + piece
  int merge_grid;  // workgroups of the merge kernel: total_rows (one per output row); 0 without a split
  int64_t total_rows;       // units * rows = num_batch * num_seq_q * num_head
  int64_t ml_offset;        // byte offset of the (max, sum) pairs [splits, total_rows, 2] fp32 behind the fp32 partial
                            // outputs [splits, total_rows, 512]
  int64_t workspace_bytes;  // both arrays; 0 without a split.  Never zeroed, never read where a piece did not write (sparse:
                            // every launched piece writes all of its rows)
};

// splits_wanted 0, the starting rule (unmeasured when it was written; profiles/mla_decode.txt and
// profiles/mla_decode_sparse.txt show where it over- or under-splits): with W = units * row_tiles workgroups before any split,
// one piece when W >= the CU count, otherwise min(max_splits, ceil(2 * CUs / W)) - and, sparse, never more pieces than the
// list has tiles of 64.  cu_count <= 0: 256.  `topk` is read only with `sparse`.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline MlaRoute mla_route(int num_batch, int num_seq_q, int num_head, bool sparse, int topk, int splits_wanted,
                                 int cu_count) {
  MlaRoute r{};
  r.splits = 1;
  r.max_splits = kMlaMaxSplits;
  if (num_batch < 0 || num_seq_q <= 0 || num_head <= 0 || splits_wanted < 0 || (sparse && topk <= 0)) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  if ((num_head & 15) || num_head > 128 || num_seq_q > kMlaMaxSeqQ || (sparse && topk > kMlaSparseMaxTopk)) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  if (splits_wanted > r.max_splits) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  const int64_t units = sparse ? static_cast<int64_t>(num_batch) * num_seq_q : num_batch;
  r.rows = sparse ? num_head : num_seq_q * num_head;
  r.narrow = r.rows == 16;
  r.row_tiles = (r.rows + kMlaRowTile - 1) / kMlaRowTile;
  const int list_tiles = sparse ? (topk + kMlaKvTile - 1) / kMlaKvTile : 0;
  r.plen = list_tiles * kMlaKvTile;
  if (num_batch == 0) return r;  // nothing to launch
  const int cus = cu_count > 0 ? cu_count : 256;
  const int64_t w = units * r.row_tiles;
  int64_t cut = 1;
  if (splits_wanted > 0) {
    cut = splits_wanted;
  } else if (w < cus) {
    cut = (2ll * cus + w - 1) / w;
    cut = cut < r.max_splits ? cut : r.max_splits;
    if (sparse) cut = cut < list_tiles ? cut : list_tiles;
  }
  r.splits = static_cast<int>(cut);
  if (sparse) {
    r.plen = static_cast<int>(((topk + cut - 1) / cut + kMlaKvTile - 1) / kMlaKvTile) * kMlaKvTile;
    r.splits = (topk + r.plen - 1) / r.plen;  // <= cut
  }
  r.total_rows = units * r.rows;
  if (w * r.splits > 0x7fffffffll || r.total_rows > 0x7fffffffll) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  r.grid = static_cast<int>(w * r.splits);
  if (r.splits > 1) {
    r.merge_grid = static_cast<int>(r.total_rows);
    r.ml_offset = static_cast<int64_t>(r.splits) * r.total_rows * kMlaLatent * 4;
    r.workspace_bytes = r.ml_offset + static_cast<int64_t>(r.splits) * r.total_rows * 2 * 4;
  }
  return r;
}

}  // namespace hpc
