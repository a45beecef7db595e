// The DSA lightning indexer, stated once.  In this order:
//   the cache    the paged index-key cache and the host rule for a cache a launcher accepts (mla_indexer_cache_check);
//   the rows     MlaRows, where the rows of a reader's call come from - a decode step (num_seq_kvcache, mtp, new_kv_included) or
//                a ragged prefill chunk (num_seqlen_per_req, q_index, row_begin) - with the refusals, the row count and the
//                "is there work" of either.  The logits / top-k launchers and the token-sparse MLA attention
//                (attention_decode_mla.hip) all take it;
//   the routes   mla_indexer_route() of a decode step (mla_indexer.hip: grid, chunking of the context, scratch of the fused
//                call) and mla_indexer_prefill_route() of a chunk (mla_indexer_prefill.hip: row tile, chunk, grid, slab,
//                scratch).  What both refuse of a shape is mla_indexer_shape(), how both cut the columns mla_indexer_chunk();
//   the checks   mla_indexer_logits_check, _topk_check and _fused_check: every refusal of the six reader entries with its reason
//                in words, one function per op for both forms, given the rows and the form's route;
//   the front end  the one host rule of mla_indexer_prep.hip, at the end.
// Internal header, plain C++17, no HIP header: the launchers of mla_indexer.hip, mla_indexer_prefill.hip and
// mla_indexer_prep.hip, the plan entries and the torch shim (torch_mla_indexer.cpp) all read it.
//
// The index-key cache.  Every token of every request has ONE index key of 128 columns, shared by all index heads: 128
// float8_e4m3fn codes and one float32 scale, column d = fp32(code[d]) * scale, for any finite non-negative scale.  The cache is
// a uint8 tensor, logically [num_blocks, P * 132], addressed through the block_ids page table of the latent cache.  Within a page
// the codes of its P tokens come first, [P, 128] at byte 0 (token t at byte 128 t), and the P float32 scales follow at byte
// 128 P (token t at byte 128 P + 4 t): every 16-byte access of a key is aligned without padding a row to 144 bytes.
// P in {16, 32, 64, 128}; block stride >= 132 P bytes and a multiple of 16; base 16-byte aligned.
#pragma once
#include <stdint.h>

#include "byte_span.h"
#include "hpc_status.h"
#include "mla_cache.h"

namespace hpc {

constexpr int kIdxDim = 128;                      // columns of an index key, and of a q head
constexpr int kIdxTokenBytes = kIdxDim + 4;       // 132: codes + scale, what a token costs a page
constexpr int kIdxMaxTopk = 65536;                // list entries per q row at most, as the sparse attention takes
constexpr int kIdxMaxSeqQ = 4;                    // mtp + 1 at most
constexpr int kIdxTile = 64;                      // tokens a wave takes per step: four 16 x 16 blocks
constexpr int kIdxWaves = 4;                      // waves of a logits workgroup
constexpr int kIdxMinChunk = kIdxTile * kIdxWaves * 2;  // 512 tokens: the shortest piece of a context a workgroup owns
constexpr int kIdxMaxChunk = 8192;
constexpr int64_t kIdxMaxCols = int64_t{1} << 30;  // max_blocks * P at most, as the MLA decode ops

constexpr int64_t mla_indexer_scales_at(int64_t block_size) { return block_size * kIdxDim; }
constexpr int64_t mla_indexer_page_bytes(int64_t block_size) { return block_size * kIdxTokenBytes; }

struct MlaIndexerCheck {
  int code;         // HPC_OK or the refusal
  const char* why;  // the refusal in words (null when accepted)
};

// The one host check of an index-key cache, for a call with or without work.  `base` is never dereferenced; null passes
// (whether a cache may be absent is the launcher's rule).  (static: product and development library may sit in one process)
static inline MlaIndexerCheck mla_indexer_cache_check(uintptr_t base, int64_t block_size, int64_t block_stride) {
  if (block_stride < 0) return {HPC_ERR_INVALID, "k_cache block stride must not be negative"};
  if (mla_page_shift(block_size) < 0) return {HPC_ERR_UNSUPPORTED, "block_size must be 16, 32, 64 or 128"};
  if (block_stride < mla_indexer_page_bytes(block_size))
    return {HPC_ERR_UNSUPPORTED, "k_cache block stride must be at least block_size * 132 bytes"};
  if (block_stride % 16) return {HPC_ERR_UNSUPPORTED, "k_cache block stride must be a multiple of 16 bytes"};
  if (base % 16) return {HPC_ERR_UNSUPPORTED, "k_cache must be 16-byte aligned"};
  return {HPC_OK, nullptr};
}

// The scratch of the fused call (logits then top-k): one float32 row per q row, rows of row_stride floats.  Sizer
// (hpc_mla_indexer_plan), launcher (hpc_mla_indexer_topk_fp8_async) and shim all take it from here.
struct MlaIndexerScratch {
  int64_t row_stride;  // floats: the logits' columns (a multiple of 16 already: max_blocks * P)
  int64_t bytes;       // rows * row_stride * 4; never zeroed: the top-k reads only the columns the logits op wrote
};
static inline MlaIndexerScratch mla_indexer_scratch(int64_t rows, int64_t cols) { return {cols, rows * cols * 4}; }

// ---- the rows of a call ------------------------------------------------------------------------------------------------------
// A decode step: num_batch requests of num_seq_q rows each, row r is (b, s) = (r / num_seq_q, r % num_seq_q), lens is
// num_seq_kvcache [num_batch].  A ragged chunk: num_rows rows that the writers' row rule (mla_indexer_dev.h::locate_row) places
// in num_req requests, lens is num_seqlen_per_req [num_req], q_index [num_req + 1], and row r of the call is row row_begin + r of
// the chunk.  What a row sees is the device's (mla_indexer_dev.h: step_sees, row_sees).  The pointers are held as given and
// never dereferenced on the host.
struct MlaRows {
  bool ragged;
  const int* lens;
  const int* q_index;                         // a chunk's; null for a step
  int num_batch, num_seq_q, new_kv_included;  // a step's; a chunk holds (0, 1, 1): what the shared kernels are told
  int num_rows, num_req, row_begin;           // a chunk's; zeros for a step

  static MlaRows step(const int* lens, int num_batch, int num_seq_q, int new_kv_included) {
    return {false, lens, nullptr, num_batch, num_seq_q, new_kv_included, 0, 0, 0};
  }
  static MlaRows chunk(const int* lens, const int* q_index, int num_rows, int num_req, int row_begin) {
    return {true, lens, q_index, 0, 1, 1, num_rows, num_req, row_begin};
  }
  int64_t rows() const { return ragged ? num_rows : static_cast<int64_t>(num_batch) * num_seq_q; }
  bool work() const { return ragged ? num_rows > 0 && num_req > 0 : num_batch > 0; }  // without it nothing is launched
  bool tables() const { return lens && (!ragged || q_index); }                        // what a call with work reads
  // the refusals: the counts that make no sense, then what the kernels' int32 arithmetic does not hold.  pad: the rows past
  // its last that a chunk's logits call counts (its row tile)
  MlaIndexerCheck negative() const {
    if (ragged && (num_rows < 0 || num_req < 0 || row_begin < 0))
      return {HPC_ERR_INVALID, "num_rows, num_req and row_begin must not be negative"};
    if (!ragged && num_batch < 0) return {HPC_ERR_INVALID, "num_batch must not be negative"};
    if (!ragged && num_seq_q <= 0) return {HPC_ERR_INVALID, "num_seq_q must be positive"};
    return {HPC_OK, nullptr};
  }
  MlaIndexerCheck limits(int pad = 0) const {
    if (!ragged && num_seq_q > kIdxMaxSeqQ) return {HPC_ERR_UNSUPPORTED, "mtp must be 0 .. 3"};
    if (!ragged && rows() > INT32_MAX) return {HPC_ERR_UNSUPPORTED, "num_batch * num_seq_q beyond int32"};
    if (ragged && (static_cast<int64_t>(row_begin) + num_rows + pad > INT32_MAX || num_req == INT32_MAX))
      return {HPC_ERR_UNSUPPORTED, "row_begin + num_rows and num_req + 1 must fit int32"};
    return {HPC_OK, nullptr};
  }
};

// ---- what the two routes share -------------------------------------------------------------------------------------------------
// The shape refusals: head count, page size, list length (logits_only: not looked at) and columns; head_blocks and cols are set
// on the way
static inline MlaIndexerCheck mla_indexer_shape(int num_head, int block_size, int max_blocks, int topk, bool logits_only,
                                                int* head_blocks, int64_t* cols) {
  if (num_head != 16 && num_head != 32 && num_head != 64) return {HPC_ERR_UNSUPPORTED, "the index head count must be 16, 32 or 64"};
  if (mla_page_shift(block_size) < 0) return {HPC_ERR_UNSUPPORTED, "block_size must be 16, 32, 64 or 128"};
  if (!logits_only && (topk < 1 || topk > kIdxMaxTopk)) return {HPC_ERR_UNSUPPORTED, "topk must be 1 .. 65536"};
  *head_blocks = num_head / 16;
  *cols = static_cast<int64_t>(max_blocks) * block_size;
  if (*cols > kIdxMaxCols) return {HPC_ERR_UNSUPPORTED, "block_ids reaches beyond 2^30 tokens"};
  return {HPC_OK, nullptr};
}
// The chunk rule: the columns one logits workgroup owns are 512, doubled up to 8192 while `units` (requests of a step, row tiles
// of a chunk's launch) times the chunks of a row are beyond 16 workgroups per CU - a host value: nothing here or on the device
// depends on the lengths of the requests for it.  cu_count <= 0: 256.
static inline int mla_indexer_chunk(int64_t units, int64_t cols, int cu_count) {
  const int cus = cu_count > 0 ? cu_count : 256;
  int chunk = kIdxMinChunk;
  while (chunk < kIdxMaxChunk && units * ((cols + chunk - 1) / chunk) > 16ll * cus) chunk *= 2;
  return chunk;
}

struct MlaIndexerRoute {
  int code;          // HPC_OK or the refusal; the rest is set either way (zeros where it has no meaning)
  const char* why;   // the refusal in words (null when accepted)
  int head_blocks;   // num_head / 16: matrix instructions per 16 tokens and q row
  int64_t cols;      // max_blocks * block_size: the logits' columns
  int chunk;         // tokens of a request's context one logits workgroup owns (a multiple of 256)
  int chunks;        // ceil(cols / chunk)
  int grid;          // logits workgroups, one dimension: id = b * chunks + piece; a piece at or past the request's end leaves at once
  int topk_grid;     // top-k workgroups: one per q row
  MlaIndexerScratch scratch;  // of the fused call
};

// logits_only: the list length has no part in the call and topk is not looked at; otherwise 1 .. 65536.  The chunk is
// mla_indexer_chunk()'s with the requests as units.
static inline MlaIndexerRoute mla_indexer_route(int num_batch, int num_seq_q, int num_head, int block_size, int max_blocks,
                                                int topk, bool logits_only, int cu_count) {
  MlaIndexerRoute r{};
  const auto refuse = [&](int code, const char* why) {
    r.code = code;
    r.why = why;
    return r;
  };
  const MlaRows rows = MlaRows::step(nullptr, num_batch, num_seq_q, 1);
  MlaIndexerCheck c = rows.negative();
  if (c.code == HPC_OK && max_blocks < 0) c = {HPC_ERR_INVALID, "max_blocks must not be negative"};
  if (c.code == HPC_OK) c = rows.limits();
  if (c.code == HPC_OK) c = mla_indexer_shape(num_head, block_size, max_blocks, topk, logits_only, &r.head_blocks, &r.cols);
  if (c.code != HPC_OK) return refuse(c.code, c.why);
  r.topk_grid = static_cast<int>(rows.rows());
  r.scratch = mla_indexer_scratch(rows.rows(), r.cols);
  r.chunk = mla_indexer_chunk(num_batch, r.cols, cu_count);
  r.chunks = static_cast<int>((r.cols + r.chunk - 1) / r.chunk);
  const int64_t grid = static_cast<int64_t>(num_batch) * r.chunks;
  if (grid > 0x7fffffffll) return refuse(HPC_ERR_UNSUPPORTED, "the logits grid is beyond int32");
  r.grid = static_cast<int>(grid);
  return r;
}

// ---- a ragged prefill chunk (mla_indexer_prefill.hip: logits; mla_indexer.hip: top-k) -------------------------------------------
// The rows of a chunk follow the writers' row rule (mla_indexer_dev.h::locate_row), read on the device.  The logits kernel is
// key-stationary: a workgroup stages a tile of kIdxPrefillTile q rows (codes and weights) in LDS once and runs all of them
// against every 64-key step of its chunk of columns, so a key tile is loaded once per row tile.  Tiles are cut from the row
// index of the call, not per request, which makes the grid a host value: ceil(rows / tile) * chunks; the chunking of the columns
// is mla_indexer_chunk()'s with the row tiles of a launch as units.
// The fused call runs logits then top-k over slabs of rows through one float32 scratch [slab_rows, cols]; the slab is the
// caller's (scratch_rows > 0) or, with 0, what fits kIdxPrefillScratchBytes.  That budget is a resource cap, not a tuned number:
// 256 MiB holds the logits of a 2048-row slab over a 32k-token table, so that the scratch does not grow with the chunk while a
// slab still fills the device many times over; nothing was measured to pick it.
constexpr int kIdxPrefillTile = 16;  // q rows of a workgroup: 16 x Hi x 132 B of LDS, 132 KiB at Hi = 64 of the 160 KiB
constexpr int kIdxPrefillWaves = 8;  // waves of a workgroup, two per SIMD: each takes 64 of every 512 columns of the chunk
constexpr int64_t kIdxPrefillScratchBytes = int64_t{256} << 20;
constexpr int64_t kIdxPrefillMaxScratchBytes = int64_t{1} << 40;  // a caller's slab beyond 1 TiB of logits is refused (and the
                                                                  // product slab_rows * cols * 4 stays far inside int64)
constexpr int64_t mla_indexer_prefill_lds_bytes(int num_head) { return int64_t{kIdxPrefillTile} * num_head * kIdxTokenBytes; }

struct MlaIndexerPrefillRoute {
  int code;          // HPC_OK or the refusal; the rest is set either way (zeros where it has no meaning)
  const char* why;   // the refusal in words (null when accepted)
  int head_blocks;   // num_head / 16
  int64_t cols;      // max_blocks * block_size: the logits' columns
  int tile;          // q rows of a logits workgroup
  int tiles;         // ceil(num_rows / tile) of a logits call over all num_rows rows
  int chunk;         // columns one logits workgroup owns (a multiple of 512), chosen for a launch over a whole slab (logits op:
                     // over all rows).  The fused call launches the logits once per slab and each launch routes itself from
                     // its own rows and the device's CU count: a partial last slab may take a shorter chunk.  No logit
                     // depends on the chunk.
  int chunks;        // ceil(cols / chunk)
  int grid;          // workgroups of ONE logits launch over num_rows rows at that chunk: id = tile * chunks + piece; 0: nothing
                     // to launch.  The fused call's launches together have as many tiles, each slab's rounded up
  int topk_grid;     // top-k workgroups: one per row
  int slab_rows;     // rows of a slab of the fused call
  int slabs;         // ceil(num_rows / slab_rows): a host value
  MlaIndexerScratch scratch;  // of the fused call: [slab_rows, cols] float32, never zeroed
};

// logits_only: topk and scratch_rows are not looked at.  The chunk is chosen from rows_per_call, the rows one logits launch
// takes: num_rows for the logits op, a slab for the fused one.  cu_count <= 0: 256.
static inline MlaIndexerPrefillRoute mla_indexer_prefill_route(int num_rows, int num_req, int num_head, int block_size, int max_blocks,
                                                               int topk, bool logits_only, int scratch_rows, int cu_count) {
  MlaIndexerPrefillRoute r{};
  const auto refuse = [&](int code, const char* why) {
    r.code = code;
    r.why = why;
    return r;
  };
  const MlaRows rows = MlaRows::chunk(nullptr, nullptr, num_rows, num_req, 0);
  MlaIndexerCheck c = rows.negative();
  if (c.code == HPC_OK && max_blocks < 0) c = {HPC_ERR_INVALID, "max_blocks must not be negative"};
  if (c.code == HPC_OK && !logits_only && scratch_rows < 0)
    c = {HPC_ERR_INVALID, "scratch_rows must be 0 (the library chooses) or a row count"};
  if (c.code == HPC_OK) c = rows.limits();
  if (c.code == HPC_OK) c = mla_indexer_shape(num_head, block_size, max_blocks, topk, logits_only, &r.head_blocks, &r.cols);
  if (c.code != HPC_OK) return refuse(c.code, c.why);
  r.tile = kIdxPrefillTile;
  r.tiles = static_cast<int>((static_cast<int64_t>(num_rows) + r.tile - 1) / r.tile);
  r.topk_grid = num_rows;
  // the slab: the caller's, or the rows the budget holds, in whole tiles and at least one; never more than the chunk has
  int64_t slab = num_rows;
  if (!logits_only) {
    slab = scratch_rows > 0 ? scratch_rows : kIdxPrefillScratchBytes / 4 / (r.cols > 0 ? r.cols : 1) / r.tile * r.tile;
    slab = slab < r.tile && scratch_rows == 0 ? r.tile : slab;
    slab = slab > num_rows ? num_rows : slab;
  }
  if (slab > kIdxPrefillMaxScratchBytes / 4 / (r.cols > 0 ? r.cols : 1))
    return refuse(HPC_ERR_UNSUPPORTED, "scratch_rows * max_blocks * block_size * 4 beyond 2^40 bytes of scratch");
  r.slab_rows = static_cast<int>(slab);
  r.slabs = slab > 0 ? static_cast<int>((num_rows + slab - 1) / slab) : 0;
  r.scratch = mla_indexer_scratch(logits_only ? 0 : slab, r.cols);
  r.chunk = mla_indexer_chunk((slab + r.tile - 1) / r.tile, r.cols, cu_count);
  r.chunks = static_cast<int>((r.cols + r.chunk - 1) / r.chunk);
  const int64_t grid = static_cast<int64_t>(r.tiles) * r.chunks;
  if (grid > 0x7fffffffll) return refuse(HPC_ERR_UNSUPPORTED, "the logits grid is beyond int32");
  r.grid = num_req > 0 ? static_cast<int>(grid) : 0;
  return r;
}

// ---- the host rules of the six reader entries, one function per op for both forms: the refusal code and its reason in words, no
// device call.  Each takes the rows of the call and, through them, the form's route. -------------------------------------------
struct MlaIndexerRouted {  // what a check takes from either route
  int code;
  const char* why;
  int64_t cols;
  MlaIndexerScratch scratch;
};
static inline MlaIndexerRouted mla_indexer_routed(const MlaRows& rows, int num_head, int block_size, int max_blocks, int topk,
                                                  bool logits_only, int scratch_rows) {
  if (rows.ragged) {
    const MlaIndexerPrefillRoute r = mla_indexer_prefill_route(rows.num_rows, rows.num_req, num_head, block_size, max_blocks, topk,
                                                               logits_only, scratch_rows, 256);
    return {r.code, r.why, r.cols, r.scratch};
  }
  const MlaIndexerRoute r = mla_indexer_route(rows.num_batch, rows.num_seq_q, num_head, block_size, max_blocks, topk, logits_only, 256);
  return {r.code, r.why, r.cols, r.scratch};
}

static inline MlaIndexerCheck mla_indexer_logits_check(const MlaRows& rows, const float* logits, const void* q, const float* weights,
                                                       const void* k_cache, const int* block_ids, int num_head, int block_size,
                                                       int max_blocks, int num_blocks, int64_t block_stride,
                                                       int64_t logits_row_stride) {
  const MlaIndexerRouted r = mla_indexer_routed(rows, num_head, block_size, max_blocks, 0, true, 0);
  if (r.code != HPC_OK) return {r.code, r.why};
  if (num_blocks < 0) return {HPC_ERR_INVALID, "num_blocks must not be negative"};
  if (rows.row_begin < 0) return {HPC_ERR_INVALID, "row_begin must not be negative"};
  const MlaIndexerCheck fits = rows.limits(kIdxPrefillTile);
  if (fits.code != HPC_OK) return fits;
  const MlaIndexerCheck cache = mla_indexer_cache_check(reinterpret_cast<uintptr_t>(k_cache), block_size, block_stride);
  if (cache.code != HPC_OK) return cache;
  if (rows.work() && (!logits || !q || !weights || !k_cache || !block_ids || !rows.tables()))
    return {HPC_ERR_INVALID, "logits, q, weights, k_cache, block_ids and the rows' tables (the lengths, a chunk's q_index) must not be null"};
  if (rows.work() && max_blocks == 0) return {HPC_ERR_INVALID, "block_ids has no columns"};
  if (misaligned(q, 16) || misaligned(weights, 16) || misaligned(logits, 4))
    return {HPC_ERR_UNSUPPORTED, "q and weights must be 16-byte aligned, logits 4-byte"};
  if (logits_row_stride < r.cols) return {HPC_ERR_UNSUPPORTED, "logits row stride must be at least max_blocks * block_size"};
  if (logits_row_stride > kMaxSpan / 4 / INT32_MAX || (num_blocks > 0 && block_stride > kMaxSpan / num_blocks))
    return {HPC_ERR_UNSUPPORTED, "strides whose offsets would leave 2^60 bytes"};
  return {HPC_OK, nullptr};
}

static inline MlaIndexerCheck mla_indexer_topk_check(const MlaRows& rows, const int* indices, const float* logits, int64_t num_cols,
                                                     int topk, int64_t logits_row_stride) {
  MlaIndexerCheck c = rows.negative();
  if (c.code == HPC_OK && num_cols < 0) c = {HPC_ERR_INVALID, "the logits' column count must not be negative"};
  if (c.code == HPC_OK) c = rows.limits();
  if (c.code != HPC_OK) return c;
  if (topk < 1 || topk > kIdxMaxTopk) return {HPC_ERR_UNSUPPORTED, "topk must be 1 .. 65536"};
  if (num_cols > kIdxMaxCols) return {HPC_ERR_UNSUPPORTED, "logits reach beyond 2^30 columns"};
  // a row that sees no more than topk tokens reads no logit, so a call over zero columns needs no logits at all
  if (rows.work() && (!indices || !rows.tables() || (!logits && num_cols > 0)))
    return {HPC_ERR_INVALID, "indices, logits and the rows' tables (the lengths, a chunk's q_index) must not be null"};
  if (misaligned(indices, 4) || misaligned(logits, 4)) return {HPC_ERR_UNSUPPORTED, "indices and logits must be 4-byte aligned"};
  if (logits_row_stride < num_cols) return {HPC_ERR_UNSUPPORTED, "logits row stride must be at least the column count"};
  if (logits_row_stride > kMaxSpan / 4 / INT32_MAX) return {HPC_ERR_UNSUPPORTED, "strides whose offsets would leave 2^60 bytes"};
  return {HPC_OK, nullptr};
}

// The fused call: the scratch stands in for the logits (without work neither is looked at), then the two checks above.  A
// chunk's list is looked at before its scratch, a step's behind the logits' rules: a call with two faults keeps its code.
static inline MlaIndexerCheck mla_indexer_fused_check(const MlaRows& rows, const int* indices, const void* q, const float* weights,
                                                      const void* k_cache, const int* block_ids, int num_head, int block_size,
                                                      int max_blocks, int num_blocks, int64_t block_stride, int topk,
                                                      int scratch_rows, const void* workspace, int64_t workspace_bytes) {
  const MlaIndexerRouted r = mla_indexer_routed(rows, num_head, block_size, max_blocks, topk, false, scratch_rows);
  if (r.code != HPC_OK) return {r.code, r.why};
  if (rows.ragged && rows.work() && !indices) return {HPC_ERR_INVALID, "indices must not be null"};
  if (rows.ragged && misaligned(indices, 4)) return {HPC_ERR_UNSUPPORTED, "indices must be 4-byte aligned"};
  const float* ws = rows.work() ? static_cast<const float*>(workspace) : nullptr;
  if (rows.work() && (!workspace || workspace_bytes < r.scratch.bytes))
    return {HPC_ERR_INVALID, "the workspace is missing or smaller than the workspace_bytes of the form's plan entry"};
  const MlaIndexerCheck c = mla_indexer_logits_check(rows, ws, q, weights, k_cache, block_ids, num_head, block_size, max_blocks,
                                                     num_blocks, block_stride, r.scratch.row_stride);
  if (c.code != HPC_OK) return c;
  return mla_indexer_topk_check(rows, indices, ws, r.cols, topk, r.scratch.row_stride);
}

// ---- the front end (mla_indexer_prep.hip): LayerNorm + RoPE + rotation + quantisation of the index key and the index queries ----
// One launch over T * (1 + Hi) vectors of 128 columns: the T keys first, then the T * Hi q heads.  A vector is 16 lanes wide, a
// workgroup of 256 threads takes 16 of them.
constexpr int kIdxPrepThreads = 256;
constexpr int kIdxPrepLanes = 16;                                   // lanes of one vector: 8 columns each
constexpr int kIdxPrepVectors = kIdxPrepThreads / kIdxPrepLanes;    // vectors of a workgroup
constexpr int kIdxRope = 64;                                        // columns of a vector that RoPE turns (the FIRST 64), and of a cos_sin row

// Every argument of hpc_mla_indexer_prep_fp8_async the host rule looks at; pointers as integers: none is dereferenced.
struct MlaIndexerPrepCall {
  uintptr_t k_cache, out_k, out_q, out_weights, out_q_rot, k, q, head_weights, k_norm_weight, k_norm_bias, cos_sin,
      num_seqlen_per_req, q_index, block_ids;
  int num_rows, num_req, num_head, block_size, max_blocks, num_blocks, max_pos, head_weights_bf16;
  int64_t block_stride, k_row_stride, q_row_stride, q_head_stride;
  float weight_scale, eps, rotate_scale;
};

// Hi ** -0.5 in double, as Python forms it: the weight_scale of a call is float32(softmax_scale * Hi ** -0.5), formed by the
// caller in double (the torch shim does)
constexpr double mla_indexer_prep_head_factor(int num_head) {
  return num_head == 16 ? 0.25 : num_head == 32 ? 0.1767766952966369 : 0.125;
}

struct MlaIndexerPrepRoute {
  int code;         // HPC_OK or the refusal
  const char* why;  // the refusal in words (null when accepted)
  int head_shift;   // log2(num_head) with q, 0 without: vector T + (r << head_shift) + h is head h of row r
  int64_t vectors;  // T * (1 + Hi) with q, T without
  int grid;         // workgroups of 16 vectors; 0: nothing to launch
};

// The one host rule of the front end: the grid and every refusal with its reason.  q == 0: the key alone, num_head, head_weights
// and weight_scale are not looked at.  k_cache == 0: the key goes to out_k alone and block_size, the block stride and block_ids
// are not looked at.
static inline MlaIndexerPrepRoute mla_indexer_prep_route(const MlaIndexerPrepCall& c) {
  MlaIndexerPrepRoute r{};
  const auto refuse = [&](int code, const char* why) {
    r.code = code;
    r.why = why;
    return r;
  };
  if (c.num_rows < 0 || c.num_req < 0 || c.max_blocks < 0 || c.num_blocks < 0 || c.max_pos < 0)
    return refuse(HPC_ERR_INVALID, "num_rows, num_req, max_blocks, num_blocks and max_pos must not be negative");
  if (!c.k_cache && !c.out_k) return refuse(HPC_ERR_INVALID, "the key has no destination: one of k_cache and out_k must be given");
  const bool with_q = c.q != 0, work = c.num_rows > 0 && c.num_req > 0;
  if (!with_q && (c.out_q || c.out_weights || c.out_q_rot || c.head_weights))
    return refuse(HPC_ERR_INVALID, "out_q, out_weights, out_q_rot and head_weights need q");
  if (with_q) {
    if (c.num_head != 16 && c.num_head != 32 && c.num_head != 64)
      return refuse(HPC_ERR_UNSUPPORTED, "the index head count must be 16, 32 or 64");
    if (!c.head_weights || !(c.weight_scale - c.weight_scale == 0.f))
      return refuse(HPC_ERR_INVALID, "q needs head_weights and a finite weight_scale (softmax_scale * num_head^-0.5)");
    if (!c.out_q || !c.out_weights) return refuse(HPC_ERR_INVALID, "q needs out_q and out_weights");
  }
  if (c.k_cache) {
    const MlaIndexerCheck cache = mla_indexer_cache_check(c.k_cache, c.block_size, c.block_stride);
    if (cache.code != HPC_OK) return refuse(cache.code, cache.why);
  }
  if (work && (!c.k || !c.k_norm_weight || !c.k_norm_bias || !c.cos_sin || !c.num_seqlen_per_req || !c.q_index ||
               (c.k_cache && !c.block_ids)))
    return refuse(HPC_ERR_INVALID, "k, k_norm_weight, k_norm_bias, cos_sin, num_seqlen_per_req, q_index and block_ids must not be null");
  if (work && c.max_pos == 0) return refuse(HPC_ERR_INVALID, "cos_sin has no rows");
  if (!(c.eps >= 0.f) || !(c.rotate_scale - c.rotate_scale == 0.f))
    return refuse(HPC_ERR_INVALID, "eps must not be negative and rotate_scale must be finite");
  if (c.k % 16 || c.q % 16 || c.out_k % 16 || c.out_q_rot % 16 || c.k_norm_weight % 16 || c.k_norm_bias % 16 || c.cos_sin % 16)
    return refuse(HPC_ERR_UNSUPPORTED, "k, q, out_k, out_q_rot, k_norm_weight, k_norm_bias and cos_sin must be 16-byte aligned");
  if (c.out_q % 8 || c.out_weights % 4 || c.head_weights % (c.head_weights_bf16 ? 2 : 4))
    return refuse(HPC_ERR_UNSUPPORTED, "out_q must be 8-byte aligned, out_weights 4-byte and head_weights to its element");
  if (c.k_row_stride < 0 || c.k_row_stride % 8 != 0 || (c.num_rows > 1 && c.k_row_stride < kIdxDim))
    return refuse(HPC_ERR_UNSUPPORTED, "k row stride must be a multiple of 8 elements and at least 128");
  if (with_q) {
    if (c.q_head_stride < 0 || c.q_head_stride % 8 != 0 || c.q_head_stride < kIdxDim)
      return refuse(HPC_ERR_UNSUPPORTED, "q head stride must be a multiple of 8 elements and at least 128");
    if (c.q_row_stride < 0 || c.q_row_stride % 8 != 0 ||
        (c.num_rows > 1 && c.q_row_stride < (c.num_head - 1) * c.q_head_stride + kIdxDim))
      return refuse(HPC_ERR_UNSUPPORTED, "q row stride must be a multiple of 8 elements and hold num_head heads");
  }
  r.head_shift = !with_q ? 0 : c.num_head == 16 ? 4 : c.num_head == 32 ? 5 : 6;
  r.vectors = static_cast<int64_t>(c.num_rows) * (with_q ? 1 + c.num_head : 1);
  if (r.vectors > 0x7fffffffll - kIdxPrepVectors || c.num_req == 0x7fffffff)
    return refuse(HPC_ERR_UNSUPPORTED, "num_rows * (1 + num_head) vectors do not fit int32");
  if (c.k_row_stride > kMaxSpan / 2 / 0x7fffffffll || (with_q && c.q_row_stride > kMaxSpan / 2 / 0x7fffffffll) ||
      (c.k_cache && c.num_blocks > 0 && c.block_stride > kMaxSpan / c.num_blocks))
    return refuse(HPC_ERR_UNSUPPORTED, "strides whose offsets would leave 2^60 bytes");
  r.grid = work ? static_cast<int>((r.vectors + kIdxPrepVectors - 1) / kIdxPrepVectors) : 0;
  return r;
}

}  // namespace hpc
