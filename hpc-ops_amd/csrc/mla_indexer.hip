// The DSA lightning indexer of a DeepSeek-V3.2 decode step - gfx950: the writer of the paged FP8 index-key cache, the FP8 MQA
// logits over it and the top-k that turns them into the `indices` of hpc_attention_decode_mla_sparse_*_async.
//
// Ours only (no reference kernel).  Semantics = the float64 PyTorch statement tests/mla_indexer_ref.py; the cache's layout, the
// host rule for a cache and the one route (grid, chunking, scratch, refusals in words) are mla_indexer_route.h's.
//
// MI355X design.
//   store    a stream: 16 lanes own one row of 128 bf16 (one 16-byte load each), the row's abs-max is four xor steps inside the
//            16 lanes, the codes are the project's 128-column quantiser (act_quant.h: bit for bit hpc_blockwise_fp8_quant_async
//            on the row) and leave as one 8-byte store per lane, the scale as one 4-byte store per row.  The request and position
//            of a row are mla_store.hip's: binary search in q_index, one page-table entry, every index checked against a host
//            value before it is used.  Lookup, quantiser and store are mla_indexer_dev.h's, shared with mla_indexer_prep.hip.
//   logits   a 132 B/token stream with one v_mfma_f32_16x16x128_f8f6f4 per 16 heads x 16 tokens: A = q (heads on the rows), B =
//            keys straight from global memory (tokens on the columns, 32 contiguous bytes per lane, no LDS).  Lane (n, g) of the
//            result holds heads 4 g .. 4 g + 3 of token n, so ReLU, the weight and the sum over a lane's heads stay in the lane -
//            in a fixed order - and two xor steps (16, 32) finish the head sum: no atomics, the same bits on every call.  A wave
//            takes 64 tokens per step, four 16-token blocks each inside one page (pages are >= 16 tokens), whose page ids are
//            wave-uniform scalar loads issued one step ahead; lane (n, g) then stores block g's token n: 256 contiguous bytes per
//            wave and q row.  q and the weights of all num_seq_q rows of the request stay in registers, so a key tile is read
//            once for all of them.  A workgroup owns a host-sized chunk of one request's context and leaves at once when the
//            chunk starts at or past the request's end; columns at or past a row's visible length are never written.
//   top-k    one workgroup of 1024 threads per q row.  A row that sees no more than topk tokens writes 0 .. n - 1 and -1 without
//            reading a logit.  Otherwise a radix select over the 32-bit torch_topk_key (ordered_key.h) in four passes of 8 bits
//            with an LDS histogram (integer atomics: the counts do not depend on their order) finds the threshold key and how
//            many of its ties are taken; a last pass compacts in POSITION order by wave ballots and prefix counts - keys above
//            the threshold and the first `need` ties - so the list ascends and ties go to the smaller position.
#include "act_quant.h"
#include "hpc_common.h"
#include "mla_indexer_dev.h"
#include "mla_indexer_route.h"
#include "ordered_key.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace mla_indexer {

// ---- store ------------------------------------------------------------------------------------------------------------------------
struct StoreArgs {
  const uint16_t* k;     // [rows, 128] bf16, row stride k_rs elements
  uint8_t* cache;        // page p at cache + p * cache_bs bytes
  const int* seqlen;     // [num_req] total length incl. the new tokens
  const int* q_index;    // [num_req + 1]
  const int* block_ids;  // [num_req, max_blocks]
  long k_rs, cache_bs;
  int num_rows, num_req, page_shift, max_blocks, num_blocks;
};

constexpr int kStoreThreads = 256, kStoreLanes = 16, kStoreRows = kStoreThreads / kStoreLanes;

__global__ __launch_bounds__(kStoreThreads) void store_kernel(const StoreArgs a) {
  const int sub = threadIdx.x & (kStoreLanes - 1);
  const int row = blockIdx.x * kStoreRows + (threadIdx.x >> 4);  // the host keeps num_rows + kStoreRows within int32
  const bool in = row < a.num_rows;
  u32x4 raw = u32x4{0u, 0u, 0u, 0u};
  if (in) raw = ld16(a.k + row * a.k_rs + 8 * sub);  // in flight before the lookup

  // request and position of this row and its cache cell with their guards: mla_indexer_dev.h
  Cell cell{false, 0, 0};
  if (in) cell = locate_cell(locate_row(a.q_index, a.seqlen, a.num_req, row), a.block_ids, a.page_shift, a.max_blocks, a.num_blocks, a.cache_bs);
  float v[8];
  unpack8(raw, v);
  const float amax = amax16(v);  // every lane takes part
  const float scale = e4m3_block_scale(amax), inv = e4m3_block_inv(scale);
  if (!cell.store) return;
  store_key(a.cache, cell, sub, codes8(v, inv), scale);
}

// ---- logits -----------------------------------------------------------------------------------------------------------------------
struct LogitsArgs {
  const uint8_t* q;      // [B * Sq, Hi, 128] e4m3 codes, contiguous
  const float* w;        // [B * Sq, Hi]
  const uint8_t* cache;  // page p at cache + p * cache_bs bytes
  const int* block_ids;  // [B, max_blocks]
  const int* lens;       // [B]
  float* out;            // row r at out + r * out_rs floats
  long cache_bs, out_rs;
  int page_shift, max_blocks, num_blocks, cols, chunk, chunks, nki;
};

constexpr int kLogitsThreads = 64 * kIdxWaves;

template <int kHB, int kSq>
__global__ __launch_bounds__(kLogitsThreads) void logits_kernel(const LogitsArgs a) {
  constexpr int kHi = 16 * kHB;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int n = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / a.chunks, piece = blockIdx.x % a.chunks;  // b < num_batch: the grid is num_batch * chunks

  // the rows' visible lengths (the step's row rule, mla_indexer_dev.h), clamped to the table: device values never reach an
  // address unchecked
  const long len = step_len(as_const(a.lens)[b], kSq, a.nki);
  int vis[kSq];
#pragma unroll
  for (int s = 0; s < kSq; ++s) vis[s] = step_sees(len, kSq, s, a.cols);
  const int lim = vis[kSq - 1];  // the longest of them
  const int c0 = piece * a.chunk;
  if (c0 >= lim) return;
  const int c1 = min(c0 + a.chunk, lim);

  // q and the weights of the request's rows: lane (n, g) holds bytes 32 g .. 32 g + 31 of head 16 hb + n (the A operand) and the
  // weights of heads 16 hb + 4 g .. + 3 (the rows of the result it holds)
  i32x8 qf[kSq][kHB];
  f32x4 wt[kSq][kHB];
#pragma unroll
  for (int s = 0; s < kSq; ++s) {
    const long r = static_cast<long>(b) * kSq + s;
#pragma unroll
    for (int hb = 0; hb < kHB; ++hb) {
      const uint8_t* p = a.q + (r * kHi + 16 * hb + n) * kIdxDim + 32 * g;
      qf[s][hb] = operand32(ld16(p), ld16(p + 16));
      wt[s][hb] = *reinterpret_cast<const f32x4*>(a.w + r * kHi + 16 * hb + 4 * g);
    }
  }

  const cint_ptr table = as_const(a.block_ids) + static_cast<long>(b) * a.max_blocks;
  // page ids of the four blocks of the step at t0 (wave-uniform); -1 for a block at or past c1.  (t0 + 16 u) >> shift <
  // max_blocks because t0 + 16 u < c1 <= cols = max_blocks << shift.
  const auto lookup = [&](int t0, int (&phys)[kSub]) {
#pragma unroll
    for (int u = 0; u < kSub; ++u) {
      const int j0 = t0 + 16 * u;
      phys[u] = j0 < c1 ? table[j0 >> a.page_shift] : -1;
    }
  };
  const int mask = (1 << a.page_shift) - 1;
  const long scales_at = static_cast<long>(kIdxDim) << a.page_shift;

  int phys[kSub] = {-1, -1, -1, -1}, next[kSub] = {-1, -1, -1, -1};
  int t0 = c0 + wave * kIdxTile;
  if (t0 < c1) lookup(t0, phys);
  for (; t0 < c1; t0 += kIdxTile * kIdxWaves) {
    const int t1 = t0 + kIdxTile * kIdxWaves;
    if (t1 < c1) lookup(t1, next);  // a step ahead of its keys

    // the step's four key blocks, their operand layout and guards: mla_indexer_dev.h
    KeyBlock key[kSub];
#pragma unroll
    for (int u = 0; u < kSub; ++u)
      key[u] = load_key_block(a.cache, a.cache_bs, scales_at, phys[u], a.num_blocks, (t0 + 16 * u + n) & mask, g);
    const int j = t0 + 16 * g + n;  // the column this lane stores
#pragma unroll
    for (int s = 0; s < kSq; ++s) {
      float val[kSub];
#pragma unroll
      for (int u = 0; u < kSub; ++u) val[u] = key_logit(key[u], head_sum<kHB>(qf[s], wt[s], key[u].kv));
      const float mine = g == 0 ? val[0] : g == 1 ? val[1] : g == 2 ? val[2] : val[3];
      if (j < vis[s]) a.out[(static_cast<long>(b) * kSq + s) * a.out_rs + j] = mine;
    }
#pragma unroll
    for (int u = 0; u < kSub; ++u) phys[u] = next[u];
  }
}

// ---- top-k ------------------------------------------------------------------------------------------------------------------------
struct TopkArgs {
  const float* logits;  // row r at logits + r * rs floats
  const int* lens;      // [B]; ragged: num_seqlen_per_req [num_req]
  const int* q_index;   // null: a decode step, row r is (b, s) = (r / sq, r % sq).  Given: a ragged chunk, [num_req + 1]
  int* out;             // [rows, topk]
  long rs;
  int sq, cols, topk, nki, num_req, row_begin;  // ragged: row r of the call is row row_begin + r of the chunk
};

constexpr int kTopkThreads = 1024, kTopkWaves = kTopkThreads / 64, kTopkBatch = 4;

__global__ __launch_bounds__(kTopkThreads) void topk_kernel(const TopkArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t found[2];  // the prefix with the pass's digit behind it, and what is still needed inside it
  __shared__ uint32_t wave_gt[kTopkWaves], wave_tie[kTopkWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x;
  int n;  // the columns row r sees: the one thing the two forms take from different rules (mla_indexer_dev.h)
  if (a.q_index) {
    n = row_sees(a.q_index, a.lens, a.num_req, a.row_begin + r, a.cols).vis;
  } else {
    const int b = r / a.sq, s = r % a.sq;
    n = step_sees(step_len(a.lens[b], a.sq, a.nki), a.sq, s, a.cols);
  }
  int* o = a.out + static_cast<long>(r) * a.topk;
  if (n <= a.topk) {  // the identity list: no logit is read
    for (int i = tid; i < a.topk; i += kTopkThreads) o[i] = i < n ? i : -1;
    return;
  }
  const float* x = a.logits + r * a.rs;

  // radix select: after pass p `prefix` holds the top 8 (p + 1) bits of the threshold key and `need` how many keys with that
  // prefix are still to be taken (every key with a larger prefix is taken)
  uint32_t prefix = 0, need = static_cast<uint32_t>(a.topk);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    // kTopkBatch loads in flight per thread before the first is counted: a long row is one workgroup's stream from L2.
    // (Measured: adding a wave's population of a bin at once - ballots on the first uncounted lane's bin, four rounds, the rest
    // lane by lane - made the 64k row 1.8 x SLOWER than one LDS atomic per lane, 215 against 122 us; not kept.)
    for (int i0 = tid; i0 < n; i0 += kTopkBatch * kTopkThreads) {
      float v[kTopkBatch];
#pragma unroll
      for (int u = 0; u < kTopkBatch; ++u) {
        const int i = i0 + u * kTopkThreads;  // n <= 2^30: no overflow
        v[u] = i < n ? x[i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kTopkBatch; ++u) {
        const uint32_t key = torch_topk_key(v[u]);
        if (i0 + u * kTopkThreads < n && (pass == 0 || (key >> (shift + 8)) == prefix)) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (wave == 0) {
      // lane l owns digits 255 - 4 l .. 252 - 4 l: ascending lanes descend the digits
      uint32_t c[4], sum = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c[k] = hist[255 - 4 * lane - k];
        sum += c[k];
      }
      uint32_t incl = sum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      uint32_t run = incl - sum;  // keys with a larger digit
      if (run < need && need <= incl) {  // exactly one lane: the histogram holds at least `need` keys
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (run < need && need <= run + c[k]) {
            found[0] = (prefix << 8) | static_cast<uint32_t>(255 - 4 * lane - k);
            found[1] = need - run;
          }
          run += c[k];
        }
      }
    }
    __syncthreads();
    prefix = found[0];
    need = found[1];
  }
  const uint32_t thr = prefix;  // the threshold key; `need` of its ties are taken, the first in position order

  // compaction in position order: entry = (keys above the threshold before i) + min(ties before i, need)
  uint32_t gt_base = 0, tie_base = 0;
  for (int base = 0; base < n; base += kTopkThreads) {
    const int i = base + tid;
    const uint32_t key = i < n ? torch_topk_key(x[i]) : 0u;  // 0 is below the key of every float
    const bool gt = key > thr, tie = i < n && key == thr;
    const uint64_t mg = __ballot(gt), mt = __ballot(tie);
    const uint64_t below = (uint64_t{1} << lane) - 1;
    if (lane == 0) {
      wave_gt[wave] = __popcll(mg);
      wave_tie[wave] = __popcll(mt);
    }
    __syncthreads();
    uint32_t gb = gt_base + __popcll(mg & below), tb = tie_base + __popcll(mt & below), tot_g = 0, tot_t = 0;
#pragma unroll
    for (int w = 0; w < kTopkWaves; ++w) {
      const uint32_t cg = wave_gt[w], ct = wave_tie[w];
      if (w < wave) {
        gb += cg;
        tb += ct;
      }
      tot_g += cg;
      tot_t += ct;
    }
    const uint32_t at = gb + (tb < need ? tb : need);  // < topk: keys above + need = topk
    if ((gt || (tie && tb < need)) && at < static_cast<uint32_t>(a.topk)) o[at] = i;
    gt_base += tot_g;
    tie_base += tot_t;
    __syncthreads();  // the counts are rewritten by the next step
  }
}

}  // namespace mla_indexer
}  // namespace hpc

namespace {
using hpc::MlaIndexerCheck;
using hpc::MlaRows;

// ---- the host rule of the store: the refusal code and its reason in words, no device call.  The readers' rules - logits, top-k
// and the fused call, for a decode step and a ragged chunk alike - are mla_indexer_route.h's ---------------------------------------
MlaIndexerCheck store_check(const void* k_cache, const void* k, const int* num_seqlen_per_req, const int* q_index,
                            const int* block_ids, int num_rows, int num_req, int block_size, int max_blocks, int num_blocks,
                            int64_t block_stride, int64_t k_row_stride) {
  using namespace hpc;
  if (num_rows < 0 || num_req < 0 || max_blocks < 0 || num_blocks < 0)
    return {HPC_ERR_INVALID, "num_rows, num_req, max_blocks and num_blocks must not be negative"};
  const bool work = num_rows > 0 && num_req > 0;
  if (work && (!k_cache || !k || !num_seqlen_per_req || !q_index || !block_ids))
    return {HPC_ERR_INVALID, "k_cache, k, num_seqlen_per_req, q_index and block_ids must not be null"};
  const MlaIndexerCheck cache = mla_indexer_cache_check(reinterpret_cast<uintptr_t>(k_cache), block_size, block_stride);
  if (cache.code != HPC_OK) return cache;
  if (misaligned(k, 16)) return {HPC_ERR_UNSUPPORTED, "k must be 16-byte aligned"};
  if (k_row_stride < 0 || k_row_stride % 8 != 0 || (num_rows > 1 && k_row_stride < kIdxDim))
    return {HPC_ERR_UNSUPPORTED, "k row stride must be a multiple of 8 elements and at least 128"};
  if (num_rows > INT32_MAX - mla_indexer::kStoreRows || num_req == INT32_MAX) return {HPC_ERR_UNSUPPORTED, "sizes beyond int32"};
  if (k_row_stride > kMaxSpan / 2 / INT32_MAX || (num_blocks > 0 && block_stride > kMaxSpan / num_blocks))
    return {HPC_ERR_UNSUPPORTED, "strides whose offsets would leave 2^60 bytes"};
  return {HPC_OK, nullptr};
}

// ---- the readers' launchers: the check, nothing without work, the launch ------------------------------------------------------------
template <int kHB>
void launch_logits_sq(const hpc::mla_indexer::LogitsArgs& a, int num_seq_q, int grid, hipStream_t stream) {
  using namespace hpc::mla_indexer;
  switch (num_seq_q) {
    case 1: logits_kernel<kHB, 1><<<grid, kLogitsThreads, 0, stream>>>(a); break;
    case 2: logits_kernel<kHB, 2><<<grid, kLogitsThreads, 0, stream>>>(a); break;
    case 3: logits_kernel<kHB, 3><<<grid, kLogitsThreads, 0, stream>>>(a); break;
    default: logits_kernel<kHB, 4><<<grid, kLogitsThreads, 0, stream>>>(a); break;
  }
}

// the logits of a decode step (a chunk's: mla_indexer_prefill.hip)
int launch_logits(const MlaRows& rows, float* logits, const void* q, const float* weights, const void* k_cache, const int* block_ids,
                  int num_head, int block_size, int max_blocks, int num_blocks, int64_t block_stride, int64_t logits_row_stride,
                  hipStream_t stream) {
  using namespace hpc;
  const MlaIndexerCheck c = mla_indexer_logits_check(rows, logits, q, weights, k_cache, block_ids, num_head, block_size, max_blocks,
                                                     num_blocks, block_stride, logits_row_stride);
  if (c.code != HPC_OK) return c.code;
  if (!rows.work()) return HPC_OK;
  const MlaIndexerRoute r =
      mla_indexer_route(rows.num_batch, rows.num_seq_q, num_head, block_size, max_blocks, 0, true, current_cu_count());
  if (r.code != HPC_OK) return r.code;
  mla_indexer::LogitsArgs a{};
  a.q = static_cast<const uint8_t*>(q);
  a.w = weights;
  a.cache = static_cast<const uint8_t*>(k_cache);
  a.block_ids = block_ids;
  a.lens = rows.lens;
  a.out = logits;
  a.cache_bs = block_stride;
  a.out_rs = logits_row_stride;
  a.page_shift = mla_page_shift(block_size);
  a.max_blocks = max_blocks;
  a.num_blocks = num_blocks;
  a.cols = static_cast<int>(r.cols);
  a.chunk = r.chunk;
  a.chunks = r.chunks;
  a.nki = rows.new_kv_included ? 1 : 0;
  switch (r.head_blocks) {
    case 1: launch_logits_sq<1>(a, rows.num_seq_q, r.grid, stream); break;
    case 2: launch_logits_sq<2>(a, rows.num_seq_q, r.grid, stream); break;
    default: launch_logits_sq<4>(a, rows.num_seq_q, r.grid, stream); break;
  }
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

// the top-k of either form: one workgroup per row, the kernel takes the form from q_index
int launch_topk(const MlaRows& rows, int* indices, const float* logits, int64_t num_cols, int topk, int64_t logits_row_stride,
                hipStream_t stream) {
  using namespace hpc::mla_indexer;
  const MlaIndexerCheck c = hpc::mla_indexer_topk_check(rows, indices, logits, num_cols, topk, logits_row_stride);
  if (c.code != HPC_OK) return c.code;
  if (!rows.work()) return HPC_OK;
  TopkArgs a{};
  a.logits = logits;
  a.lens = rows.lens;
  a.q_index = rows.q_index;
  a.num_req = rows.num_req;
  a.row_begin = rows.row_begin;
  a.out = indices;
  a.rs = logits_row_stride;
  a.sq = rows.num_seq_q;
  a.cols = static_cast<int>(num_cols);
  a.topk = topk;
  a.nki = rows.new_kv_included ? 1 : 0;
  topk_kernel<<<static_cast<int>(rows.rows()), kTopkThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
}  // namespace

// ---- C-ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int hpc_mla_indexer_plan(int num_batch, int num_seq_q, int num_head, int block_size, int max_blocks, int topk, int num_cu,
                                    int* grid, int* chunk, int* topk_grid, int64_t* logits_row_stride, int64_t* workspace_bytes) {
  if (!grid || !chunk || !topk_grid || !logits_row_stride || !workspace_bytes) return HPC_ERR_INVALID;
  const bool logits_only = topk == 0;
  hpc::MlaIndexerRoute r = hpc::mla_indexer_route(num_batch, num_seq_q, num_head, block_size, max_blocks, topk, logits_only,
                                                  num_cu > 0 ? num_cu : 256);
  if (r.code == HPC_OK && num_cu <= 0 && num_batch > 0)
    r = hpc::mla_indexer_route(num_batch, num_seq_q, num_head, block_size, max_blocks, topk, logits_only, hpc::current_cu_count());
  *grid = r.grid, *chunk = r.chunk, *topk_grid = r.topk_grid;
  *logits_row_stride = r.scratch.row_stride, *workspace_bytes = r.scratch.bytes;
  return r.code;
}

extern "C" const char* hpc_mla_indexer_store_k_fp8_refusal(const void* k_cache, const void* k, const int* num_seqlen_per_req,
                                                           const int* q_index, const int* block_ids, int num_rows, int num_req,
                                                           int block_size, int max_blocks, int num_blocks,
                                                           int64_t k_cache_block_stride_bytes, int64_t k_row_stride) {
  return store_check(k_cache, k, num_seqlen_per_req, q_index, block_ids, num_rows, num_req, block_size, max_blocks, num_blocks,
                     k_cache_block_stride_bytes, k_row_stride)
      .why;
}

extern "C" int hpc_mla_indexer_store_k_fp8_async(void* k_cache, const void* k, const int* num_seqlen_per_req, const int* q_index,
                                                 const int* block_ids, int num_rows, int num_req, int block_size, int max_blocks,
                                                 int num_blocks, int64_t k_cache_block_stride_bytes, int64_t k_row_stride,
                                                 hipStream_t stream) {
  using namespace hpc;
  using namespace hpc::mla_indexer;
  const MlaIndexerCheck c = store_check(k_cache, k, num_seqlen_per_req, q_index, block_ids, num_rows, num_req, block_size,
                                        max_blocks, num_blocks, k_cache_block_stride_bytes, k_row_stride);
  if (c.code != HPC_OK) return c.code;
  if (num_rows == 0 || num_req == 0) return HPC_OK;  // nothing to launch
  StoreArgs a{};
  a.k = static_cast<const uint16_t*>(k);
  a.cache = static_cast<uint8_t*>(k_cache);
  a.seqlen = num_seqlen_per_req;
  a.q_index = q_index;
  a.block_ids = block_ids;
  a.k_rs = k_row_stride;
  a.cache_bs = k_cache_block_stride_bytes;
  a.num_rows = num_rows;
  a.num_req = num_req;
  a.page_shift = mla_page_shift(block_size);
  a.max_blocks = max_blocks;
  a.num_blocks = num_blocks;
  store_kernel<<<(num_rows + kStoreRows - 1) / kStoreRows, kStoreThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

extern "C" const char* hpc_mla_indexer_logits_fp8_refusal(const float* logits, const void* q, const float* weights,
                                                          const void* k_cache, const int* block_ids, const int* num_seq_kvcache,
                                                          int num_batch, int num_seq_q, int num_head, int block_size,
                                                          int max_blocks, int num_blocks, int64_t k_cache_block_stride_bytes,
                                                          int64_t logits_row_stride) {
  return hpc::mla_indexer_logits_check(MlaRows::step(num_seq_kvcache, num_batch, num_seq_q, 0), logits, q, weights, k_cache, block_ids,
                                       num_head, block_size, max_blocks, num_blocks, k_cache_block_stride_bytes, logits_row_stride)
      .why;
}

extern "C" int hpc_mla_indexer_logits_fp8_async(float* logits, const void* q, const float* weights, const void* k_cache,
                                                const int* block_ids, const int* num_seq_kvcache, int num_batch, int num_seq_q,
                                                int num_head, int block_size, int max_blocks, int num_blocks,
                                                int64_t k_cache_block_stride_bytes, int64_t logits_row_stride,
                                                int new_kv_included, hipStream_t stream) {
  return launch_logits(MlaRows::step(num_seq_kvcache, num_batch, num_seq_q, new_kv_included), logits, q, weights, k_cache, block_ids,
                       num_head, block_size, max_blocks, num_blocks, k_cache_block_stride_bytes, logits_row_stride, stream);
}

extern "C" const char* hpc_mla_indexer_topk_refusal(const int* indices, const float* logits, const int* num_seq_kvcache,
                                                    int num_batch, int num_seq_q, int64_t num_cols, int topk,
                                                    int64_t logits_row_stride) {
  return hpc::mla_indexer_topk_check(MlaRows::step(num_seq_kvcache, num_batch, num_seq_q, 0), indices, logits, num_cols, topk,
                                     logits_row_stride)
      .why;
}

extern "C" int hpc_mla_indexer_topk_async(int* indices, const float* logits, const int* num_seq_kvcache, int num_batch,
                                          int num_seq_q, int64_t num_cols, int topk, int64_t logits_row_stride, int new_kv_included,
                                          hipStream_t stream) {
  return launch_topk(MlaRows::step(num_seq_kvcache, num_batch, num_seq_q, new_kv_included), indices, logits, num_cols, topk,
                     logits_row_stride, stream);
}

// the top-k of a ragged chunk: the same check, launcher and kernel with the row rule as the source of what a row sees
extern "C" const char* hpc_mla_indexer_topk_prefill_refusal(const int* indices, const float* logits, const int* num_seqlen_per_req,
                                                            const int* q_index, int num_rows, int num_req, int row_begin,
                                                            int64_t num_cols, int topk, int64_t logits_row_stride) {
  return hpc::mla_indexer_topk_check(MlaRows::chunk(num_seqlen_per_req, q_index, num_rows, num_req, row_begin), indices, logits,
                                     num_cols, topk, logits_row_stride)
      .why;
}

extern "C" int hpc_mla_indexer_topk_prefill_async(int* indices, const float* logits, const int* num_seqlen_per_req,
                                                  const int* q_index, int num_rows, int num_req, int row_begin, int64_t num_cols,
                                                  int topk, int64_t logits_row_stride, hipStream_t stream) {
  return launch_topk(MlaRows::chunk(num_seqlen_per_req, q_index, num_rows, num_req, row_begin), indices, logits, num_cols, topk,
                     logits_row_stride, stream);
}

extern "C" const char* hpc_mla_indexer_topk_fp8_refusal(const int* indices, const void* q, const float* weights,
                                                        const void* k_cache, const int* block_ids, const int* num_seq_kvcache,
                                                        int num_batch, int num_seq_q, int num_head, int block_size, int max_blocks,
                                                        int num_blocks, int64_t k_cache_block_stride_bytes, int topk,
                                                        const void* workspace, int64_t workspace_bytes) {
  return hpc::mla_indexer_fused_check(MlaRows::step(num_seq_kvcache, num_batch, num_seq_q, 0), indices, q, weights, k_cache, block_ids,
                                      num_head, block_size, max_blocks, num_blocks, k_cache_block_stride_bytes, topk, 0, workspace,
                                      workspace_bytes)
      .why;
}

// logits then top-k through the scratch, whose layout is mla_indexer_scratch()'s
extern "C" int hpc_mla_indexer_topk_fp8_async(int* indices, const void* q, const float* weights, const void* k_cache,
                                              const int* block_ids, const int* num_seq_kvcache, int num_batch, int num_seq_q,
                                              int num_head, int block_size, int max_blocks, int num_blocks,
                                              int64_t k_cache_block_stride_bytes, int topk, int new_kv_included, void* workspace,
                                              int64_t workspace_bytes, hipStream_t stream) {
  const MlaRows rows = MlaRows::step(num_seq_kvcache, num_batch, num_seq_q, new_kv_included);
  const MlaIndexerCheck c =
      hpc::mla_indexer_fused_check(rows, indices, q, weights, k_cache, block_ids, num_head, block_size, max_blocks, num_blocks,
                                   k_cache_block_stride_bytes, topk, 0, workspace, workspace_bytes);
  if (c.code != HPC_OK) return c.code;
  if (!rows.work()) return HPC_OK;  // nothing to launch
  const hpc::MlaIndexerScratch ws = hpc::mla_indexer_scratch(rows.rows(), static_cast<int64_t>(max_blocks) * block_size);
  float* logits = static_cast<float*>(workspace);
  const int rc = launch_logits(rows, logits, q, weights, k_cache, block_ids, num_head, block_size, max_blocks, num_blocks,
                               k_cache_block_stride_bytes, ws.row_stride, stream);
  if (rc != HPC_OK) return rc;
  return launch_topk(rows, indices, logits, ws.row_stride, topk, ws.row_stride, stream);
}
