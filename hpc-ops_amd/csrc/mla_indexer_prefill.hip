// The DSA lightning indexer over a ragged prefill chunk - gfx950: the FP8 MQA logits of every row of a chunk against the paged
// index-key cache, and the fused logits + top-k over slabs of rows.  The top-k of a chunk is mla_indexer.hip's topk_kernel with
// the row rule as the source of a row's column count.
//
// Ours only (no reference kernel).  Semantics = the float64 statement of tests/mla_indexer_ref.py applied to the expanded form
// of tests/mla_indexer_prefill_ref.py (every row its own one-row request).  The row rule is the writers'
// (mla_indexer_dev.h::locate_row): row r of the chunk belongs to the last request b with q_index[b] <= r at position
// pos = num_seqlen_per_req[b] - (q_index[b + 1] - r) and sees vis = min(pos + 1, max_blocks * P) tokens; a row at or past
// q_index[num_req] or with pos < 0 is a row of no request and is not written.  The one route - tile, chunk, grid, slab, scratch
// and every refusal in words - is mla_indexer_route.h's mla_indexer_prefill_route().
//
// MI355X design.  The decode kernel (mla_indexer.hip) keeps at most four q rows in registers per key tile, so a caller that
// presents a prompt as one-row requests reads every key T / 4 times.  This kernel is key-stationary:
//   rows     a workgroup of eight waves owns a tile of 16 rows cut from the row index of the call (the grid is a host value:
//            ceil(rows / 16) * chunks) and a host-sized chunk of columns, as the decode route cuts them.  Its first 16 threads
//            find the request and vis of the 16 rows; a workgroup whose chunk starts at or past the largest vis leaves at once.
//   q in LDS the 16 rows' codes are staged ONCE, in operand order: for (row, head block, half) the 64 lanes' 16-byte quads lie
//            back to back, so a row's A operands are 2 * Hi / 16 ds_read_b128 of 1 KiB, each conflict-free (lane l at 16 l),
//            and the weights follow as float32 [16, Hi].  16 x Hi x 132 B: 132 KiB at Hi = 64, 66 at 32, 33 at 16, of 160 KiB -
//            one workgroup per CU at Hi = 64; its eight waves are two per SIMD, so that one wave's head sums and lane
//            exchanges run under the other's matrix instructions (measured with four waves, one per SIMD, and a branch per
//            16-key block: 474 us on a fresh 4096-token prompt where this form takes 251 us).  From L2 instead a wave would pull
//            8 KiB of q per 16 matrix instructions, 64 B per clock and CU: the whole L2 port for operands that never change.
//   keys     a wave holds a step of 64 keys as the B operands of v_mfma_f32_16x16x128_f8f6f4 with their scales
//            (mla_indexer_dev.h: load_key_block, the decode kernel's) and runs every row of the tile that sees the step against
//            them before it takes the next: a key tile is loaded once per row tile.  The next step's keys are in flight during
//            the rows of this one, their page ids were looked up a step before that (wave-uniform scalar loads), and the next
//            row's operands are read from LDS while this row's matrix instructions run.
//   segments a tile may straddle requests.  The rows of a tile with the same request are a segment with its own page-table row;
//            the kernel walks the segments (wave-uniform values out of LDS) and runs the key loop once per segment over the
//            columns the segment's longest row sees.
//   result   A = q heads, B = keys, the per-lane fmaf chain over head blocks and the lane's four heads, then the xor-16 and
//            xor-32 steps: mla_indexer_dev.h::head_sum, shared with the decode kernel, so a logit has the same bits from either
//            op.  Lane (n, g) stores block g's token n: 256 contiguous bytes per wave and row.  No float atomics.
//   guards   a request is a request of the call (locate_row), vis <= max_blocks * P, a page id is checked against num_blocks
//            before its page is loaded: no device value reaches an address unchecked.
//   budget   registers: two steps of keys (2 x 36), two rows of operands (2 x 48 at Hi = 64), the result quads and addresses:
//            212 at Hi = 64 (164 at 32, 140 at 16), no spills, inside the 256 a wave has at two waves per SIMD.  LDS as above.
#include "hpc_common.h"
#include "mla_indexer_dev.h"
#include "mla_indexer_route.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace mla_indexer {

struct PrefillArgs {
  const uint8_t* q;      // [num_rows, Hi, 128] e4m3 codes, contiguous: rows row_begin .. of the chunk
  const float* w;        // [num_rows, Hi]
  const uint8_t* cache;  // page p at cache + p * cache_bs bytes
  const int* block_ids;  // [num_req, max_blocks]
  const int* seqlen;     // [num_req] total lengths incl. the chunk's tokens
  const int* q_index;    // [num_req + 1]
  float* out;            // row r of the call at out + r * out_rs floats
  long cache_bs, out_rs;
  int num_rows, num_req, row_begin, page_shift, max_blocks, num_blocks, cols, chunk, chunks;
};

constexpr int kPrefillThreads = 64 * kIdxPrefillWaves;
static_assert(kIdxMinChunk % (kIdxTile * kIdxPrefillWaves) == 0, "a chunk is whole rounds of the workgroup's waves");
constexpr int kTile = kIdxPrefillTile;

template <int kHB>
__global__ __launch_bounds__(kPrefillThreads) void logits_prefill_kernel(const PrefillArgs a) {
  constexpr int kHi = 16 * kHB;
  constexpr int kRowBytes = kHi * kIdxDim;  // a row's codes: 2 * kHB quads of 16 bytes per lane
  __shared__ __attribute__((aligned(16))) uint8_t s_q[kTile * kRowBytes];
  __shared__ __attribute__((aligned(16))) float s_w[kTile * kHi];
  __shared__ int s_req[kTile], s_vis[kTile];
  static_assert(sizeof(s_q) + sizeof(s_w) == mla_indexer_prefill_lds_bytes(kHi), "the route states the LDS of a tile");

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x / a.chunks, piece = blockIdx.x % a.chunks;
  const int l0 = tile * kTile;  // < num_rows: the grid is ceil(num_rows / kTile) * chunks
  const int rows = min(kTile, a.num_rows - l0);
  const int c0 = piece * a.chunk;

  // request and vis of the tile's rows (the row rule, mla_indexer_dev.h); a row past the call's last sees nothing
  if (tid < kTile) {
    RowSees at{0, 0};
    if (tid < rows) at = row_sees(a.q_index, a.seqlen, a.num_req, a.row_begin + l0 + tid, a.cols);  // the host keeps the sum in int32
    s_req[tid] = at.req;
    s_vis[tid] = at.vis;
  }
  __syncthreads();
  int top = 0;
#pragma unroll
  for (int i = 0; i < kTile; ++i) top = max(top, s_vis[i]);
  if (c0 >= __builtin_amdgcn_readfirstlane(top)) return;  // the whole workgroup: nothing of this chunk is seen

  // q and the weights of the tile, once, in operand order: quad ((row kHB + hb) 2 + half) 64 + lane of s_q is lane (n, g)'s
  // bytes 32 g + 16 half .. of head 16 hb + n of the row
  {
    const uint8_t* qt = a.q + static_cast<long>(l0) * kRowBytes;
    // read in memory order - consecutive lanes take consecutive 16 bytes, eight lanes a head - and permuted on the LDS side
    for (int i = tid; i < rows * kHB * 128; i += kPrefillThreads) {
      const int c = i & 7, h = (i >> 3) % kHi, row = i / (8 * kHi);  // quad c of head h of row `row`: bytes 16 c .. of the head
      const int ln = 16 * (c >> 1) + (h & 15), half = c & 1, hb = h >> 4;
      *reinterpret_cast<u32x4*>(s_q + 16 * ((((row * kHB + hb) * 2 + half) << 6) + ln)) = ld16(qt + 16 * i);
    }
    const float* wt = a.w + static_cast<long>(l0) * kHi;
    for (int i = tid; i < rows * kHi / 4; i += kPrefillThreads)
      *reinterpret_cast<f32x4*>(s_w + 4 * i) = *reinterpret_cast<const f32x4*>(wt + 4 * i);
  }
  __syncthreads();

  // row r of the tile as the A operands and the weights of the rows of the result this lane holds
  const auto load_row = [&](int r, i32x8 (&qf)[kHB], f32x4 (&wt)[kHB]) {
    const uint8_t* base = s_q + r * kRowBytes + 16 * lane;
#pragma unroll
    for (int hb = 0; hb < kHB; ++hb) {
      qf[hb] = operand32(*reinterpret_cast<const u32x4*>(base + (2 * hb) * 1024), *reinterpret_cast<const u32x4*>(base + (2 * hb + 1) * 1024));
      wt[hb] = *reinterpret_cast<const f32x4*>(s_w + r * kHi + 16 * hb + 4 * g);
    }
  };

  const int mask = (1 << a.page_shift) - 1;
  const long scales_at = static_cast<long>(kIdxDim) << a.page_shift;

  // the segments of the tile: rows [i, e) of one request, with its page-table row
  for (int i = 0; i < rows;) {
    const int req = __builtin_amdgcn_readfirstlane(s_req[i]);  // in [0, num_req): locate_row
    int e = i + 1, seg_top = __builtin_amdgcn_readfirstlane(s_vis[i]);
    while (e < rows && __builtin_amdgcn_readfirstlane(s_req[e]) == req) {
      seg_top = max(seg_top, __builtin_amdgcn_readfirstlane(s_vis[e]));
      ++e;
    }
    const int c1 = min(c0 + a.chunk, seg_top);  // <= cols

    const cint_ptr table = as_const(a.block_ids) + static_cast<long>(req) * a.max_blocks;
    // page ids of the four blocks of the step at t0 (wave-uniform); -1 for a block at or past c1.  (t0 + 16 u) >> shift <
    // max_blocks because t0 + 16 u < c1 <= cols = max_blocks << shift.
    const auto lookup = [&](int t0, int (&phys)[kSub]) {
#pragma unroll
      for (int u = 0; u < kSub; ++u) {
        const int j0 = t0 + 16 * u;
        phys[u] = j0 < c1 ? table[j0 >> a.page_shift] : -1;
      }
    };
    const auto load_keys = [&](int t0, const int (&phys)[kSub], KeyBlock (&key)[kSub]) {
#pragma unroll
      for (int u = 0; u < kSub; ++u)
        key[u] = load_key_block(a.cache, a.cache_bs, scales_at, phys[u], a.num_blocks, (t0 + 16 * u + n) & mask, g);
    };

    constexpr int kStride = kIdxTile * kIdxPrefillWaves;
    int t0 = c0 + wave * kIdxTile;
    int phys[kSub] = {-1, -1, -1, -1}, ahead[kSub] = {-1, -1, -1, -1};
    KeyBlock key[kSub], next[kSub];
    if (t0 < c1) {
      lookup(t0, phys);
      load_keys(t0, phys, key);
      if (t0 + kStride < c1) lookup(t0 + kStride, phys);  // the next step's, a step ahead of its keys
    }
    for (; t0 < c1; t0 += kStride) {
      if (t0 + 2 * kStride < c1) lookup(t0 + 2 * kStride, ahead);
      const bool more = t0 + kStride < c1;
      if (more) load_keys(t0 + kStride, phys, next);  // in flight during this step's rows

      const int j = t0 + 16 * g + n;  // the column this lane stores; < c0 + chunk, the chunk being a multiple of kStride
      i32x8 qf[kHB];
      f32x4 wt[kHB];
      load_row(i, qf, wt);
      int vis_v = s_vis[i];
      for (int r = i; r < e; ++r) {
        const int vis = __builtin_amdgcn_readfirstlane(vis_v);
        // the next row's operands and vis while this row's products run (nothing of this row waits for them)
        i32x8 qn[kHB];
        f32x4 wn[kHB];
        const int rn = r + 1 < e ? r + 1 : r;
        load_row(rn, qn, wn);
        vis_v = s_vis[rn];
        if (t0 < vis) {  // wave-uniform: a row that ends before this step has nothing in it
          // the four blocks in one straight line, as the decode kernel has them: their matrix instructions, head sums and
          // lane exchanges interleave.  A block at or past vis costs its products; its lanes store nothing.
          float val[kSub];
#pragma unroll
          for (int u = 0; u < kSub; ++u) val[u] = key_logit(key[u], head_sum<kHB>(qf, wt, key[u].kv));
          const float mine = g == 0 ? val[0] : g == 1 ? val[1] : g == 2 ? val[2] : val[3];
          if (j < vis) a.out[static_cast<long>(l0 + r) * a.out_rs + j] = mine;
        }
#pragma unroll
        for (int hb = 0; hb < kHB; ++hb) {
          qf[hb] = qn[hb];
          wt[hb] = wn[hb];
        }
      }
      if (more) {
#pragma unroll
        for (int u = 0; u < kSub; ++u) {
          key[u] = next[u];
          phys[u] = ahead[u];
        }
      }
    }
    i = e;
  }
}

}  // namespace mla_indexer
}  // namespace hpc

// ---- C-ABI: the host rules of these entries are mla_indexer_route.h's, the ones of a decode step's with a chunk's rows --------------
using hpc::MlaIndexerCheck;
using hpc::MlaRows;

extern "C" int hpc_mla_indexer_prefill_plan(int num_rows, int num_req, int num_head, int block_size, int max_blocks, int topk,
                                            int scratch_rows, int num_cu, int* tile, int* grid, int* chunk, int* slab_rows,
                                            int* slabs, int64_t* logits_row_stride, int64_t* workspace_bytes) {
  if (!tile || !grid || !chunk || !slab_rows || !slabs || !logits_row_stride || !workspace_bytes) return HPC_ERR_INVALID;
  const bool logits_only = topk == 0;
  hpc::MlaIndexerPrefillRoute r = hpc::mla_indexer_prefill_route(num_rows, num_req, num_head, block_size, max_blocks, topk,
                                                                 logits_only, scratch_rows, num_cu > 0 ? num_cu : 256);
  if (r.code == HPC_OK && num_cu <= 0 && num_rows > 0 && num_req > 0)
    r = hpc::mla_indexer_prefill_route(num_rows, num_req, num_head, block_size, max_blocks, topk, logits_only, scratch_rows,
                                       hpc::current_cu_count());
  *tile = r.tile, *grid = r.grid, *chunk = r.chunk, *slab_rows = r.slab_rows, *slabs = r.slabs;
  *logits_row_stride = r.scratch.row_stride, *workspace_bytes = r.scratch.bytes;
  return r.code;
}

extern "C" const char* hpc_mla_indexer_logits_prefill_fp8_refusal(const float* logits, const void* q, const float* weights,
                                                                  const void* k_cache, const int* block_ids,
                                                                  const int* num_seqlen_per_req, const int* q_index, int num_rows,
                                                                  int num_req, int row_begin, int num_head, int block_size,
                                                                  int max_blocks, int num_blocks, int64_t k_cache_block_stride_bytes,
                                                                  int64_t logits_row_stride) {
  return hpc::mla_indexer_logits_check(MlaRows::chunk(num_seqlen_per_req, q_index, num_rows, num_req, row_begin), logits, q, weights,
                                       k_cache, block_ids, num_head, block_size, max_blocks, num_blocks, k_cache_block_stride_bytes,
                                       logits_row_stride)
      .why;
}

extern "C" int hpc_mla_indexer_logits_prefill_fp8_async(float* logits, const void* q, const float* weights, const void* k_cache,
                                                        const int* block_ids, const int* num_seqlen_per_req, const int* q_index,
                                                        int num_rows, int num_req, int row_begin, int num_head, int block_size,
                                                        int max_blocks, int num_blocks, int64_t k_cache_block_stride_bytes,
                                                        int64_t logits_row_stride, hipStream_t stream) {
  using namespace hpc;
  using namespace hpc::mla_indexer;
  const MlaRows rows = MlaRows::chunk(num_seqlen_per_req, q_index, num_rows, num_req, row_begin);
  const MlaIndexerCheck c = mla_indexer_logits_check(rows, logits, q, weights, k_cache, block_ids, num_head, block_size, max_blocks,
                                                     num_blocks, k_cache_block_stride_bytes, logits_row_stride);
  if (c.code != HPC_OK) return c.code;
  if (!rows.work()) return HPC_OK;  // nothing to launch
  const MlaIndexerPrefillRoute r =
      mla_indexer_prefill_route(num_rows, num_req, num_head, block_size, max_blocks, 0, true, 0, current_cu_count());
  if (r.code != HPC_OK) return r.code;
  PrefillArgs a{};
  a.q = static_cast<const uint8_t*>(q);
  a.w = weights;
  a.cache = static_cast<const uint8_t*>(k_cache);
  a.block_ids = block_ids;
  a.seqlen = num_seqlen_per_req;
  a.q_index = q_index;
  a.out = logits;
  a.cache_bs = k_cache_block_stride_bytes;
  a.out_rs = logits_row_stride;
  a.num_rows = num_rows;
  a.num_req = num_req;
  a.row_begin = row_begin;
  a.page_shift = mla_page_shift(block_size);
  a.max_blocks = max_blocks;
  a.num_blocks = num_blocks;
  a.cols = static_cast<int>(r.cols);
  a.chunk = r.chunk;
  a.chunks = r.chunks;
  switch (r.head_blocks) {
    case 1: logits_prefill_kernel<1><<<r.grid, kPrefillThreads, 0, stream>>>(a); break;
    case 2: logits_prefill_kernel<2><<<r.grid, kPrefillThreads, 0, stream>>>(a); break;
    default: logits_prefill_kernel<4><<<r.grid, kPrefillThreads, 0, stream>>>(a); break;
  }
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

extern "C" const char* hpc_mla_indexer_topk_prefill_fp8_refusal(const int* indices, const void* q, const float* weights,
                                                                const void* k_cache, const int* block_ids,
                                                                const int* num_seqlen_per_req, const int* q_index, int num_rows,
                                                                int num_req, int num_head, int block_size, int max_blocks,
                                                                int num_blocks, int64_t k_cache_block_stride_bytes, int topk,
                                                                int scratch_rows, const void* workspace, int64_t workspace_bytes) {
  return hpc::mla_indexer_fused_check(MlaRows::chunk(num_seqlen_per_req, q_index, num_rows, num_req, 0), indices, q, weights, k_cache,
                                      block_ids, num_head, block_size, max_blocks, num_blocks, k_cache_block_stride_bytes, topk,
                                      scratch_rows, workspace, workspace_bytes)
      .why;
}

// The two ops over slabs of rows through the scratch: slab s takes rows s * slab_rows .. of the chunk, its logits land in the
// scratch's rows 0 .., its lists in rows s * slab_rows .. of indices.  One stream: a slab's top-k has read the scratch before
// the next slab's logits write it.  The slab count is a host value.
extern "C" int hpc_mla_indexer_topk_prefill_fp8_async(int* indices, const void* q, const float* weights, const void* k_cache,
                                                      const int* block_ids, const int* num_seqlen_per_req, const int* q_index,
                                                      int num_rows, int num_req, int num_head, int block_size, int max_blocks,
                                                      int num_blocks, int64_t k_cache_block_stride_bytes, int topk, int scratch_rows,
                                                      void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  using namespace hpc;
  const MlaRows rows = MlaRows::chunk(num_seqlen_per_req, q_index, num_rows, num_req, 0);
  const MlaIndexerCheck c = mla_indexer_fused_check(rows, indices, q, weights, k_cache, block_ids, num_head, block_size, max_blocks,
                                                    num_blocks, k_cache_block_stride_bytes, topk, scratch_rows, workspace,
                                                    workspace_bytes);
  if (c.code != HPC_OK) return c.code;
  if (!rows.work()) return HPC_OK;  // nothing to launch
  const MlaIndexerPrefillRoute r =
      mla_indexer_prefill_route(num_rows, num_req, num_head, block_size, max_blocks, topk, false, scratch_rows, 256);
  float* logits = static_cast<float*>(workspace);
  for (int s = 0; s < r.slabs; ++s) {
    const int begin = s * r.slab_rows, n = begin + r.slab_rows < num_rows ? r.slab_rows : num_rows - begin;
    int rc = hpc_mla_indexer_logits_prefill_fp8_async(
        logits, static_cast<const uint8_t*>(q) + static_cast<int64_t>(begin) * num_head * kIdxDim,
        weights + static_cast<int64_t>(begin) * num_head, k_cache, block_ids, num_seqlen_per_req, q_index, n, num_req, begin,
        num_head, block_size, max_blocks, num_blocks, k_cache_block_stride_bytes, r.scratch.row_stride, stream);
    if (rc != HPC_OK) return rc;
    rc = hpc_mla_indexer_topk_prefill_async(indices + static_cast<int64_t>(begin) * topk, logits, num_seqlen_per_req, q_index, n,
                                            num_req, begin, r.cols, topk, r.scratch.row_stride, stream);
    if (rc != HPC_OK) return rc;
  }
  return HPC_OK;
}
