// MLA latent-cache gather: paged latent cache (bf16, or the FP8 row of mla_fp8_format.h) -> contiguous bf16 [T, 576] - gfx950.
//
// Ours only (no reference kernel): the step between the cache that hpc_mla_rope_norm_store_kv[_fp8]_async writes and the kv_b
// projection of a chunked-prefill context pass, whose output rows have the shape and meaning of the writer's out_ckv.
// Semantics = the float-free PyTorch statement tests/mla_gather_ref.py: the bf16 cache is copied bit for bit, the FP8 cache is
// dequantised by the code hpc_attention_decode_mla_fp8_async dequantises it with, dequant16 of mla_fp8_format.h
// (c[d] = bf16_rne(fp32(code[d]) * scale[d / 128])).  The row's dimensions and the host rule for a cache: mla_cache.h.
//
// MI355X design: a pure stream, 1,152 bytes out per token - no LDS, no matrix instruction, 16-byte accesses only.  A 64-lane
// wave owns kRowsPerWave = 8 consecutive output rows, a workgroup of four waves a tile of 32:
//   lookup   lane r < 8 resolves row r of the wave on its own: request by binary search in cu_seqlens (as mla_store_kernel does
//            over q_index), position, one page-table entry, the guards - eight dependent chains side by side, not in turn.
//            The result is the row's byte offset in the cache, or one of two marks (not written / written as zeros), and
//            reaches the lanes that move the row by a shuffle;
//   bf16     8 rows x 72 chunks of 16 bytes = 9 chunks per lane: chunk c = 64 i + lane is chunk c % 72 of row c / 72, so a
//            wave instruction covers consecutive bytes of (at most two) rows on both sides;
//   FP8      8 rows x 32 code chunks = 4 per lane (chunk c = 64 i + lane: row c / 32, chunk c % 32, its scale one 4-byte load
//            of the same row), each giving two output chunks, and 8 rows x 8 RoPE chunks = 1 per lane.
// The loads carry no branch - a row that fetches nothing reads a safe address and drops the result - so every load of the
// wave's rows is issued before the first store (9 KiB per wave in flight with the bf16 cache, 5.1 KiB with
// FP8, up to 32 waves per CU); the stores are plain vector stores.  Device values are never trusted with an address: the
// output row comes from the grid and the host's num_rows alone, see `resolve`.
#include "byte_span.h"
#include "hpc_common.h"
#include "mla_cache.h"
#include "mla_fp8_format.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace mla_gather {

struct Args {
  const uint8_t* cache;   // token (page, t) at cache + page * cache_bs + t * cache_ts, strides in BYTES for both kinds
  const uint8_t* safe;    // 1,152 readable bytes: what a row that fetches nothing loads (and discards) instead of branching
  const int* block_ids;   // [num_req, max_blocks]
  const int* cu_seqlens;  // [num_req + 1]
  const int* seq_starts;  // [num_req] or null = zeros
  uint8_t* out;           // row r at out + r * out_rs (bytes), 1,152 bytes written
  long cache_bs, cache_ts, out_rs;
  int num_rows, num_req, page_shift, max_blocks, num_blocks;
};

constexpr int kThreads = 256;
constexpr int kRowsPerWave = 8, kRowsPerBlock = kRowsPerWave * (kThreads / 64);
constexpr int kRowBytes = 2 * kMlaRow;             // 1,152: an output row, and a bf16 cache row
constexpr int kRowChunks = kRowBytes / 16;         // 72
constexpr long kNotWritten = -1, kZeros = -2;      // marks in place of a row's cache offset (an offset is >= 0)

// Where output row `row` comes from: its byte offset in the cache, kZeros for a row of a request whose token cannot be fetched,
// kNotWritten for a row of no request.  Every index is checked against a host value before it is used: b stays in [0, num_req),
// the table column in [0, max_blocks), the page id in [0, num_blocks) - whatever cu_seqlens, seq_starts and block_ids hold.
__device__ __forceinline__ long resolve(const Args& a, const int row) {
  if (row >= a.num_rows) return kNotWritten;
  int lo = 0, hi = a.num_req;  // first b with cu_seqlens[b + 1] > row
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.cu_seqlens[mid + 1] <= row) lo = mid + 1; else hi = mid;
  }
  if (lo >= a.num_req) return kNotWritten;
  // a cu_seqlens that does not ascend can lead the search anywhere: the row is this request's only if it lies in its range
  const int first = a.cu_seqlens[lo];
  if (row < first || row >= a.cu_seqlens[lo + 1]) return kNotWritten;
  const long pos = static_cast<long>(a.seq_starts ? a.seq_starts[lo] : 0) + (row - first);
  if (pos < 0) return kZeros;
  const long blk = pos >> a.page_shift;
  if (blk >= a.max_blocks) return kZeros;
  const int phys = a.block_ids[static_cast<long>(lo) * a.max_blocks + blk];
  if (phys < 0 || phys >= a.num_blocks) return kZeros;  // frameworks pad tables with -1
  return phys * a.cache_bs + (pos & ((1L << a.page_shift) - 1)) * a.cache_ts;
}

__device__ __forceinline__ long shfl_long(const long v, const int src) {
  const uint32_t lo = __shfl(static_cast<int>(static_cast<uint64_t>(v)), src, 64);
  const uint32_t hi = __shfl(static_cast<int>(static_cast<uint64_t>(v) >> 32), src, 64);
  return static_cast<long>(static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32));
}

template <bool kFp8>
__global__ __launch_bounds__(kThreads) void mla_gather_kernel(const Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * kRowsPerBlock + wave * kRowsPerWave;  // the host keeps num_rows + kRowsPerBlock within int32
  if (row0 >= a.num_rows) return;
  const long mine = lane < kRowsPerWave ? resolve(a, row0 + lane) : kNotWritten;
  const u32x4 zero = u32x4{0u, 0u, 0u, 0u};

  if constexpr (!kFp8) {
    constexpr int kN = kRowsPerWave * kRowChunks / 64;  // 9
    static_assert(kRowsPerWave * kRowChunks % 64 == 0, "the wave's rows are a whole number of wave instructions");
    long src[kN];
    u32x4 v[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) {
      const int c = 64 * i + lane, r = c / kRowChunks, k = c % kRowChunks;
      src[i] = shfl_long(mine, r);
      v[i] = ld16((src[i] >= 0 ? a.cache + src[i] : a.safe) + 16 * k);
    }
#pragma unroll
    for (int i = 0; i < kN; ++i) {
      const int c = 64 * i + lane, r = c / kRowChunks, k = c % kRowChunks;
      if (src[i] != kNotWritten) st16(a.out + (row0 + r) * a.out_rs + 16 * k, src[i] >= 0 ? v[i] : zero);
    }
  } else {
    constexpr int kCodeChunks = kMlaLatent / 16;             // 32 per row
    constexpr int kN = kRowsPerWave * kCodeChunks / 64;      // 4 per lane
    constexpr int kRopeChunks = 2 * kMlaRope / 16;           // 8 per row: one per lane
    static_assert(kRowsPerWave * kRopeChunks == 64 && kMlaFp8Group % 16 == 0, "one RoPE chunk per lane, a chunk in one group");
    long src[kN];
    u32x4 codes[kN];
    float scale[kN];
#pragma unroll
    for (int i = 0; i < kN; ++i) {
      const int c = 64 * i + lane, r = c / kCodeChunks, k = c % kCodeChunks;
      src[i] = shfl_long(mine, r);
      const uint8_t* row = src[i] >= 0 ? a.cache + src[i] : a.safe;
      codes[i] = ld16(row + kMlaFp8CodesAt + 16 * k);
      scale[i] = *reinterpret_cast<const float*>(row + kMlaFp8ScalesAt + 4 * (16 * k / kMlaFp8Group));
    }
    const int rr = lane / kRopeChunks, rk = lane % kRopeChunks;
    const long rsrc = shfl_long(mine, rr);
    const u32x4 rope = ld16((rsrc >= 0 ? a.cache + rsrc : a.safe) + kMlaFp8RopeAt + 16 * rk);
#pragma unroll
    for (int i = 0; i < kN; ++i) {
      const int c = 64 * i + lane, r = c / kCodeChunks, k = c % kCodeChunks;
      u32x4 lo, hi;
      dequant16(codes[i], scale[i], lo, hi);
      if (src[i] != kNotWritten) {
        uint8_t* dst = a.out + (row0 + r) * a.out_rs + 32 * k;
        st16(dst, src[i] >= 0 ? lo : zero);
        st16(dst + 16, src[i] >= 0 ? hi : zero);
      }
    }
    if (rsrc != kNotWritten) st16(a.out + (row0 + rr) * a.out_rs + 2 * kMlaLatent + 16 * rk, rsrc >= 0 ? rope : zero);
  }
}

}  // namespace mla_gather
}  // namespace hpc

namespace {
// Both launchers: the checks and the launch.  What a valid cache is - its page size, its strides in the kind's units (bf16
// elements or FP8 bytes) and its alignment - is mla_cache_check() of mla_cache.h.
template <bool kFp8>
int mla_gather_launch(void* out, const void* ckv_cache, const int* block_ids, const int* cu_seqlens, const int* seq_starts,
                      int num_rows, int num_req, int block_size, int max_blocks, int num_blocks, int64_t ckv_block_stride,
                      int64_t ckv_token_stride, int64_t out_row_stride, hipStream_t stream) {
  using namespace hpc;
  using namespace hpc::mla_gather;
  constexpr MlaCacheKind kind = kFp8 ? kMlaCacheFp8 : kMlaCacheBf16;
  // every check on the host, before any device call
  if (num_rows < 0 || num_req < 0 || max_blocks < 0 || num_blocks < 0) return HPC_ERR_INVALID;
  const bool work = num_rows > 0 && num_req > 0;
  if (work && (!out || !ckv_cache || !block_ids || !cu_seqlens)) return HPC_ERR_INVALID;
  const MlaCacheCheck cache =
      mla_cache_check(kind, reinterpret_cast<uintptr_t>(ckv_cache), block_size, ckv_block_stride, ckv_token_stride);
  if (cache.code != HPC_OK) return cache.code;
  if (reinterpret_cast<uintptr_t>(out) % 16 != 0 || out_row_stride < 0 || out_row_stride % 8 != 0) return HPC_ERR_UNSUPPORTED;
  if (num_rows > 1 && out_row_stride < kMlaRow) return HPC_ERR_UNSUPPORTED;  // rows would overlap
  // sizes beyond int32 (the grid's row arithmetic) and cache offsets beyond 64 bits
  if (num_rows > INT32_MAX - kRowsPerBlock || num_req == INT32_MAX) return HPC_ERR_UNSUPPORTED;
  if (ckv_token_stride > kMaxSpan / kind.unit / 128 || out_row_stride > kMaxSpan / 2 / INT32_MAX ||
      (num_blocks > 0 && ckv_block_stride > kMaxSpan / kind.unit / num_blocks))
    return HPC_ERR_UNSUPPORTED;
  if (!work) return HPC_OK;  // nothing to launch

  Args a{};
  a.cache = static_cast<const uint8_t*>(ckv_cache);
  // a row that fetches nothing still issues its loads, from an address that always holds a row: the cache's first cell, or
  // - without a single page - the first output row (num_rows > 0 here; whatever is read there is discarded)
  a.safe = num_blocks > 0 ? a.cache : static_cast<const uint8_t*>(out);
  a.block_ids = block_ids;
  a.cu_seqlens = cu_seqlens;
  a.seq_starts = seq_starts;
  a.out = static_cast<uint8_t*>(out);
  a.cache_bs = ckv_block_stride * kind.unit;
  a.cache_ts = ckv_token_stride * kind.unit;
  a.out_rs = out_row_stride * 2;
  a.num_rows = num_rows;
  a.num_req = num_req;
  a.page_shift = mla_page_shift(block_size);
  a.max_blocks = max_blocks;
  a.num_blocks = num_blocks;
  const int grid = (num_rows + kRowsPerBlock - 1) / kRowsPerBlock;
  mla_gather_kernel<kFp8><<<grid, kThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
}  // namespace

extern "C" int hpc_mla_gather_ckv_async(void* out, const void* ckv_cache, const int* block_ids, const int* cu_seqlens,
                                        const int* seq_starts, int num_rows, int num_req, int block_size, int max_blocks,
                                        int num_blocks, int64_t ckv_block_stride, int64_t ckv_token_stride,
                                        int64_t out_row_stride, hipStream_t stream) {
  return mla_gather_launch<false>(out, ckv_cache, block_ids, cu_seqlens, seq_starts, num_rows, num_req, block_size, max_blocks,
                                  num_blocks, ckv_block_stride, ckv_token_stride, out_row_stride, stream);
}

// the same from the FP8 latent cache (mla_fp8_format.h); the cache's two strides in bytes, the output's in bf16 elements
extern "C" int hpc_mla_gather_ckv_fp8_async(void* out, const void* ckv_cache, const int* block_ids, const int* cu_seqlens,
                                            const int* seq_starts, int num_rows, int num_req, int block_size, int max_blocks,
                                            int num_blocks, int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes,
                                            int64_t out_row_stride, hipStream_t stream) {
  return mla_gather_launch<true>(out, ckv_cache, block_ids, cu_seqlens, seq_starts, num_rows, num_req, block_size, max_blocks,
                                 num_blocks, ckv_block_stride_bytes, ckv_token_stride_bytes, out_row_stride, stream);
}
