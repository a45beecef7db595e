// Device pieces the writers of the index-key cache share (mla_indexer.hip: store_kernel; mla_indexer_prep.hip: prep_kernel), stated
// once: the request and position of a row, the cache cell of a token with its guards, the 16-lane abs-max, the 128-column
// quantiser on a vector held as 8 columns per lane, and the store of a token's 128 + 4 bytes.  Internal, device only.
// Behind them what the READERS share (mla_indexer.hip: logits_kernel, topk_kernel; mla_indexer_prefill.hip: logits_prefill_kernel;
// attention_decode_mla.hip: the token-sparse form): the operand roles, the key block and the head sum of a logit, and the two
// row rules as what a row sees - row_sees for a ragged chunk, step_sees for a decode step.
#pragma once
#include "act_quant.h"
#include "hpc_common.h"
#include "mla_indexer_route.h"

namespace hpc {
namespace mla_indexer {

// Request and position of row `row`, as mla_store.hip: the last b with q_index[b] <= row, pos = seqlen[b] - (q_index[b + 1] -
// row); live is false for a row at or past q_index[num_req] and for pos < 0 (a row of no request).  num_req >= 1.
struct RowAt {
  bool live;
  int req;
  long pos;
};
__device__ __forceinline__ RowAt locate_row(const int* q_index, const int* seqlen, int num_req, int row) {
  bool live = row < q_index[num_req];
  int lo = 0, hi = num_req;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q_index[mid + 1] <= row) lo = mid + 1; else hi = mid;
  }
  const int req = lo < num_req ? lo : num_req - 1;  // a q_index that does not ascend must not index past seqlen
  const long pos = static_cast<long>(seqlen[req]) - (static_cast<long>(q_index[req + 1]) - row);
  live = live && pos >= 0;
  return {live, req, pos};
}

// Where the token of `at` lies in the cache: nothing is stored for a row of no request, a token whose page the table does not
// hold, or whose page id is not a page.  Every device value is checked against a host value before it reaches an address.
struct Cell {
  bool store;
  long codes_at, scale_at;  // bytes from the cache's base
};
__device__ __forceinline__ Cell locate_cell(const RowAt& at, const int* block_ids, int page_shift, int max_blocks, int num_blocks,
                                            long cache_bs) {
  Cell c{false, 0, 0};
  const long blk = at.pos >> page_shift;
  if (at.live && blk < max_blocks) {
    const int phys = block_ids[static_cast<long>(at.req) * max_blocks + blk];
    c.store = phys >= 0 && phys < num_blocks;  // frameworks pad tables with -1
    const long t = at.pos & ((1L << page_shift) - 1);
    c.codes_at = phys * cache_bs + t * kIdxDim;
    c.scale_at = phys * cache_bs + (static_cast<long>(kIdxDim) << page_shift) + 4 * t;
  }
  return c;
}

// 16 bytes of bf16 -> the lane's 8 columns
__device__ __forceinline__ void unpack8(const u32x4 raw, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = bf16lo_to_f32(raw[i]);
    v[2 * i + 1] = bf16hi_to_f32(raw[i]);
  }
}

// abs-max of a vector of 128 columns held 8 per lane by 16 consecutive lanes: every lane of the wave takes part
__device__ __forceinline__ float amax16(const float (&v)[8]) {
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
  return amax;
}

// the lane's 8 codes: the project's quantiser (act_quant.h) with the multiplier `inv`
__device__ __forceinline__ u32x2 codes8(const float (&v)[8], float inv) {
  return u32x2{quant_4xe4m3(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv), quant_4xe4m3(v[4] * inv, v[5] * inv, v[6] * inv, v[7] * inv)};
}

// the 128 + 4 bytes of a token: 8 bytes per lane, the scale from the vector's first lane
__device__ __forceinline__ void store_key(uint8_t* cache, const Cell& c, int sub, u32x2 codes, float scale) {
  *reinterpret_cast<u32x2*>(cache + c.codes_at + 8 * sub) = codes;
  if (sub == 0) *reinterpret_cast<float*>(cache + c.scale_at) = scale;
}

// ---- the readers: logits_kernel (mla_indexer.hip, a decode step) and logits_prefill_kernel (mla_indexer_prefill.hip, a ragged
// chunk).  The operand roles, the key block and the head sum are stated here once, so that logit (row, j) has the same bits from
// either kernel: A = 16 q heads (lane (n, g) holds bytes 32 g .. 32 g + 31 of head 16 hb + n), B = 16 keys (lane (n, g) holds
// bytes 32 g .. 32 g + 31 of token n of the block), and lane (n, g) of the result holds heads 16 hb + 4 g .. + 3 of token n.
constexpr int kSub = kIdxTile / 16;  // 16-token blocks of a wave's step
static_assert(kSub == 4, "lane group g stores block g");

__device__ __forceinline__ int clamp_len(long v, int cols) { return static_cast<int>(v < 0 ? 0 : (v > cols ? cols : v)); }

__device__ __forceinline__ i32x8 operand32(const u32x4 x, const u32x4 y) {
  return i32x8{static_cast<int>(x[0]), static_cast<int>(x[1]), static_cast<int>(x[2]), static_cast<int>(x[3]),
               static_cast<int>(y[0]), static_cast<int>(y[1]), static_cast<int>(y[2]), static_cast<int>(y[3])};
}

// One 16-token block of a page as the B operand, with the scale of the lane's token n.  `phys` is a device value: a block at
// or past the end of the piece (-1), -1 padding and a poisoned id are not ok, and such a page is never loaded.
struct KeyBlock {
  i32x8 kv;
  float sc;
  bool ok;
};
__device__ __forceinline__ KeyBlock load_key_block(const uint8_t* cache, long cache_bs, long scales_at, int phys, int num_blocks,
                                                   int t, int g) {
  KeyBlock k{i32x8{0, 0, 0, 0, 0, 0, 0, 0}, 0.f, phys >= 0 && phys < num_blocks};
  if (k.ok) {
    const uint8_t* page = cache + phys * cache_bs;
    k.kv = operand32(ld16(page + t * kIdxDim + 32 * g), ld16(page + t * kIdxDim + 32 * g + 16));
    k.sc = *reinterpret_cast<const float*>(page + scales_at + 4 * t);
  }
  return k;
}

// sum_h w[h] * relu(q[h] . key) of the lane's token, before the key's scale: per lane the fmaf chain over the head blocks and
// the lane's four heads, then the xor-16 and xor-32 steps - a fixed order, no atomics
template <int kHB>
__device__ __forceinline__ float head_sum(const i32x8 (&qf)[kHB], const f32x4 (&wt)[kHB], const i32x8 kv) {
  float acc = 0.f;
#pragma unroll
  for (int hb = 0; hb < kHB; ++hb) {
    const f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(qf[hb], kv, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = fmaf(wt[hb][i], fmaxf(d[i], 0.f), acc);
  }
  acc += __shfl_xor(acc, 16, 64);
  acc += __shfl_xor(acc, 32, 64);
  return acc;
}
__device__ __forceinline__ float key_logit(const KeyBlock& k, float acc) { return k.ok ? k.sc * acc : -__builtin_inff(); }

// The ragged row rule of the readers: what row `row` of a chunk sees, vis = min(pos + 1, cols) for a live row and 0 for a row
// of no request; req is a request of the call either way (locate_row)
struct RowSees {
  int req, vis;
};
__device__ __forceinline__ RowSees row_sees(const int* q_index, const int* seqlen, int num_req, int row, int cols) {
  const RowAt at = locate_row(q_index, seqlen, num_req, row);
  return {at.req, at.live ? clamp_len(at.pos + 1, cols) : 0};
}

// The decode-step row rule of the readers: what row (b, s) of a step of sq rows per request sees.  step_len is the request's
// length including the new tokens, L = lens[b] + (new_kv_included ? 0 : sq); row s sees the L - sq + s + 1 first of them, never
// beyond the page table's reach (so a position below vis has a page-table entry).  Two functions, so that a kernel with several
// rows of a request forms L once.
__device__ __forceinline__ long step_len(int len_b, int sq, int new_kv_included) {
  return static_cast<long>(len_b) + (new_kv_included ? 0 : sq);
}
__device__ __forceinline__ int step_sees(long len, int sq, int s, int cols) { return clamp_len(len - sq + s + 1, cols); }

}  // namespace mla_indexer
}  // namespace hpc
