// MLA latent-cache write: kv_a RMSNorm + RoPE + paged store, bf16 - gfx950.
//
// Ours only (no reference kernel): the producer of hpc_attention_decode_mla_bf16_async's inputs, which defines their wire
// format - one latent row of 576 bf16 per token (512 normalised compressed KV + 64 RoPE'd k_pe) in the paged cache, and the
// RoPE columns of the absorbed-q buffer.  Semantics = the float64 PyTorch statement tests/mla_store_ref.py.  The row's
// dimensions and the host rule for a cache are mla_cache.h's, shared with the cache's readers.
//
// MI355X design: pure stream / latency work like rope.hip - no LDS, no matrix instruction.  One 64-lane wave per unit:
//   latent unit (one per row)      lane l owns columns 8l..8l+7 of the 512 (one 16-byte load, its 8 norm weights loaded
//                                  before the reduction), the sum of squares is a full-wave reduction, one 16-byte store
//                                  per destination; lanes 0..7 also carry the 64 k_pe columns;
//   q unit (one per row, 16 heads) 8 lanes per 128-byte head, two passes of 8 heads behind one position lookup.
//                                  Interleaved pairing: a lane's 16 bytes are four whole pairs.
//                                  Neox pairing: a lane takes the same 8-byte piece of both halves.  Either way lane j turns
//                                  with cos[4j..4j+3] / sin[32+4j..32+4j+3] and no value crosses lanes.
// The data loads are issued before the dependent chain q_index search -> seqlen -> page-table entry (the last in the latent
// unit only), which bounds a decode-sized launch.  Device values are never trusted with an address: see the guards at `live` and `store`.
//
// FP8 latent cache (kFp8, hpc_mla_rope_norm_store_kv_fp8_async): the cache cell is the 656-byte row of mla_fp8_format.h.  Only
// the latent unit's cache store differs.  Lane l owns columns 8 l .. 8 l + 7, so scale group g is lanes 16 g .. 16 g + 15: the
// group amax of the lane's eight bf16-ROUNDED values (what the bf16 writer stores - the FP8 cache is an exact function of it) is
// a four-step xor-shuffle, the codes are the project's 128-column quantiser (act_quant.h) and leave as one 8-byte store per
// lane, the scale as one 4-byte store per group, k_pe unquantised from lanes 0..7.  out_ckv and out_q_pe are the bf16 form's.
#include "act_quant.h"
#include "byte_span.h"
#include "hpc_common.h"
#include "mla_cache.h"
#include "mla_fp8_format.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace mla_store {

struct Args {
  const uint16_t* kv_a;      // [rows, 576] bf16, row stride kv_a_rs
  const uint16_t* q_pe;      // [rows, H, 64] bf16 or null
  const float* cos_sin;      // [max_pos, 64]: cos[0..31], sin[0..31]
  const float* norm_w;       // [512]
  const int* seqlen;         // [num_req] total length incl. the new tokens
  const int* q_index;        // [num_req + 1]
  const int* block_ids;      // [num_req, max_blocks]
  uint16_t* cache;           // token (page, t) at cache + page * cache_bs + t * cache_ts, or null (kFp8: uint8_t, strides in bytes)
  uint16_t* out_ckv;         // [rows, 576], row stride out_ckv_rs, or null
  uint16_t* out_q_pe;        // [rows, H, 64] or null
  long kv_a_rs, q_rs, q_hs, oq_rs, oq_hs, out_ckv_rs, cache_bs, cache_ts;  // elements
  int num_rows, num_req, num_head, page_shift, max_blocks, num_blocks, max_pos;
  float eps;
};

constexpr int kThreads = 256;
constexpr int kHeadsPerGroup = 8;  // 8 lanes per 128-byte head: a wave takes 8 heads per pass
// Groups of 8 heads a q-unit wave takes behind ONE position lookup, like rope.hip's kU = 2.  Measured at 1, 2 and 4
// (profiles/mla_store.txt): 2 is within 0.8 us of the fastest at every size - 64 us against 84 us with 1 at 8192 rows x 128
// heads, level with it at decode sizes - so it is the only form; 4 is no faster than 2 and costs occupancy (94 registers).
constexpr int kGroupsPerWave = 2;

__device__ __forceinline__ void unpack4(const u32x2 r, float* x) {
  x[0] = bf16lo_to_f32(r[0]);
  x[1] = bf16hi_to_f32(r[0]);
  x[2] = bf16lo_to_f32(r[1]);
  x[3] = bf16hi_to_f32(r[1]);
}

// One 64-element RoPE vector, 8 lanes wide.  Lane j holds the pairs 4j..4j+3 as (a[i], b[i]): elements (8j + 2i, 8j + 2i + 1)
// when interleaved, elements (4j + i, 32 + 4j + i) for neox.
template <bool kInterleaved>
struct Piece {
  u32x4 raw;  // interleaved: the lane's 16 bytes; neox: {low half's 8 bytes, high half's 8 bytes}

  __device__ __forceinline__ void load(const uint16_t* vec, int j) {
    if constexpr (kInterleaved) {
      raw = ld16(vec + 8 * j);
    } else {
      const u32x2 lo = *reinterpret_cast<const u32x2*>(vec + 4 * j), hi = *reinterpret_cast<const u32x2*>(vec + 32 + 4 * j);
      raw = u32x4{lo[0], lo[1], hi[0], hi[1]};
    }
  }
  __device__ __forceinline__ void rotate(const f32x4 c, const f32x4 s) {
    float a[4], b[4];
    if constexpr (kInterleaved) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = bf16lo_to_f32(raw[i]);
        b[i] = bf16hi_to_f32(raw[i]);
      }
    } else {
      unpack4(u32x2{raw[0], raw[1]}, a);
      unpack4(u32x2{raw[2], raw[3]}, b);
    }
    float p[4], q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = a[i] * c[i] - b[i] * s[i];
      q[i] = b[i] * c[i] + a[i] * s[i];
    }
    if constexpr (kInterleaved) {
#pragma unroll
      for (int i = 0; i < 4; ++i) raw[i] = pack_bf16x2(p[i], q[i]);
    } else {
      raw = u32x4{pack_bf16x2(p[0], p[1]), pack_bf16x2(p[2], p[3]), pack_bf16x2(q[0], q[1]), pack_bf16x2(q[2], q[3])};
    }
  }
  __device__ __forceinline__ void store(uint16_t* vec, int j) const {
    if constexpr (kInterleaved) {
      st16(vec + 8 * j, raw);
    } else {
      *reinterpret_cast<u32x2*>(vec + 4 * j) = u32x2{raw[0], raw[1]};
      *reinterpret_cast<u32x2*>(vec + 32 + 4 * j) = u32x2{raw[2], raw[3]};
    }
  }
};

// kU groups of 8 heads per q-unit wave (same row): one position lookup for all of them; kFp8: the FP8 cache row
template <bool kInterleaved, int kU, bool kFp8>
__global__ __launch_bounds__(kThreads) void mla_store_kernel(const Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hsub = lane >> 3, j = lane & 7;
  const int q_units = a.q_pe ? (a.num_head + kHeadsPerGroup * kU - 1) / (kHeadsPerGroup * kU) : 0;
  const int units_per_row = 1 + q_units;
  const int work = blockIdx.x * 4 + wave;
  if (work >= a.num_rows * units_per_row) return;
  const int row = work / units_per_row, unit = work % units_per_row;  // unit 0: the latent row, unit u: heads 8 kU (u-1) ..
  const bool latent = unit == 0;
  const int head0 = (unit - 1) * kHeadsPerGroup * kU + hsub;
  // piece u of this lane: a RoPE vector's 16 bytes - k_pe on lanes 0..7 of the latent unit, head head0 + 8u of a q unit
  const auto has_piece = [&](int u) { return latent ? (u == 0 && lane < 8) : head0 + u * kHeadsPerGroup < a.num_head; };

  // ---- the token's data do not depend on its position: in flight before the lookup ---------------------------------
  u32x4 raw = u32x4{0u, 0u, 0u, 0u};
  f32x4 w0 = f32x4{0.f, 0.f, 0.f, 0.f}, w1 = w0;
  Piece<kInterleaved> pe[kU];
  const uint16_t* src_row = a.kv_a + row * a.kv_a_rs;
  if (latent) {
    raw = ld16(src_row + 8 * lane);
    w0 = *reinterpret_cast<const f32x4*>(a.norm_w + 8 * lane);
    w1 = *reinterpret_cast<const f32x4*>(a.norm_w + 8 * lane + 4);
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    pe[u].raw = u32x4{0u, 0u, 0u, 0u};
    if (has_piece(u)) pe[u].load(latent ? src_row + kMlaLatent : a.q_pe + row * a.q_rs + (head0 + u * kHeadsPerGroup) * a.q_hs, j);
  }

  // ---- request and position of this row (wave-uniform): last b with q_index[b] <= row ------------------------------
  const cint_ptr qidx = as_const(a.q_index);
  bool live = row < qidx[a.num_req];  // rows past the last request belong to none
  int lo = 0, hi = a.num_req;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (qidx[mid + 1] <= row) lo = mid + 1; else hi = mid;
  }
  const int req = lo < a.num_req ? lo : a.num_req - 1;  // a q_index that does not ascend must not index past seqlen
  const int pos = as_const(a.seqlen)[req] - (qidx[req + 1] - row);
  live = live && pos >= 0;  // length-0 requests own the padding rows
  // cache cell: nothing is stored for a token whose page the table does not hold, or whose page id is not a page
  const int blk = pos >> a.page_shift;
  bool store = live && latent && a.cache && blk < a.max_blocks;
  long cell = 0;
  if (store) {
    const int phys = as_const(a.block_ids)[static_cast<long>(req) * a.max_blocks + blk];
    store = phys >= 0 && phys < a.num_blocks;  // frameworks pad tables with -1
    cell = phys * a.cache_bs + static_cast<long>(pos & ((1 << a.page_shift) - 1)) * a.cache_ts;
  }
  if (live) {
    const int tp = pos < a.max_pos ? pos : a.max_pos - 1;  // beyond the table: unspecified result, no read out of bounds
    const float* cs = a.cos_sin + static_cast<long>(tp) * kMlaRope + 4 * j;
    const f32x4 c = *reinterpret_cast<const f32x4*>(cs), s = *reinterpret_cast<const f32x4*>(cs + 32);
#pragma unroll
    for (int u = 0; u < kU; ++u) pe[u].rotate(c, s);  // a piece that does not exist turns zeros
  }

  if (!latent) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      // rows of no request: zeros, so that no uninitialised memory reaches a later kernel
      if (!live) pe[u].raw = u32x4{0u, 0u, 0u, 0u};
      if (has_piece(u)) pe[u].store(a.out_q_pe + row * a.oq_rs + (head0 + u * kHeadsPerGroup) * a.oq_hs, j);
    }
    return;
  }

  // ---- latent row: RMSNorm over the 512 columns, fp32, one rounding -------------------------------------------------
  float x[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = bf16lo_to_f32(raw[i]);
    x[2 * i + 1] = bf16hi_to_f32(raw[i]);
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss += x[i] * x[i];
  const float r = rsqrtf(wave_sum(ss) * (1.0f / kMlaLatent) + a.eps);
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float wa = i < 2 ? w0[2 * i] : w1[2 * i - 4], wb = i < 2 ? w0[2 * i + 1] : w1[2 * i - 3];
    o[i] = pack_bf16x2(x[2 * i] * r * wa, x[2 * i + 1] * r * wb);
  }
  if constexpr (kFp8) {
    // the bf16-rounded values, quantised per 128 columns = 16 lanes (the shuffles run on every lane: `store` is per wave anyway)
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = bf16lo_to_f32(o[i]);
      v[2 * i + 1] = bf16hi_to_f32(o[i]);
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
    const float scale = e4m3_block_scale(amax), inv = e4m3_block_inv(scale);
    if (store) {
      uint8_t* row = reinterpret_cast<uint8_t*>(a.cache) + cell;
      *reinterpret_cast<u32x2*>(row + kMlaFp8CodesAt + 8 * lane) =
          u32x2{quant_4xe4m3(v[0] * inv, v[1] * inv, v[2] * inv, v[3] * inv), quant_4xe4m3(v[4] * inv, v[5] * inv, v[6] * inv, v[7] * inv)};
      if ((lane & 15) == 0) *reinterpret_cast<float*>(row + kMlaFp8ScalesAt + 4 * (lane >> 4)) = scale;
      if (lane < 8) pe[0].store(reinterpret_cast<uint16_t*>(row + kMlaFp8RopeAt), j);
    }
  } else if (store) {
    st16(a.cache + cell + 8 * lane, o);
    if (lane < 8) pe[0].store(a.cache + cell + kMlaLatent, j);
  }
  if (a.out_ckv) {
    if (!live) {
      o = u32x4{0u, 0u, 0u, 0u};
      pe[0].raw = o;
    }
    uint16_t* dst = a.out_ckv + row * a.out_ckv_rs;
    st16(dst + 8 * lane, o);
    if (lane < 8) pe[0].store(dst + kMlaLatent, j);
  }
}

}  // namespace mla_store
}  // namespace hpc

namespace {
// Both launchers: the checks and the launch.  What a valid cache is - its page size, its strides in the kind's units (bf16
// elements or FP8 bytes) and its alignment - is mla_cache_check() of mla_cache.h; a call without a cache skips it.
template <bool kFp8>
int mla_store_launch(void* ckv_cache, void* out_ckv, void* out_q_pe, const void* kv_a, const void* q_pe, const float* cos_sin,
                     const float* kv_norm_weight, const int* num_seqlen_per_req, const int* q_index, const int* block_ids,
                     int num_rows, int num_req, int num_head, int block_size, int max_blocks, int num_blocks, int max_pos,
                     int64_t ckv_block_stride, int64_t ckv_token_stride, int64_t kv_a_row_stride, int64_t out_ckv_row_stride,
                     int64_t q_pe_row_stride, int64_t q_pe_head_stride, int64_t out_q_pe_row_stride,
                     int64_t out_q_pe_head_stride, float eps, int interleaved, hipStream_t stream) {
  using namespace hpc;
  using namespace hpc::mla_store;
  constexpr MlaCacheKind kind = kFp8 ? kMlaCacheFp8 : kMlaCacheBf16;
  // every check on the host, before any device call
  if (num_rows < 0 || num_req < 0 || num_head < 0 || max_blocks < 0 || num_blocks < 0 || max_pos < 0) return HPC_ERR_INVALID;
  if (!kv_a || !cos_sin || !kv_norm_weight || !num_seqlen_per_req || !q_index) return HPC_ERR_INVALID;
  if (!ckv_cache && !out_ckv) return HPC_ERR_INVALID;      // neither destination
  if ((q_pe == nullptr) != (out_q_pe == nullptr)) return HPC_ERR_INVALID;
  if (ckv_cache && !block_ids) return HPC_ERR_INVALID;
  if (max_pos == 0) return HPC_ERR_INVALID;
  if (ckv_cache) {  // behind every other invalid argument, in front of everything else that is not supported
    const MlaCacheCheck cache =
        mla_cache_check(kind, reinterpret_cast<uintptr_t>(ckv_cache), block_size, ckv_block_stride, ckv_token_stride);
    if (cache.code != HPC_OK) return cache.code;
  }
  const auto misaligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 != 0; };
  const auto bad_stride = [](int64_t s) { return s < 0 || s % 8 != 0; };
  if (q_pe && (num_head < 1 || num_head > 128)) return HPC_ERR_UNSUPPORTED;
  if (misaligned(kv_a) || misaligned(cos_sin) || misaligned(kv_norm_weight) || bad_stride(kv_a_row_stride)) return HPC_ERR_UNSUPPORTED;
  if (num_rows > 1 && kv_a_row_stride < kMlaRow) return HPC_ERR_UNSUPPORTED;
  if (out_ckv && (misaligned(out_ckv) || bad_stride(out_ckv_row_stride))) return HPC_ERR_UNSUPPORTED;
  if (out_ckv && num_rows > 1 && out_ckv_row_stride < kMlaRow) return HPC_ERR_UNSUPPORTED;  // rows would overlap
  if (q_pe && (misaligned(q_pe) || misaligned(out_q_pe) || bad_stride(q_pe_row_stride) || bad_stride(q_pe_head_stride) ||
               bad_stride(out_q_pe_row_stride) || bad_stride(out_q_pe_head_stride)))
    return HPC_ERR_UNSUPPORTED;
  if (q_pe && ((num_head > 1 && (q_pe_head_stride < kMlaRope || out_q_pe_head_stride < kMlaRope)) ||
               (num_rows > 1 && (q_pe_row_stride < kMlaRope || out_q_pe_row_stride < kMlaRope))))
    return HPC_ERR_UNSUPPORTED;  // heads or rows would overlap
  if (q_pe && num_rows > 0) {
    // an output row must end before the next one starts, and out_q_pe may share memory with q_pe only as the same tensor
    // (in place: a lane reads and writes the same bytes); any other overlap would let one wave read what another wrote
    if (num_rows > 1 && out_q_pe_row_stride < (num_head - 1) * out_q_pe_head_stride + kMlaRope) return HPC_ERR_UNSUPPORTED;
    const bool in_place = q_pe == out_q_pe && q_pe_row_stride == out_q_pe_row_stride && q_pe_head_stride == out_q_pe_head_stride;
    const ByteSpan in = byte_span(q_pe, num_rows, q_pe_row_stride, num_head, q_pe_head_stride, kMlaRope, 2);
    const ByteSpan out = byte_span(out_q_pe, num_rows, out_q_pe_row_stride, num_head, out_q_pe_head_stride, kMlaRope, 2);
    if (!in_place && overlap(in, out)) return HPC_ERR_UNSUPPORTED;
  }
  const int q_units = q_pe ? (num_head + kHeadsPerGroup * kGroupsPerWave - 1) / (kHeadsPerGroup * kGroupsPerWave) : 0;
  const int64_t units = static_cast<int64_t>(num_rows) * (1 + q_units);  // one wave each
  if (units > INT32_MAX - 4) return HPC_ERR_UNSUPPORTED;
  if (num_rows == 0 || num_req == 0) return HPC_OK;  // nothing to launch

  Args a{};
  a.kv_a = static_cast<const uint16_t*>(kv_a);
  a.q_pe = static_cast<const uint16_t*>(q_pe);
  a.cos_sin = cos_sin;
  a.norm_w = kv_norm_weight;
  a.seqlen = num_seqlen_per_req;
  a.q_index = q_index;
  a.block_ids = block_ids;
  a.cache = static_cast<uint16_t*>(ckv_cache);
  a.out_ckv = static_cast<uint16_t*>(out_ckv);
  a.out_q_pe = static_cast<uint16_t*>(out_q_pe);
  a.kv_a_rs = kv_a_row_stride;
  a.q_rs = q_pe_row_stride;
  a.q_hs = q_pe_head_stride;
  a.oq_rs = out_q_pe_row_stride;
  a.oq_hs = out_q_pe_head_stride;
  a.out_ckv_rs = out_ckv_row_stride;
  a.cache_bs = ckv_block_stride;
  a.cache_ts = ckv_token_stride;
  a.num_rows = num_rows;
  a.num_req = num_req;
  a.num_head = num_head;
  a.page_shift = ckv_cache ? mla_page_shift(block_size) : 0;
  a.max_blocks = ckv_cache ? max_blocks : 0;
  a.num_blocks = num_blocks;
  a.max_pos = max_pos;
  a.eps = eps;
  const int grid = static_cast<int>((units + 3) / 4);
  if (interleaved) mla_store_kernel<true, kGroupsPerWave, kFp8><<<grid, kThreads, 0, stream>>>(a);
  else mla_store_kernel<false, kGroupsPerWave, kFp8><<<grid, kThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
}  // namespace

extern "C" int hpc_mla_rope_norm_store_kv_async(void* ckv_cache, void* out_ckv, void* out_q_pe, const void* kv_a, const void* q_pe,
                                                const float* cos_sin, const float* kv_norm_weight, const int* num_seqlen_per_req,
                                                const int* q_index, const int* block_ids, int num_rows, int num_req, int num_head,
                                                int block_size, int max_blocks, int num_blocks, int max_pos,
                                                int64_t ckv_block_stride, int64_t ckv_token_stride, int64_t kv_a_row_stride,
                                                int64_t out_ckv_row_stride, int64_t q_pe_row_stride, int64_t q_pe_head_stride,
                                                int64_t out_q_pe_row_stride, int64_t out_q_pe_head_stride, float eps,
                                                int interleaved, hipStream_t stream) {
  return mla_store_launch<false>(ckv_cache, out_ckv, out_q_pe, kv_a, q_pe, cos_sin, kv_norm_weight, num_seqlen_per_req, q_index,
                                 block_ids, num_rows, num_req, num_head, block_size, max_blocks, num_blocks, max_pos,
                                 ckv_block_stride, ckv_token_stride, kv_a_row_stride, out_ckv_row_stride, q_pe_row_stride,
                                 q_pe_head_stride, out_q_pe_row_stride, out_q_pe_head_stride, eps, interleaved, stream);
}

// the same into the FP8 latent cache (mla_fp8_format.h); the cache's two strides in bytes, every other stride in bf16 elements
extern "C" int hpc_mla_rope_norm_store_kv_fp8_async(void* ckv_cache, void* out_ckv, void* out_q_pe, const void* kv_a,
                                                    const void* q_pe, const float* cos_sin, const float* kv_norm_weight,
                                                    const int* num_seqlen_per_req, const int* q_index, const int* block_ids,
                                                    int num_rows, int num_req, int num_head, int block_size, int max_blocks,
                                                    int num_blocks, int max_pos, int64_t ckv_block_stride_bytes,
                                                    int64_t ckv_token_stride_bytes, int64_t kv_a_row_stride,
                                                    int64_t out_ckv_row_stride, int64_t q_pe_row_stride, int64_t q_pe_head_stride,
                                                    int64_t out_q_pe_row_stride, int64_t out_q_pe_head_stride, float eps,
                                                    int interleaved, hipStream_t stream) {
  return mla_store_launch<true>(ckv_cache, out_ckv, out_q_pe, kv_a, q_pe, cos_sin, kv_norm_weight, num_seqlen_per_req, q_index,
                                block_ids, num_rows, num_req, num_head, block_size, max_blocks, num_blocks, max_pos,
                                ckv_block_stride_bytes, ckv_token_stride_bytes, kv_a_row_stride, out_ckv_row_stride,
                                q_pe_row_stride, q_pe_head_stride, out_q_pe_row_stride, out_q_pe_head_stride, eps, interleaved,
                                stream);
}
