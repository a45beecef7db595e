// The front end of the DSA lightning indexer - gfx950: what a DeepSeek-V3.2 layer runs between its wq_b / wk / weights_proj GEMMs
// and hpc_mla_indexer_topk_fp8_async, in ONE launch for the index key and all index-query heads of every new token:
//   key      LayerNorm over the 128 columns -> RoPE on the FIRST 64 -> 128-point Hadamard rotation x rotate_scale -> bf16 -> the
//            128-column quantiser -> the paged index-key cache (bit for bit store_kernel of mla_indexer.hip on the bf16 row)
//   q head   RoPE on the first 64 -> rotation x rotate_scale -> bf16 -> the quantiser -> codes, and the head's weight
//            fp32(fp32(head_weights * scale) * weight_scale), weight_scale = float(softmax_scale * Hi^-0.5) from the caller: the
//            q / weights of the logits op.
//
// Ours only (no reference kernel).  Semantics = the float64 PyTorch statement tests/mla_indexer_prep_ref.py; the host rule (grid
// and every refusal in words) is mla_indexer_route.h's mla_indexer_prep_route; the request / position lookup, the cache cell with
// its guards, the quantiser calls and the store are mla_indexer_dev.h's, shared with store_kernel.
//
// MI355X design.  At decode sizes this is launch latency, at a prefill chunk a stream (4096 tokens x 64 heads: ~100 MB in and
// out), so: no LDS, no matrix instruction.  One vector of 128 columns per 16 lanes - one DPP row -, lane `sub` owns columns
// 8 sub .. 8 sub + 7 behind one 16-byte load issued before the lookup.  Everything between load and store is fp32 with ONE rounding
// to bf16, after the rotation.
//   Hadamard   Sylvester order, y[i] = sum_j (-1)^popcount(i & j) x[j], as seven butterfly stages in natural order (stride 1, 2, 4
//              inside the lane's registers, then across the lanes at xor 1, 2, 4, 8): the lower index takes a + b, the upper a - b.
//              The cross-lane exchanges of the data are ds_swizzle (the LDS crossbar, no LDS memory), those of the reductions DPP
//              row operations (quad_perm for xor 1 and 2, quad reversal then row_half_mirror for xor 4, row_ror:8 for xor 8).
//              A fixed order, no atomics: the same bits on every call.
//   RoPE       neox pairs column i with i + 32: lane sub < 4 holds a, lane sub + 4 holds b - the same xor-4 exchange; interleaved
//              pairs sit inside a lane.  cos / sin come from the table row of the token's position, clamped to max_pos - 1.
//   LayerNorm  mean, then the biased variance of the centred values (two passes over registers), both as a lane sum of 8 and
//              four xor steps; rsqrtf.
//   pow2       scale = the smallest power of two >= amax / 448 (exponent field + 1 when the mantissa is not zero, clamped to
//              [1, 254]); the codes are e4m3(x / scale) by v_ldexp_f32: exact, and saturation cannot trigger.
// Vectors [0, T) are the keys, vector T + (r << log2 Hi) + h is head h of row r, so no division runs on the device.  Lanes of a
// vector past the end, and of a row of no request, keep taking part in every cross-lane step (they read lanes, not memory) and
// write zeros / nothing.  Device values never reach an address unchecked: see locate_cell and the clamp of the table row.
#include "act_quant.h"
#include "hpc_common.h"
#include "mla_indexer_dev.h"
#include "mla_indexer_route.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace mla_indexer {

struct PrepArgs {
  const uint16_t* k;        // [T, 128] bf16, row stride k_rs elements
  const uint16_t* q;        // [T, Hi, 128] bf16, strides q_rs / q_hs elements, or null
  const void* head_w;       // [T, Hi] fp32 or bf16 (hw_bf16), contiguous
  const float* norm_w;      // [128]
  const float* norm_b;      // [128]
  const float* cos_sin;     // [max_pos, 64]: cos[0..31], sin[0..31]
  const int* seqlen;        // [num_req] total length incl. the new tokens
  const int* q_index;       // [num_req + 1]
  const int* block_ids;     // [num_req, max_blocks]
  uint8_t* cache;           // page p at cache + p * cache_bs bytes, or null
  uint16_t* out_k;          // [T, 128] bf16 contiguous, or null
  uint8_t* out_q;           // [T, Hi, 128] e4m3 codes, contiguous
  float* out_w;             // [T, Hi]
  uint16_t* out_q_rot;      // [T, Hi, 128] bf16 contiguous, or null
  long k_rs, q_rs, q_hs, cache_bs;
  int num_rows, num_req, head_shift, vectors, page_shift, max_blocks, num_blocks, max_pos, hw_bf16, pow2;
  float eps, rotate_scale, weight_scale;
};

// the value of the lane this one is paired with at xor kD inside its row of 16 lanes.  v_mov_dpp without an `old` value (every
// lane has a source: full masks, no shifts), so that the compiler may fold the move into the add or max that takes it.
template <int kCtrl>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), kCtrl, 0xf, 0xf, true));
}
template <int kD>
__device__ __forceinline__ float row_xor(float v) {
  static_assert(kD == 1 || kD == 2 || kD == 4 || kD == 8, "a lane's partner inside a row of 16");
  if constexpr (kD == 1) return dpp<0xB1>(v);             // quad_perm [1, 0, 3, 2]
  else if constexpr (kD == 2) return dpp<0x4E>(v);        // quad_perm [2, 3, 0, 1]
  else if constexpr (kD == 4) return dpp<0x141>(dpp<0x1B>(v));  // quad_perm [3, 2, 1, 0], then row_half_mirror
  else return dpp<0x128>(v);                              // row_ror:8
}
// The same exchange through the LDS crossbar (ds_swizzle, bit-mask mode: and 0x1f, xor kD; no LDS memory is touched): for the
// 40 exchanges of a vector's data.  Measured against DPP moves for them (the front end's section): 40.0 against 43.4 us at
// 4096 tokens x 64 heads, 6.1 against 7.0 us at 256 rows - the DPP form costs a VALU slot per move and wait states in front of
// each, and this kernel is short of VALU slots, not of LDS ones.
template <int kD>
__device__ __forceinline__ float data_xor(float v) {
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (kD << 10) | 0x1f));
}
// sum over the 16 lanes of a row: the same value in all of them (an xor tree of commutative adds)
__device__ __forceinline__ float row_sum(float s) {
  s += row_xor<1>(s);
  s += row_xor<2>(s);
  s += row_xor<4>(s);
  s += row_xor<8>(s);
  return s;
}
__device__ __forceinline__ float row_max(float s) {
  s = fmaxf(s, row_xor<1>(s));
  s = fmaxf(s, row_xor<2>(s));
  s = fmaxf(s, row_xor<4>(s));
  s = fmaxf(s, row_xor<8>(s));
  return s;
}

// one cross-lane butterfly stage: the lane with the bit clear holds a and takes a + b, its partner holds b and takes a - b -
// as sign * mine + other, sign = +-1: the product is exact, so these are the bits of a + b and a - b, in two instructions
template <int kD>
__device__ __forceinline__ void butterfly_lanes(float (&v)[8], int sub) {
  const float sign = (sub & kD) != 0 ? -1.0f : 1.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = __builtin_fmaf(v[i], sign, data_xor<kD>(v[i]));
}

// the 128-point Walsh-Hadamard transform in Sylvester order of a vector held 8 columns per lane (column 8 sub + i)
__device__ __forceinline__ void hadamard128(float (&v)[8], int sub) {
#pragma unroll
  for (int h = 1; h < 8; h <<= 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if ((i & h) == 0) {
        const float a = v[i], b = v[i + h];
        v[i] = a + b;
        v[i + h] = a - b;
      }
    }
  }
  butterfly_lanes<1>(v, sub);
  butterfly_lanes<2>(v, sub);
  butterfly_lanes<4>(v, sub);
  butterfly_lanes<8>(v, sub);
}

// RoPE on the first 64 columns (lanes sub < 8).  c, s: the lane's 8 cosines and sines - neox: of pairs 8 (sub & 3) + i, the sines
// NEGATED in the lanes that hold a (sub < 4), so that both halves are mine * c + other * s; interleaved: c[m], s[m], m < 4, of
// pairs 4 sub + m.  Every lane runs the exchange; lanes sub >= 8 hold c = 1, s = 0 and keep their values.
template <bool kInterleaved>
__device__ __forceinline__ void rope64(float (&v)[8], int sub, const float (&c)[8], const float (&s)[8]) {
  if constexpr (kInterleaved) {
    if (sub < 8) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float a = v[2 * m], b = v[2 * m + 1];
        v[2 * m] = a * c[m] - b * s[m];
        v[2 * m + 1] = b * c[m] + a * s[m];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float o = data_xor<4>(v[i]);
      v[i] = v[i] * c[i] + o * s[i];  // a cos - b sin where this lane holds a, b cos + a sin where it holds b
    }
  }
}

// scale of a 128-column block in DeepSeek's ue8m0 form: the smallest power of two at or above amax / 448
__device__ __forceinline__ float pow2_block_scale(float amax, int& exponent) {
  const uint32_t bits = __float_as_uint(e4m3_block_scale(amax));
  int e = static_cast<int>((bits >> 23) & 0xffu) + ((bits & 0x7fffffu) != 0u ? 1 : 0);
  e = e < 1 ? 1 : (e > 254 ? 254 : e);
  exponent = e - 127;
  return __uint_as_float(static_cast<uint32_t>(e) << 23);
}

template <bool kInterleaved>
__global__ __launch_bounds__(kIdxPrepThreads) void prep_kernel(const PrepArgs a) {
  const int sub = threadIdx.x & (kIdxPrepLanes - 1);
  const int vec = blockIdx.x * kIdxPrepVectors + (threadIdx.x >> 4);  // the host keeps vectors + 16 within int32
  const bool in = vec < a.vectors;
  const bool key = vec < a.num_rows;
  const int qv = vec - a.num_rows;                        // q vectors: row-major [T, Hi]
  const int row = key ? vec : qv >> a.head_shift;
  const int head = qv & ((1 << a.head_shift) - 1);

  // ---- the vector's data do not depend on its position: in flight before the lookup --------------------------------------------
  u32x4 raw = u32x4{0u, 0u, 0u, 0u};
  f32x4 w0 = f32x4{0.f, 0.f, 0.f, 0.f}, w1 = w0, b0 = w0, b1 = w0;
  float hw = 0.f;
  if (in) {
    if (key) {
      raw = ld16(a.k + row * a.k_rs + 8 * sub);
      w0 = *reinterpret_cast<const f32x4*>(a.norm_w + 8 * sub);
      w1 = *reinterpret_cast<const f32x4*>(a.norm_w + 8 * sub + 4);
      b0 = *reinterpret_cast<const f32x4*>(a.norm_b + 8 * sub);
      b1 = *reinterpret_cast<const f32x4*>(a.norm_b + 8 * sub + 4);
    } else {
      raw = ld16(a.q + row * a.q_rs + head * a.q_hs + 8 * sub);
      if (sub == 0)
        hw = a.hw_bf16 ? bf16_to_f32(static_cast<const uint16_t*>(a.head_w)[qv]) : static_cast<const float*>(a.head_w)[qv];
    }
  }

  // ---- request, position, cache cell (mla_indexer_dev.h), and the table row of the position --------------------------------------
  RowAt at{false, 0, 0};
  Cell cell{false, 0, 0};
  if (in) {
    at = locate_row(a.q_index, a.seqlen, a.num_req, row);
    if (key && a.cache) cell = locate_cell(at, a.block_ids, a.page_shift, a.max_blocks, a.num_blocks, a.cache_bs);
  }
  float c[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (at.live && sub < 8) {
    const long tp = at.pos < a.max_pos ? at.pos : a.max_pos - 1;  // beyond the table: unspecified result, no read out of bounds
    const float* cs = a.cos_sin + tp * kIdxRope;
    if constexpr (kInterleaved) {
      const f32x4 cc = *reinterpret_cast<const f32x4*>(cs + 4 * sub), ss = *reinterpret_cast<const f32x4*>(cs + 32 + 4 * sub);
#pragma unroll
      for (int m = 0; m < 4; ++m) c[m] = cc[m], s[m] = ss[m];
    } else {
      const int p0 = 8 * (sub & 3);
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(cs + p0), c1 = *reinterpret_cast<const f32x4*>(cs + p0 + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(cs + 32 + p0), s1 = *reinterpret_cast<const f32x4*>(cs + 32 + p0 + 4);
      const float sign = sub < 4 ? -1.0f : 1.0f;  // see rope64
#pragma unroll
      for (int m = 0; m < 4; ++m) c[m] = c0[m], c[m + 4] = c1[m], s[m] = sign * s0[m], s[m + 4] = sign * s1[m];
    }
  }

  float v[8];
  unpack8(raw, v);

  // ---- key: LayerNorm, fp32.  `key` is the same in the 16 lanes of a row, and a DPP row operation reads no lane outside the row
  if (key) {
    float sum = v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) sum += v[i];
    const float mean = row_sum(sum) * (1.0f / kIdxDim);
    float d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = v[i] - mean;
    float sq = d[0] * d[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) sq += d[i] * d[i];
    const float rstd = rsqrtf(row_sum(sq) * (1.0f / kIdxDim) + a.eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = d[i] * rstd * (i < 4 ? w0[i] : w1[i - 4]) + (i < 4 ? b0[i] : b1[i - 4]);
  }

  // ---- RoPE on the first 64 columns, the rotation, the one rounding ---------------------------------------------------------------
  rope64<kInterleaved>(v, sub, c, s);
  hadamard128(v, sub);
  u32x4 rot;
#pragma unroll
  for (int i = 0; i < 4; ++i) rot[i] = pack_bf16x2(v[2 * i] * a.rotate_scale, v[2 * i + 1] * a.rotate_scale);
  if (!at.live) rot = u32x4{0u, 0u, 0u, 0u};  // rows of no request: zeros in every output

  // ---- the 128-column quantiser on the bf16 row: what store_kernel / hpc_blockwise_fp8_quant_async make of it ---------------------
  unpack8(rot, v);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
  amax = row_max(amax);
  float scale;
  u32x2 codes;
  if (a.pow2) {
    int e;
    scale = pow2_block_scale(amax, e);
    float t[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = ldexpf(v[i], -e);
    codes = codes8(t, 1.0f);
  } else {
    scale = e4m3_block_scale(amax);
    codes = codes8(v, e4m3_block_inv(scale));
  }
  if (!in) return;

  if (key) {
    if (cell.store) store_key(a.cache, cell, sub, codes, scale);
    if (a.out_k) st16(a.out_k + static_cast<long>(row) * kIdxDim + 8 * sub, rot);
    return;
  }
  if (!at.live) {
    codes = u32x2{0u, 0u};
    scale = 0.f;
  }
  *reinterpret_cast<u32x2*>(a.out_q + static_cast<long>(qv) * kIdxDim + 8 * sub) = codes;
  if (a.out_q_rot) st16(a.out_q_rot + static_cast<long>(qv) * kIdxDim + 8 * sub, rot);
  if (sub == 0) {
    const float folded = hw * scale;  // two fp32 multiplies, each rounded
    a.out_w[qv] = at.live ? folded * a.weight_scale : 0.f;
  }
}

}  // namespace mla_indexer
}  // namespace hpc

namespace {
hpc::MlaIndexerPrepCall prep_call(const void* k_cache, const void* out_k, const void* out_q, const float* out_weights,
                                  const void* out_q_rot, const void* k, const void* q, const void* head_weights,
                                  const float* k_norm_weight, const float* k_norm_bias, const float* cos_sin,
                                  const int* num_seqlen_per_req, const int* q_index, const int* block_ids, int num_rows, int num_req,
                                  int num_head, int block_size, int max_blocks, int num_blocks, int max_pos,
                                  int64_t k_cache_block_stride_bytes, int64_t k_row_stride, int64_t q_row_stride,
                                  int64_t q_head_stride, int head_weights_bf16, float weight_scale, float eps, float rotate_scale) {
  const auto u = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  hpc::MlaIndexerPrepCall c{};
  c.k_cache = u(k_cache), c.out_k = u(out_k), c.out_q = u(out_q), c.out_weights = u(out_weights), c.out_q_rot = u(out_q_rot);
  c.k = u(k), c.q = u(q), c.head_weights = u(head_weights), c.k_norm_weight = u(k_norm_weight), c.k_norm_bias = u(k_norm_bias);
  c.cos_sin = u(cos_sin), c.num_seqlen_per_req = u(num_seqlen_per_req), c.q_index = u(q_index), c.block_ids = u(block_ids);
  c.num_rows = num_rows, c.num_req = num_req, c.num_head = num_head, c.block_size = block_size, c.max_blocks = max_blocks;
  c.num_blocks = num_blocks, c.max_pos = max_pos, c.head_weights_bf16 = head_weights_bf16;
  c.block_stride = k_cache_block_stride_bytes, c.k_row_stride = k_row_stride, c.q_row_stride = q_row_stride;
  c.q_head_stride = q_head_stride, c.weight_scale = weight_scale, c.eps = eps, c.rotate_scale = rotate_scale;
  return c;
}
}  // namespace

// ---- C-ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" const char* hpc_mla_indexer_prep_fp8_refusal(const void* k_cache, const void* out_k, const void* out_q,
                                                        const float* out_weights, const void* out_q_rot, const void* k,
                                                        const void* q, const void* head_weights, const float* k_norm_weight,
                                                        const float* k_norm_bias, const float* cos_sin,
                                                        const int* num_seqlen_per_req, const int* q_index, const int* block_ids,
                                                        int num_rows, int num_req, int num_head, int block_size, int max_blocks,
                                                        int num_blocks, int max_pos, int64_t k_cache_block_stride_bytes,
                                                        int64_t k_row_stride, int64_t q_row_stride, int64_t q_head_stride,
                                                        int head_weights_bf16, float weight_scale, float eps,
                                                        float rotate_scale) {
  return hpc::mla_indexer_prep_route(prep_call(k_cache, out_k, out_q, out_weights, out_q_rot, k, q, head_weights, k_norm_weight,
                                               k_norm_bias, cos_sin, num_seqlen_per_req, q_index, block_ids, num_rows, num_req,
                                               num_head, block_size, max_blocks, num_blocks, max_pos, k_cache_block_stride_bytes,
                                               k_row_stride, q_row_stride, q_head_stride, head_weights_bf16, weight_scale, eps,
                                               rotate_scale))
      .why;
}

extern "C" int hpc_mla_indexer_prep_fp8_async(void* k_cache, void* out_k, void* out_q, float* out_weights, void* out_q_rot,
                                              const void* k, const void* q, const void* head_weights, const float* k_norm_weight,
                                              const float* k_norm_bias, const float* cos_sin, const int* num_seqlen_per_req,
                                              const int* q_index, const int* block_ids, int num_rows, int num_req, int num_head,
                                              int block_size, int max_blocks, int num_blocks, int max_pos,
                                              int64_t k_cache_block_stride_bytes, int64_t k_row_stride, int64_t q_row_stride,
                                              int64_t q_head_stride, int head_weights_bf16, float weight_scale, float eps,
                                              float rotate_scale, int interleaved, int pow2_scale, hipStream_t stream) {
  using namespace hpc;
  using namespace hpc::mla_indexer;
  const MlaIndexerPrepRoute r = mla_indexer_prep_route(
      prep_call(k_cache, out_k, out_q, out_weights, out_q_rot, k, q, head_weights, k_norm_weight, k_norm_bias, cos_sin,
                num_seqlen_per_req, q_index, block_ids, num_rows, num_req, num_head, block_size, max_blocks, num_blocks, max_pos,
                k_cache_block_stride_bytes, k_row_stride, q_row_stride, q_head_stride, head_weights_bf16, weight_scale, eps,
                rotate_scale));
  if (r.code != HPC_OK) return r.code;
  if (r.grid == 0) return HPC_OK;  // nothing to launch
  PrepArgs a{};
  a.k = static_cast<const uint16_t*>(k);
  a.q = static_cast<const uint16_t*>(q);
  a.head_w = head_weights;
  a.norm_w = k_norm_weight;
  a.norm_b = k_norm_bias;
  a.cos_sin = cos_sin;
  a.seqlen = num_seqlen_per_req;
  a.q_index = q_index;
  a.block_ids = block_ids;
  a.cache = static_cast<uint8_t*>(k_cache);
  a.out_k = static_cast<uint16_t*>(out_k);
  a.out_q = static_cast<uint8_t*>(out_q);
  a.out_w = out_weights;
  a.out_q_rot = static_cast<uint16_t*>(out_q_rot);
  a.k_rs = k_row_stride;
  a.q_rs = q_row_stride;
  a.q_hs = q_head_stride;
  a.cache_bs = k_cache_block_stride_bytes;
  a.num_rows = num_rows;
  a.num_req = num_req;
  a.head_shift = r.head_shift;
  a.vectors = static_cast<int>(r.vectors);
  a.page_shift = k_cache ? mla_page_shift(block_size) : 0;
  a.max_blocks = max_blocks;
  a.num_blocks = num_blocks;
  a.max_pos = max_pos;
  a.hw_bf16 = head_weights_bf16 ? 1 : 0;
  a.pow2 = pow2_scale ? 1 : 0;
  a.eps = eps;
  a.rotate_scale = rotate_scale;
  a.weight_scale = q ? weight_scale : 0.f;
  if (interleaved) prep_kernel<true><<<r.grid, kIdxPrepThreads, 0, stream>>>(a);
  else prep_kernel<false><<<r.grid, kIdxPrepThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
