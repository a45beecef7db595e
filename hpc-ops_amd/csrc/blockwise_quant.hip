// 128-block e4m3 activation quantisation for gfx950, alone (blockwise_fp8_quant) and behind residual add + RMSNorm
// (fused_rmsnorm_blockwise_quant): the producers of the (x e4m3 [T, H], x_scale f32 [T, H/128]) pair that
// fuse_moe_blockwise* and group_gemm_blockwise_fp8 take.  No reference kernel exists; the PyTorch statement is
// tests/blockwise_quant_ref.py.  The arithmetic of a block is act_quant.h's (e4m3_block_scale, e4m3_block_inv), the one
// the MoE's own second GEMM input is quantised by.
//
// Both forms are HBM-bound.  A 16-byte vector of bf16 is 8 columns, so 16 consecutive lanes - one DPP row - own one
// 128-column block and its abs-max is four steps inside the row (block128_amax).
#include "act_quant.h"
#include "rmsnorm_row.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace {

// max with the lane a DPP row operation pairs this one with (rows are 16 lanes: a quant block's lanes)
template <int kCtrl>
__device__ __forceinline__ float dpp_max(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), kCtrl, 0xf, 0xf, false);
  return fmaxf(v, __int_as_float(o));
}

// abs-max of 8 values, then over the 16 lanes that share a 128-column block: the xor tree (1, 2, 4, 8) of
// act_mul_blockwise_quant_kernel, its steps as DPP row operations instead of __shfl_xor's ds_bpermute (an LDS round
// trip each).  Same bits - a maximum does not depend on the order -, 0.2-0.8 us less per call at decode sizes and 7 %
// at T = 4096 for the quant-only kernel (profiles/blockwise_quant.txt).
__device__ __forceinline__ float block128_amax(const float (&a)[8]) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(a[j]));
  amax = dpp_max<0xB1>(amax);   // quad_perm [1, 0, 3, 2]: lane ^ 1
  amax = dpp_max<0x4E>(amax);   // quad_perm [2, 3, 0, 1]: lane ^ 2
  amax = dpp_max<0x141>(amax);  // row_half_mirror: the quads agree, so this is the other quad of the 8
  amax = dpp_max<0x140>(amax);  // row_mirror: the other half of the 16
  return amax;
}

// 8 values of a block -> 8 e4m3 codes; returns the block's scale (the same in its 16 lanes)
__device__ __forceinline__ float quant_block128(const float (&a)[8], u32x2& q) {
  const float scale = e4m3_block_scale(block128_amax(a));
  const float inv = e4m3_block_inv(scale);
  q[0] = quant_4xe4m3(a[0] * inv, a[1] * inv, a[2] * inv, a[3] * inv);
  q[1] = quant_4xe4m3(a[4] * inv, a[5] * inv, a[6] * inv, a[7] * inv);
  return scale;
}

__device__ __forceinline__ void bf16x8_to_f32(u32x4 v, float (&a)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[2 * j] = bf16lo_to_f32(v[j]);
    a[2 * j + 1] = bf16hi_to_f32(v[j]);
  }
}

// ---- quant only ----------------------------------------------------------------------------------------------------
// 8 consecutive input values as fp32; kDtype as hpc_scaled_fp8_quant_async's in_dtype: 0 bf16, 1 fp16, 2 fp32
template <int kDtype>
__device__ __forceinline__ void load8(const void* in, int64_t c8, float (&a)[8]) {
  if constexpr (kDtype == 0) {
    bf16x8_to_f32(ld16_nt(static_cast<const uint16_t*>(in) + c8 * 8), a);
  } else if constexpr (kDtype == 1) {
    typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
    const f16x8 h = __builtin_bit_cast(f16x8, ld16_nt(static_cast<const uint16_t*>(in) + c8 * 8));
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = static_cast<float>(h[j]);
  } else {
    const float* p = static_cast<const float*>(in) + c8 * 8;
    const u32x4 lo = ld16_nt(p), hi = ld16_nt(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = __uint_as_float(lo[j]);
      a[4 + j] = __uint_as_float(hi[j]);
    }
  }
}

// The input is contiguous and H % 128 == 0, so the op is flat: chunk c (8 columns) of the [T * H / 8] chunks goes to
// out[c * 8 ...] and its block's scale to out_scale[c >> 4]; no row index is needed.  One thread per chunk, kU chunks
// per thread a whole grid apart (all loaded before the first is used).  chunks % 16 == 0: the 16 lanes of a block are
// in range together.
template <int kDtype, int kU>
__global__ __launch_bounds__(256) void blockwise_quant_kernel(const void* __restrict__ in, uint8_t* __restrict__ out,
                                                              float* __restrict__ out_scale, int64_t chunks) {
  const int64_t c0 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t step = static_cast<int64_t>(gridDim.x) * 256;
  float a[kU][8];
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t c = c0 + u * step;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[u][j] = 0.f;
    if (c < chunks) load8<kDtype>(in, c, a[u]);
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t c = c0 + u * step;
    u32x2 q;
    const float scale = quant_block128(a[u], q);
    if (c >= chunks) continue;
    *reinterpret_cast<u32x2*>(out + c * 8) = q;
    if ((threadIdx.x & 15) == 0) out_scale[c >> 4] = scale;
  }
}

template <int kDtype>
int launch_quant(const void* in, void* out, float* out_scale, int64_t chunks, hipStream_t stream) {
  // up to 2048 workgroups' worth of chunks: one per thread; beyond, two per thread
  const bool two = chunks > 2048 * 256;
  const int64_t per_block = two ? 512 : 256;
  const int64_t grid = (chunks + per_block - 1) / per_block;
  if (grid > 0x7fffffff) return HPC_ERR_UNSUPPORTED;
  if (two)
    blockwise_quant_kernel<kDtype, 2><<<static_cast<unsigned>(grid), 256, 0, stream>>>(in, (uint8_t*)out, out_scale, chunks);
  else
    blockwise_quant_kernel<kDtype, 1><<<static_cast<unsigned>(grid), 256, 0, stream>>>(in, (uint8_t*)out, out_scale, chunks);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

// ---- residual add + RMSNorm + quant ----------------------------------------------------------------------------------
// The row layout is rmsnorm.hip's rmsnorm_scale_kernel's (RowMap, rmsnorm_row.h), and so is the pass up to `rms`.  kTPR % 16 == 0
// and H / 8 % 16 == 0, so the 16 lanes of a group hold one 128-column block in every i and are in range together.
// kRes: h = bf16(x + residual) is stored back to residual and normed; kNormed: the bf16 y is stored too.  The codes
// and scales are those of the bf16-ROUNDED y, i.e. of blockwise_quant_kernel on the normed output.
// kNV = 8 (H > 8192) asks for 4 waves per SIMD: left alone the compiler keeps every weight vector and product of the
// unrolled row live (224-233 VGPRs, 1-2 waves per SIMD); held to 128 it needs 90-91, without scratch.
template <int kTPR, int kNV, bool kRes, bool kNormed>
__global__ __launch_bounds__(256, (kNV >= 8 ? 4 : 1)) void rmsnorm_blockwise_quant_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w, uint16_t* __restrict__ residual,
    uint8_t* __restrict__ out_fp8, float* __restrict__ out_scale, uint16_t* __restrict__ out_normed, float eps, int rows,
    int hidden) {
  constexpr int kWavesPerRow = kTPR / kWave;
  __shared__ float red[4];

  const int tid = threadIdx.x;
  const RowMap<kTPR> m(rows, hidden);
  const int t = m.t, nvec = m.nvec;
  const int64_t row = m.row;
  const bool row_ok = m.row_ok;

  u32x4 xv[kNV];
#pragma unroll
  for (int i = 0; i < kNV; ++i) {
    const int v = t + i * kTPR;
    xv[i] = u32x4{0u, 0u, 0u, 0u};
    if (row_ok && v < nvec) xv[i] = ld16_nt(x + row * hidden + v * 8);
  }
  if constexpr (kRes) {
    u32x4 rv[kNV];
#pragma unroll
    for (int i = 0; i < kNV; ++i) {
      const int v = t + i * kTPR;
      rv[i] = u32x4{0u, 0u, 0u, 0u};
      if (row_ok && v < nvec) rv[i] = ld16_nt(residual + row * hidden + v * 8);
    }
#pragma unroll
    for (int i = 0; i < kNV; ++i) {
      const int v = t + i * kTPR;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        xv[i][j] = pack_bf16x2(bf16lo_to_f32(xv[i][j]) + bf16lo_to_f32(rv[i][j]),
                               bf16hi_to_f32(xv[i][j]) + bf16hi_to_f32(rv[i][j]));
      if (row_ok && v < nvec) st16(residual + row * hidden + v * 8, xv[i]);
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < kNV; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = bf16lo_to_f32(xv[i][j]), b = bf16hi_to_f32(xv[i][j]);
      ss = fmaf(a, a, ss);
      ss = fmaf(b, b, ss);
    }
  }
  ss = wave_sum(ss);
  if constexpr (kWavesPerRow > 1) {
    const int wave = tid >> 6;
    if ((tid & 63) == 0) red[wave] = ss;
    __syncthreads();
    const int w0 = (wave / kWavesPerRow) * kWavesPerRow;
    ss = 0.f;
#pragma unroll
    for (int k = 0; k < kWavesPerRow; ++k) ss += red[w0 + k];
  }
  const float rms = rsqrtf(ss / static_cast<float>(hidden) + eps);
  if (!row_ok) return;  // whole waves: a row is kTPR >= 64 threads

#pragma unroll
  for (int i = 0; i < kNV; ++i) {
    const int v = t + i * kTPR;
    if (v >= nvec) continue;  // whole 16-lane groups
    const u32x4 wv = ld16(w + v * 8);
    u32x4 yv;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      yv[j] = pack_bf16x2(bf16lo_to_f32(xv[i][j]) * rms * bf16lo_to_f32(wv[j]),
                          bf16hi_to_f32(xv[i][j]) * rms * bf16hi_to_f32(wv[j]));
    float y[8];
    bf16x8_to_f32(yv, y);
    u32x2 q;
    const float scale = quant_block128(y, q);
    const int64_t o = row * hidden + v * 8;
    *reinterpret_cast<u32x2*>(out_fp8 + o) = q;
    if ((tid & 15) == 0) out_scale[row * (hidden >> 7) + (v >> 4)] = scale;
    if constexpr (kNormed) st16(out_normed + o, yv);
  }
}

template <int kTPR, int kNV>
int launch_norm(const void* x, const void* w, void* residual, void* o8, float* os, void* on, float eps, int rows,
                int hidden, hipStream_t stream) {
  constexpr int kRowsPerBlock = RowMap<kTPR>::kRowsPerBlock;
  const int grid = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
#define HPC_BQ_LAUNCH(RES, NORMED)                                                                               \
  rmsnorm_blockwise_quant_kernel<kTPR, kNV, RES, NORMED><<<grid, 256, 0, stream>>>(                              \
      (const uint16_t*)x, (const uint16_t*)w, (uint16_t*)residual, (uint8_t*)o8, os, (uint16_t*)on, eps, rows, hidden)
  if (residual && on)
    HPC_BQ_LAUNCH(true, true);
  else if (residual)
    HPC_BQ_LAUNCH(true, false);
  else if (on)
    HPC_BQ_LAUNCH(false, true);
  else
    HPC_BQ_LAUNCH(false, false);
#undef HPC_BQ_LAUNCH
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace
}  // namespace hpc

extern "C" int hpc_blockwise_fp8_quant_async(void* output_fp8, float* output_scale, const void* input, int in_dtype,
                                             int num_tokens, int hidden, hipStream_t stream) {
  using namespace hpc;
  if (num_tokens < 0 || in_dtype < 0 || in_dtype > 2) return HPC_ERR_INVALID;
  if (hidden < 128 || hidden > 16384 || (hidden & 127)) return HPC_ERR_UNSUPPORTED;
  if (num_tokens == 0) return HPC_OK;
  if (!output_fp8 || !output_scale || !input) return HPC_ERR_INVALID;
  if (!aligned(input, 16) || !aligned(output_fp8, 8) || !aligned(output_scale, 4)) return HPC_ERR_UNSUPPORTED;
  const int64_t chunks = static_cast<int64_t>(num_tokens) * (hidden >> 3);
  if (in_dtype == 0) return launch_quant<0>(input, output_fp8, output_scale, chunks, stream);
  if (in_dtype == 1) return launch_quant<1>(input, output_fp8, output_scale, chunks, stream);
  return launch_quant<2>(input, output_fp8, output_scale, chunks, stream);
}

extern "C" int hpc_fused_rmsnorm_blockwise_quant_async(void* output_fp8, float* output_scale, void* output_normed,
                                                       const void* input, const void* weight, void* residual, float eps,
                                                       int num_tokens, int hidden, hipStream_t stream) {
  using namespace hpc;
  if (num_tokens < 0) return HPC_ERR_INVALID;
  if (hidden < 128 || hidden > 16384 || (hidden & 127)) return HPC_ERR_UNSUPPORTED;
  if (num_tokens == 0) return HPC_OK;
  if (!output_fp8 || !output_scale || !input || !weight) return HPC_ERR_INVALID;
  if (!aligned(input, 16) || !aligned(weight, 16) || !aligned(residual, 16) || !aligned(output_normed, 16) ||
      !aligned(output_fp8, 8) || !aligned(output_scale, 4))
    return HPC_ERR_UNSUPPORTED;
  const int nvec = hidden / 8;
#define HPC_BQ_CASE(TPR, NV) \
  return launch_norm<TPR, NV>(input, weight, residual, output_fp8, output_scale, output_normed, eps, num_tokens, hidden, stream)
  HPC_RMS_LADDER(nvec, HPC_BQ_CASE);  // one case is taken: hidden <= 16384 above
#undef HPC_BQ_CASE
  return HPC_ERR_UNSUPPORTED;
}
