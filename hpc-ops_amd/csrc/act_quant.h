// The gate-up activation of the fused MoE and its e4m3 quantisation, stated once: a = silu(gate) * up on the bf16 GEMM
// output, then either one scale per 128 columns (scale = amax / 448, q = e4m3(a / (scale + 1e-8)); reference
// src/activation/activation.cu:282-355) or one scale per tensor, with the product formed in bf16 when use_bf16_mul
// (src/activation/activation.cu:19-75, :54-65).  The stand-alone kernels (csrc/fuse_moe.hip: act_mul_blockwise_quant_kernel,
// act_mul_quant_kernel) and the fused epilogues of the grouped GEMM (csrc/group_gemm_p8.hip: `finish`, the ride-along block,
// tail_finish) both call these functions, so they agree bit for bit by construction
// (tests/test_fuse_moe_blockwise.py::test_fused_activation_epilogue,
// tests/test_fuse_moe_pertensor.py::test_fuse_moe_pertensor_activation_epilogue).  Internal: not part of the C-ABI.
#pragma once

#include "hpc_common.h"

namespace hpc {

__device__ __forceinline__ float silu(float g) { return g / (1.0f + __expf(-g)); }

// blockwise form: everything in fp32
__device__ __forceinline__ float silu_mul(float g, float u) { return silu(g) * u; }

// the product of the reference's bf16 path: SiLU rounded to bf16, times up, rounded to bf16 again
__device__ __forceinline__ float mul_bf16_rounded(float sv, float u) {
  return bf16_to_f32(f32_to_bf16(bf16_to_f32(f32_to_bf16(sv)) * u));
}
// per-tensor form before its scale: the bf16-rounded product when use_bf16_mul, the fp32 product otherwise
__device__ __forceinline__ float silu_mul_pt(float g, float u, int use_bf16_mul) {
  float sv = silu(g);
  if (use_bf16_mul)
    sv = mul_bf16_rounded(sv, u);
  else
    sv *= u;
  return sv;
}
__device__ __forceinline__ float silu_mul_scaled(float g, float u, int use_bf16_mul, float sc) {
  return silu_mul_pt(g, u, use_bf16_mul) * sc;
}

// two packed bf16 pairs -> four floats (by reference: the array never leaves registers)
__device__ __forceinline__ void bf16x4_to_f32(uint32_t lo, uint32_t hi, float (&f)[4]) {
  f[0] = bf16lo_to_f32(lo);
  f[1] = bf16hi_to_f32(lo);
  f[2] = bf16lo_to_f32(hi);
  f[3] = bf16hi_to_f32(hi);
}

// scale of a 128-column block from its abs-max, and the factor its values are multiplied by before the e4m3 cast
__device__ __forceinline__ float e4m3_block_scale(float amax) { return amax / 448.0f; }
__device__ __forceinline__ float e4m3_block_inv(float scale) { return 1.0f / (scale + 1e-8f); }

}  // namespace hpc
