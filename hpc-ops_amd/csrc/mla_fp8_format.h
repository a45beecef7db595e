// The FP8 latent KV cache row of the MLA ops, stated once: what hpc_mla_rope_norm_store_kv_fp8_async (mla_store.hip) writes and
// hpc_attention_decode_mla_fp8_async (attention_decode_mla.hip) and hpc_mla_gather_ckv_fp8_async (mla_gather.hip) read.  Internal
// header, host and device: the constants, and under hipcc only the reader's dequantisation (dequant16, at the bottom).  The host
// rule for such a cache is mla_cache.h's, which the torch shim (torch_mla.cpp) checks against; include/hpc_amd.h and the Python
// docstrings restate the row in words.
//
//   bytes   0 .. 511   512 float8_e4m3fn codes: the normalised compressed KV, column d at byte d
//   bytes 512 .. 527   four little-endian fp32 scales; scale g belongs to columns 128 g .. 128 g + 127
//   bytes 528 .. 655   64 bf16: the RoPE'd k_pe, unquantised
//
// Meaning of the codes (the reader):  c[d] = bf16_rne( fp32(code[d]) * scale[d / 128] ), one fp32 multiply, one rounding.
// What the writer produces: per group of 128 columns of its own bf16-rounded latent row, scale = amax / 448 and
// code = e4m3fn_sat( lat * (1 / (scale + 1e-8)) ), every step in fp32 (act_quant.h: e4m3_block_scale, e4m3_block_inv).
// Token stride >= kMlaFp8RowBytes; token and block strides multiples of kMlaFp8Align bytes, base aligned to it: every 16-byte
// load of a row (a code chunk, the scale quad, a RoPE chunk) is aligned, 528 = 33 * 16 and 656 = 41 * 16.
#pragma once

namespace hpc {

constexpr int kMlaFp8RowBytes = 656;  // one token
constexpr int kMlaFp8CodesAt = 0;     // 512 codes
constexpr int kMlaFp8ScalesAt = 512;  // 4 fp32
constexpr int kMlaFp8RopeAt = 528;    // 64 bf16
constexpr int kMlaFp8Group = 128;     // columns per scale
constexpr int kMlaFp8Align = 16;      // of the base and of both strides, bytes
static_assert(kMlaFp8ScalesAt + 4 * 4 == kMlaFp8RopeAt && kMlaFp8RopeAt + 64 * 2 == kMlaFp8RowBytes, "the row is packed");
static_assert(kMlaFp8RopeAt % kMlaFp8Align == 0 && kMlaFp8RowBytes % kMlaFp8Align == 0, "16-byte loads of a row are aligned");

}  // namespace hpc

#ifdef __HIPCC__
#include "hpc_common.h"

namespace hpc {

// The reader's half of the format, the one every kernel that reads the cache uses (attention_decode_mla.hip, mla_gather.hip):
// 16 e4m3 codes -> 16 bf16 = bf16_rne(fp32(code) * scale).
__device__ __forceinline__ void dequant16(const u32x4 codes, const float scale, u32x4& lo, u32x4& hi) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(codes[j]), false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(codes[j]), true);
    w[2 * j] = pack_bf16x2(a[0] * scale, a[1] * scale);
    w[2 * j + 1] = pack_bf16x2(b[0] * scale, b[1] * scale);
  }
  lo = u32x4{w[0], w[1], w[2], w[3]};
  hi = u32x4{w[4], w[5], w[6], w[7]};
}

}  // namespace hpc
#endif  // __HIPCC__
