// Order-preserving integer keys of floats, (key, index) composites and the 64-bit wave operations that move them:
// what the sampler (sampler.hip) and the routers (topk_router.hip) select with.  An arg-max over composites is one
// integer max: the larger key wins, equal keys go to the SMALLER index, and composites of different indices differ.
//
// Two key conventions, because the two ops are pinned to two PyTorch statements:
//   ieee_key        the plain IEEE order: -0.0 < +0.0, a NaN ranks by its bits (above +inf with a clear sign bit).  The
//                   sampler's: its scores go through val_of(key) again (softmax statistics, probabilities), so the
//                   key must be invertible, and its tie rule is stated on the scores' bits.
//   torch_topk_key  torch.topk's order: -0.0 == +0.0 (the tie goes to the smaller index, like every other tie) and
//                   every NaN - whatever its sign bit - ranks above +inf.  The routers': their ids are held to
//                   torch.equal with a stable descending sort.  It is the plain key behind a canonicalisation, so
//                   decoding gives the canonical value (+0.0, the one NaN): all the softmax router needs, exp(x - max)
//                   sees neither the sign of a zero nor a NaN's payload.
#pragma once

#include "hpc_common.h"

namespace hpc {

// the key of a float's bits - monotonic: larger float <-> larger key
__device__ __forceinline__ uint32_t key_of_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t ieee_key(float x) { return key_of_bits(__float_as_uint(x)); }
__device__ __forceinline__ float ieee_key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ uint32_t torch_topk_key(float x) {
  uint32_t u = __float_as_uint(x + 0.0f);  // -0.0 + 0.0 = +0.0
  if (x != x) u = 0x7fc00000u;             // canonical positive NaN
  return key_of_bits(u);
}

// key high, inverted index low; 0 is below every composite of a real element (keys of floats are never 0 with index
// 0xffffffff) and serves as "nothing"
__device__ __forceinline__ uint64_t composite_of(uint32_t key, uint32_t index) {
  return (static_cast<uint64_t>(key) << 32) | (0xffffffffu - index);
}
__device__ __forceinline__ uint32_t index_of(uint64_t c) { return 0xffffffffu - static_cast<uint32_t>(c); }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), o, 64);
  const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), o, 64);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = shfl_xor_u64(v, o);
    v = other > v ? other : v;
  }
  return v;
}

}  // namespace hpc
