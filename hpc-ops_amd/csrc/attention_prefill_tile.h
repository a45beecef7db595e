// What the FP8 and the bf16 prefill kernels (attention_prefill.hip, attention_prefill_bf16.hip) state in the same words: the shape of
// a workgroup and the one step of the online softmax that is the same code in both.  Device side; the host side of the two files is
// attention_prefill_route.h.  Only pieces that leave the assembly of both files as it was live here (DESIGN 3.9 names the ones that
// did not: the epilogue's row-major re-read, bf16 pack and store, the KV-span arithmetic and the page-offset products).
#pragma once
#include "attention_prefill_route.h"
#include "hpc_common.h"

namespace hpc {
namespace prefill_tile {

constexpr int kThreads = kPrefillThreads;
constexpr int kWaves = 4;
constexpr int kNB = 2;                  // 16-row q blocks per wave
constexpr int kRowsPerWave = 16 * kNB;  // 32
constexpr int kWgRows = kWaves * kRowsPerWave;
constexpr float kNegInf = -__builtin_inff();
static_assert(kThreads == kWaves * kWave && kWgRows == kPrefillRowTile, "the grid of prefill_route() counts these row tiles");

// Online softmax: the running sum and the output block are rescaled only when some row's maximum moved (past the first tiles of a
// long row it rarely does).  m_use = m_new, or 0 while no key has been seen (m_new = -inf).
__device__ __forceinline__ void rescale_if_max_moved(float m_new, float m_use, float& m_run, float& l_run, f32x4 (&o)[8]) {
  if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
    l_run *= alpha;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) o[jj] *= alpha;
    m_run = m_new;
  }
}

}  // namespace prefill_tile
}  // namespace hpc
