// The row layout the RMSNorm kernels share (rmsnorm.hip: fused_rmsnorm_with_scale; blockwise_quant.hip:
// fused_rmsnorm_blockwise_quant): a row of bf16 held in registers by kTPR threads, and the host ladder that picks
// (kTPR, kNV) for a hidden size.  The sum of squares and the exchange between the waves of a row are written in both
// kernels: moved here as functions they compile to different listings (a branch the other way round, other registers).
#pragma once

#include "hpc_common.h"

namespace hpc {

// kTPR threads of a 256-thread workgroup cooperate on one row (kTPR in {64, 128, 256}: whole waves), kNV 16-byte vectors
// per thread stay in registers, vector i of thread t is vector t + i * kTPR of the row's nvec = hidden / 8.
template <int kTPR>
struct RowMap {
  static constexpr int kRowsPerBlock = 256 / kTPR;
  int64_t row;
  int t, nvec;
  bool row_ok;
  __device__ __forceinline__ RowMap(int rows, int hidden) {
    const int tid = threadIdx.x;
    const int row_in_block = tid / kTPR;
    t = tid % kTPR;
    row = static_cast<int64_t>(blockIdx.x) * kRowsPerBlock + row_in_block;
    row_ok = row < rows;
    nvec = hidden >> 3;
  }
};

}  // namespace hpc

// CASE(kTPR, kNV) for nvec = hidden / 8 16-byte vectors per row; CASE returns.  Past the ladder (nvec > 2048) nothing
// is called: each entry has its own upper bound before or after it.
#define HPC_RMS_LADDER(nvec, CASE)   \
  if ((nvec) <= 64) CASE(64, 1);     \
  if ((nvec) <= 128) CASE(128, 1);   \
  if ((nvec) <= 256) CASE(256, 1);   \
  if ((nvec) <= 512) CASE(256, 2);   \
  if ((nvec) <= 768) CASE(256, 3);   \
  if ((nvec) <= 1024) CASE(256, 4);  \
  if ((nvec) <= 2048) CASE(256, 8)
