// Grouped GEMM with MXFP4 weights and e4m3 activations (group_gemm_mxfp4.hip): how many tokens a pass over the weights serves,
// on which grid, and every refusal - mxfp4_route() is the one statement of it.  Internal header, host only, no HIP calls: a pure
// function of the call's shapes.  hpc_group_gemm_mxfp4_plan and the launcher hpc_group_gemm_mxfp4_async both read it.
#pragma once
#include <stdint.h>

#include "hpc_common.h"

namespace hpc {

constexpr int kMxfp4TileN = 64;  // weight rows per workgroup: four waves x 16 rows

struct Mxfp4Route {
  int code;    // HPC_OK or the refusal; the rest is zero on a refusal and when there is nothing to launch (m == 0)
  int mt;      // 16-token blocks per pass over the weights: 1 / 2 / 3 for at most 10 / at most 22 / more rows per group on average
               // (the thresholds of ggemm_route()'s streaming kernel); longer groups take several passes
  int grid_x;  // n / 64
  int grid_y;  // num_group
};

// x_rows: the rows of x (m without a row_index, the token count with one): the activations are read through one 32-bit buffer.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline Mxfp4Route mxfp4_route(int num_group, int m, int x_rows, int n, int k) {
  Mxfp4Route r{};
  if (num_group <= 0 || m < 0 || x_rows < 0 || n <= 0 || k <= 0) {
    r.code = HPC_ERR_INVALID;
    return r;
  }
  // 128-wide k-blocks (four MX blocks: one scaled MFMA), 64-row tiles, a group's weights and all of x within one 32-bit buffer
  // descriptor each, the group index on the grid's y axis
  if ((k & 127) || (n & (kMxfp4TileN - 1)) || static_cast<int64_t>(n) * k / 2 > 0xfffffff0ll ||
      static_cast<int64_t>(x_rows) * k > 0xfffffff0ll || num_group > 65535) {
    r.code = HPC_ERR_UNSUPPORTED;
    return r;
  }
  if (m == 0) return r;  // nothing to launch
  const int avg = m / num_group;
  r.mt = avg <= 10 ? 1 : (avg <= 22 ? 2 : 3);
  r.grid_x = n / kMxfp4TileN;
  r.grid_y = num_group;
  return r;
}

}  // namespace hpc
