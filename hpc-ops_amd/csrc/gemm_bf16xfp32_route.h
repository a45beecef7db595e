// Which router-GEMM kernel runs for a call, on which grid, with how many K splits, and what the split-K arrival counters must
// look like: rgemm_route() is the one statement of it.  Internal header, host only, no HIP calls: a pure function of the call's
// shapes, the CU count and - in the development build - keys kDevRouterGemm64 (40) and kDevRouterGemmSplitCap (45), read here and
// nowhere else.  The launcher (hpc_gemm_bf16xfp32_async), hpc_gemm_bf16xfp32_splits and hpc_gemm_bf16xfp32_plan (what the torch
// op sizes its scratch from) all read it.
#pragma once
#include "hpc_common.h"
#include "hpc_dev.h"

namespace hpc {

constexpr int kRgemmSkinnyMaxM = 256;  // up to here the skinny kernels, above the tile kernel
constexpr int kRgemmMaxSplits = 16;    // the last arriver of every kernel form sums at most 16 partial planes

enum RgemmKernel { kRgemmNone = 0, kRgemmSkinny = 1, kRgemmTile = 2, kRgemmTile64 = 3 };

struct RgemmRoute {
  int code;    // HPC_OK or the refusal (n or k no multiple of 64, operands beyond 32-bit offsets, grid_y > 65535); the rest is set either way
  int kernel;  // kRgemmSkinny: tm rows x 16 weight rows per workgroup; kRgemmTile: 128 tokens x 64 weight rows through LDS;
               // kRgemmTile64 (development key kDevRouterGemm64 = 1): 64 x 64, operands straight from memory; kRgemmNone: m == 0
  int tm;      // skinny: 16 / 32 / 64 tokens per workgroup
  int grid_x, grid_y;  // grid_z is the split count of the call
  int splits;          // what the library picks: 1 without use_splitk
  int max_splits;      // what a caller may pass at most: kRgemmMaxSplits, and every split keeps one 64-k step
  // Split-K arrival counters (zero-once; int32): workgroup (x, y) counts on flag[y * flag_ld + x].
  int flag_rows;  // rows a caller provides.  m <= 256: grid_y.  Above: ceil(m / 64) - that covers the tile kernel, which counts
                  // on its first ceil(m / 128) rows, and the development 64 x 64 kernel, which counts on all of them
  int flag_ld;    // smallest row stride: grid_x
};

// m <= 256 tokens: tm = 16 / 32 / 64 for m <= 16 / 32 / above, a [ceil(m / tm), n / 16] grid.  Above: [ceil(m / 128), n / 64] (the
// development kernel: [ceil(m / 64), n / 64]).  cu_count <= 0 (no device): 256.
// (static: the product and the development library may sit in one process, and each must call its own)
static inline RgemmRoute rgemm_route(int m, int n, int k, int use_splitk, int cu_count) {
  RgemmRoute r{};
  r.splits = 1;
  if (m <= 0 || n <= 0 || k <= 0) {
    r.code = m == 0 && n > 0 && k > 0 ? HPC_OK : HPC_ERR_INVALID;
    return r;
  }
  const int cus = cu_count > 0 ? cu_count : 256;
  const int k_steps = k >> 6;
  r.max_splits = k_steps < kRgemmMaxSplits ? k_steps : kRgemmMaxSplits;
  long tiles;
  if (m <= kRgemmSkinnyMaxM) {
    r.kernel = kRgemmSkinny;
    r.tm = m <= 16 ? 16 : (m <= 32 ? 32 : 64);
    r.grid_x = n / 16;
    r.grid_y = (m + r.tm - 1) / r.tm;
    r.flag_rows = r.grid_y;
    tiles = static_cast<long>(r.grid_y) * r.grid_x;
    // ~one workgroup per CU; every wave keeps at least one 64-k step
    if (use_splitk)
      while (r.splits < 16 && tiles * r.splits < cus && k_steps / (r.splits * 2) >= 4) r.splits *= 2;
  } else {
    const bool tile64 = hpc_dev_tuning_get(kDevRouterGemm64) == 1;
    r.kernel = tile64 ? kRgemmTile64 : kRgemmTile;
    r.grid_x = n / 64;
    r.grid_y = tile64 ? (m + 63) / 64 : (m + 127) / 128;
    r.flag_rows = (m + 63) / 64;
    // The split count is the tile kernel's for either kernel.  Splits until there is ONE workgroup per CU, at most 8 (every split
    // costs the hand-off of its fp32 partials: m = 4096 x n = 256 35.7 us with 4 splits = two workgroups per CU, 28.7 us with 2;
    // m = 1024 29.2 us with 16 splits, 19.9 with 8 - profiles/round5_router_tile_ab.txt); a launch that has between one and two
    // workgroups per CU without splitting is split once more (two resident workgroups per CU overlap each other's load phases).
    tiles = static_cast<long>((m + 127) / 128) * (n / 64);
    // development key kDevRouterGemmSplitCap: cap on the split count above m = 256 (never above the planes the reduce sums)
    const int k45 = hpc_dev_tuning_get(kDevRouterGemmSplitCap);
    const int cap = k45 > 0 ? (k45 < kRgemmMaxSplits ? k45 : kRgemmMaxSplits) : 8;
    if (use_splitk) {
      while (r.splits < cap && tiles * r.splits < cus && k / (r.splits * 2) >= 256) r.splits *= 2;
      if (tiles >= cus && tiles < 2 * cus && r.splits == 1 && k >= 512) r.splits = 2;
    }
  }
  r.flag_ld = r.grid_x;
  // 64-wide tiles and k steps; 32-bit buffer offsets; the grid's y limit
  if ((n & 63) || (k & 63) || static_cast<int64_t>(m) * k * 2 > 0xfffffff0ll || static_cast<int64_t>(n) * k * 2 > 0xfffffff0ll ||
      r.grid_y > 65535)
    r.code = HPC_ERR_UNSUPPORTED;
  return r;
}

}  // namespace hpc
