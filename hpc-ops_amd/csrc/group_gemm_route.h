// Which grouped FP8 GEMM kernel runs for a call, in which form and on which grid: ggemm_route() is the one statement of it
// (DESIGN 3.3).  Internal header, host only, no HIP calls: a pure function of the call's shapes and - in the development build -
// the keys that select a kernel, a form or a grid (1, 3, 6, 18, 19, 21, 22, 23, 24, 25, 26, 43, 49, 56; read here and nowhere else).
#pragma once
#include "hpc_common.h"
#include "hpc_dev.h"

namespace hpc {

struct GgemmCall {  // what the call is
  bool has_xs;      // blockwise scales (128 x 128 weight blocks, activation scales per row and k-block), else one scale per group
  bool want_act;    // gate-up GEMM of a fused MoE (n = 2 * inter): the caller would like the activation in the epilogue
  int num_group, m, n, k;
  bool has_scan;  // the exclusive scan of ceil(seqlens / 128) is there (every kernel but the streaming one needs it)
};

struct GgemmRoute {  // what runs
  int code;    // HPC_OK or the refusal; nothing below is set on a refusal
  int kernel;  // 1 streaming (group_gemm_blockwise.hip), 2 tiled 128 x 128 (_tiled.hip), 3 ring 256 x 128 (_tiled256.hip), 4 256 x 256 (_p8.hip)
  int act;     // the activation runs in the epilogue; want_act and act == 0: the caller runs the activation kernel after this route
  int grid_x, grid_y, threads;
  int mt;    // streaming: 1, 2, 3, 4 = 16 / 32 / 48 / 64 tokens per pass with 16 rows per wave; 8 = 64 tokens, 32 rows per wave; 16 / 32 = 64 / 32
             // tokens with 8 waves per workgroup (the numbers of key kDevStreamGemmForm)
  int loop;  // streaming: 0 the re-ordered loop on one K = 128 MFMA per k-block (gemm_blockwise_stream2_kernel), 1 gemm_blockwise_stream_kernel,
             // 2 the re-ordered loop on chains of four K = 32 MFMAs (development)
  int tile_tokens;  // ring: 128, or 64 / 32 (key kDevTiled256Form)
  // 256 x 256: the instantiation (k_tail: per-tensor scales, k % 128 == 64; development: no_dma - timing only -, loop_variant - blockwise,
  // key kDevP8LoopVariant), then what the launcher writes into Args (group_gemm.h)
  int k_tail, no_dma, loop_variant;
  int no_half_tile, nt_single, tail_regs, item_scan_old, ext_rows, item_order;
};

// Refusals are in the order of the launchers this function replaced; num_group, n, k > 0, m > 0 and the scale kind's divisibility of
// n and k are the entries' to check.  avg = rows per group; without the scan every call streams:
//  * n % 256 == 0, k >= 128, avg >= 16: the 256 x 256 kernel, with the activation in its epilogue where the caller wants it and
//    k % 128 == 0 (n % 256 == 0 is inter % 128 == 0);
//  * else n % 128 == 0 and avg > 20: a tiled kernel.  The ring kernel's condition (n % 256 == 0, k >= 128) is the 256 x 256 kernel's,
//    which is asked first: with all keys 0 the ring kernel never runs, the 128 x 128 kernel takes these calls;
//  * else the streaming kernel, its tokens per pass from avg.
constexpr int kGgemmTiledAboveAvg = 20;  // rows per group above which the tiled branch below is asked

// Whether a caller that does not have the scan of ceil(seqlens / 128) anyway (the torch ops of the stand-alone grouped GEMMs) should
// compute it for a call: above kGgemmTiledAboveAvg rows per group.  Below, the call streams - also at 16 ... 20 rows per group, where
// a call WITH the scan (the fused MoE always has it) takes the 256 x 256 kernel.
static inline bool ggemm_scan_wanted(int num_group, int m) { return m / (num_group > 1 ? num_group : 1) > kGgemmTiledAboveAvg; }

// (static: the product and the development library may sit in one process, and each must call its own)
static inline GgemmRoute ggemm_route(const GgemmCall& c) {
  GgemmRoute r{};
  const auto refuse = [](int code) {
    GgemmRoute x{};
    x.code = code;
    return x;
  };
  if (c.num_group <= 0) return refuse(HPC_ERR_INVALID);
  const int avg = c.m / c.num_group;
  // development key kDevGgemmTiledMode: 0 auto, 1 never tiled, 2 always 256 x 128 (when possible), 3 always 128 x 128,
  // 4 always 256 x 256 (when possible)
  const int tiled_mode = hpc_dev_tuning_get(kDevGgemmTiledMode);
  // (up to 64 groups the 256 x 256 kernel finds its work item from one round of lane-parallel loads, above that from one round
  // per 64 groups: tests/test_fuse_moe_blockwise.py::test_group_gemm_blockwise_many_groups, 65 ... 256 groups)
  // From 16 rows per group on (round 5; rounds 2-4: from 192): with the carried tails, the tail body for <= 64 rows and the
  // half-tile body for <= 128 the 256 x 256 kernel overtakes the 256 x 128 ring kernel everywhere and the streaming kernel from
  // ~16 rows per group (fused MoE, E64 / top-8 / H4096 / I11008, us: T = 128 1554-1561 against 1564-1676, T = 256
  // 1590-1596 against 1711-1836, T = 512 1753-1755 against 1876-1978, T = 1024 2069-2102 against 2432-2607; below
  // it loses: T = 64 1552-1563 against 1396-1461 - profiles/round5_moe_kernel_choice.txt).  Development key kDevGgemmP8From192 restores
  // the old threshold.
  const int p8_from = hpc_dev_tuning_get(kDevGgemmP8From192) == 1 ? 192 : 16;
  if (c.has_scan && c.n % 256 == 0 && c.k >= 128 && (tiled_mode == 4 || (tiled_mode == 0 && avg >= p8_from))) {
    r.kernel = 4;
    // a tile = 128 gate rows + the 128 up rows of the same columns: the bf16 gate-up matrix is never written (development key
    // kDevMoeSplitAct = 1: keep the two kernels apart).  The k-tail instantiation with the epilogue exists and no call is routed to it.
    r.act = c.want_act && c.k % 128 == 0 && hpc_dev_tuning_get(kDevMoeSplitAct) != 1;
    if (r.act && static_cast<int64_t>(c.n) * c.k > 0xfffffe00ll) return refuse(HPC_ERR_UNSUPPORTED);  // (the split form would run)
    const long max_tiles = c.m / 256 + c.num_group;  // upper bound of sum_g ceil(len_g / 256)
    const long items = max_tiles * (c.n / 256) + 16;  // + 16: the per-XCD chunks of the full and of the tail tiles round up
    if (items > 0x7fffffffl) return refuse(HPC_ERR_UNSUPPORTED);
    r.grid_x = static_cast<int>(items);
    r.grid_y = 1;
    r.threads = 512;
    r.k_tail = c.k % 128 != 0;
    r.no_half_tile = hpc_dev_tuning_get(kDevP8NoHalfTile);  // development: 1 = full body only, 2 = no tail body
    // a group's ONLY (<= 64-row) token tile streams its weights non-temporally (development key kDevP8TailTemporal = 1: default policy).
    // (A four-stage form of the weight rings with a single-slab token ring - 96 instead of 64 KB of weights in flight per CU -
    // was built, bit-identical, and measured no faster: T = 256 1 515-1 563 against 1 505-1 512 us, profiles/
    // round5_moe_kernel_choice.txt; the stream is not bound by the bytes in flight at that point.  Removed.)
    r.nt_single = hpc_dev_tuning_get(kDevP8TailTemporal) != 1;
    r.tail_regs = hpc_dev_tuning_get(kDevP8TailRegs) == 1;
    r.item_scan_old = hpc_dev_tuning_get(kDevP8ItemScanOld) == 1;
    // a group's short tail (<= 16 rows per full tile it has) rides along with its full tiles instead of running as a tail
    // item (blockwise scales; development key kDevP8NoRideAlong = 1: tail items for every tail, the dispatch of round 5)
    r.ext_rows = hpc_dev_tuning_get(kDevP8NoRideAlong) != 1;
    // tail tiles stay next to their full siblings (order 0).  Order 1 - all full tiles first, tail tiles last, which evens
    // out the end of a launch (the down GEMM of the MoE has ~9.4 items per CU) - measured SLOWER on the same box: gate-up /
    // down GEMM 3493 / 1624 us against 3225 / 1583 us: a tail tile that cannot meet its weight tile in L2 streams it from
    // memory and its DMA pieces land late (development key kDevP8TailsLast = 1 selects order 1; profiles/round5_moe_ggemm_ab.txt)
    r.item_order = hpc_dev_tuning_get(kDevP8TailsLast) == 1;
    // development, blockwise scales: a variant of the k-loop (1 ... 4), else key kDevP8NoDma = 1 without the epilogue
    r.loop_variant = c.has_xs && hpc_dev_tuning_get(kDevP8LoopVariant) > 0 ? hpc_dev_tuning_get(kDevP8LoopVariant) : 0;
    if (r.loop_variant > 4) return refuse(HPC_ERR_INVALID);
    r.no_dma = kHpcDevBuild && c.has_xs && !r.act && !r.loop_variant && hpc_dev_tuning_get(kDevP8NoDma) == 1;
    return r;
  }
  // groups above ~20 tokens: tiled kernels: the 256 x 128 LDS-DMA ring kernel when n allows (one pass over the weights for up to
  // 128 tokens, 100 KB in flight per CU without staging registers; measured on E64 / top-8: T = 128 (16 per group) 1.61 vs
  // 1.50 ms for the streaming form, T = 192 1.63 vs 1.79, T = 256 1.73 vs 1.85, T = 384 1.75 ms), else the 128 x 128
  // register-staged one
  if (c.has_scan && c.n % 128 == 0 && tiled_mode != 1 && (tiled_mode >= 2 || avg > kGgemmTiledAboveAvg)) {
    const long max_tiles = c.m / 128 + c.num_group;  // upper bound of sum_g ceil(len_g / 128)
    if (c.n % 256 || c.k < 128 || tiled_mode == 3) {
      r.kernel = 2;
      r.grid_x = c.n / 128;
      r.grid_y = static_cast<int>(max_tiles);
      r.threads = 256;
      return r;
    }
    // The 32-token-tile form (4-slab ring: three weight slabs in flight) was meant for 40-128 tokens per
    // group; measured it is SLOWER (E64: 3.6 ms vs 2.2 ms at T = 256 .. 768) - its extra token tiles re-read
    // the weight tile through L2 and do a quarter of the MFMA work per slab - so it only runs on request.
    // 64-token tiles (8 x 1 waves of 32 x 64, 42 KB per slab, three slabs in the ring) - also measured SLOWER than
    // the 128-token tile on groups of 24-64 rows (E64: T = 256 2.19 vs 1.73 ms, T = 384 2.25 vs 1.75 ms): on request only
    const int form = hpc_dev_tuning_get(kDevTiled256Form);
    r.kernel = 3;
    r.tile_tokens = form == 2 ? 32 : (form == 3 ? 64 : 128);
    const long items = max_tiles * (c.n / 256) * (128 / r.tile_tokens) + 8;  // + 8: the per-XCD chunks round up
    if (items > 0x7fffffffl) return refuse(HPC_ERR_UNSUPPORTED);
    r.grid_x = static_cast<int>(items);
    r.grid_y = 1;
    r.threads = 512;
    return r;
  }
  // tokens served per pass over the weights, from the average group size (the reference picks its
  // tileM the same way, fuse_moe/entry.cc:525-543); larger groups take several passes
  // measured on E64 / top-8: 16 tokens per pass up to ~10 per group, 32 up to ~22, then 48 (one pass still
  // covers nearly every group of a 32-average batch; 64 per pass is register-bound and slower)
  const int forced = hpc_dev_tuning_get(kDevStreamGemmForm);
  r.kernel = 1;
  r.mt = forced ? forced : (avg <= 10 ? 1 : (avg <= 22 ? 2 : 3));
  r.loop = 1;
  r.grid_y = c.num_group;
  if ((r.mt == 8 || r.mt == 16 || r.mt == 32) && c.n % 128 == 0) {
    r.grid_x = c.n / 128;
    r.threads = r.mt == 8 ? 256 : 512;
    return r;
  }
  r.grid_x = c.n / 64;
  r.threads = 256;
  // development key kDevStreamGemmLoop: 1 = the stage loop of rounds 1-5, 2 = the new loop on K = 32 MFMAs
  const int k56 = hpc_dev_tuning_get(kDevStreamGemmLoop);
  if (r.mt == 1 || r.mt == 2)
    r.loop = k56 == 0 ? 0 : (k56 == 2 ? 2 : 1);
  else if (r.mt != 3 && r.mt != 4)
    r.mt = 2;  // a forced form that does not exist, or 8 / 16 / 32 at n % 128 != 0, runs 32 tokens per pass
  return r;
}

}  // namespace hpc
