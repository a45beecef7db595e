// The two MLA absorb matmuls (mla_absorb.hip): on which grid a call runs, or why it is refused - mla_absorb_q_route() and
// mla_unabsorb_o_route() are the one statement of it.  Internal header, host only, no HIP calls: a pure function of the call's
// addresses (null, alignment and the byte ranges they span - never dereferenced), strides and counts.
//
//   absorb_q     out[t, h, :512]  = q_nope[t, h, :128] . w_uk[h, :128, :512]      (the reduction index is the weight's ROW)
//   unabsorb_o   o[t, h * 128 + v] = o_lat[t, h, :512] . w_uv[h, v, :512]          (both operands contiguous along the reduction)
//
// Grid order: workgroup ids go round the 8 XCDs in index order, and every token tile (and, for absorb_q, column slice) of a
// head re-reads that head's weights.  So a head is dealt to ONE XCD: workgroup id -> (xcd = id % 8, k = id / 8), head =
// (k / per_head) * 8 + xcd, piece of the head = k % per_head.  The grid is rounded up to whole rounds of 8 heads; a
// workgroup whose head does not exist returns at once.  A reasoned default (one head's pieces share an L2), not a measured one.
#pragma once
#include <stdint.h>

#include "byte_span.h"
#include "hpc_common.h"
#include "mla_cache.h"

namespace hpc {

constexpr int kMlaAbsorbNope = 128;     // q_nope columns = rows of a head's w_uk = rows of a head's w_uv = the v head
constexpr int kMlaAbsorbLatent = kMlaLatent;  // latent columns
constexpr int kMlaAbsorbMaxHead = 128;
constexpr int kMlaAbsorbThreads = 256;
constexpr int kMlaAbsorbTokTile = 64;   // tokens per workgroup: four blocks of 16, the weight fragments stay in registers
constexpr int kMlaAbsorbTokTileLong = 256;  // absorb_q with more than kMlaAbsorbFill workgroups of 64 tokens: 16 blocks, 4 a wave
constexpr int kMlaAbsorbFill = 512;     // absorb_q workgroups resident at once on 256 CUs: 2 to a CU (183 VGPRs)
constexpr int kMlaAbsorbSlice = 128;    // absorb_q: latent columns per workgroup, one LDS image of [128 d][128 c]
constexpr int kMlaAbsorbSlices = kMlaAbsorbLatent / kMlaAbsorbSlice;
constexpr int kMlaAbsorbXcds = 8;
constexpr int64_t kMlaAbsorbMaxSpan = kMaxSpan;  // bytes a tensor may span (byte_span.h): offsets are 64-bit and stay below 2^61

struct MlaAbsorbCall {  // strides in ELEMENTS of the tensor's dtype
  uintptr_t out, x, w;  // x: q_nope / o_lat
  uintptr_t out_scale;  // unabsorb_o with quant only
  int64_t num_tokens;
  int num_head;
  int64_t x_row_stride, x_head_stride, w_head_stride, w_row_stride, out_row_stride, out_head_stride;
  int quant;
};

struct MlaAbsorbRoute {
  int code;         // HPC_OK or the refusal
  const char* why;  // the refusal in words (null when accepted): one message per rule
  int empty;        // num_tokens == 0: HPC_OK with nothing launched
  int tok_tile, token_tiles, per_head;
  int64_t grid;
  int threads;
};

// Refusals in this order (a call with two faults gets the earlier one); all before the empty call but the null pointers,
// which an empty call may carry.  (static: the product and the development library may sit in one process)
static inline MlaAbsorbRoute mla_absorb_route(const MlaAbsorbCall& c, bool unabsorb) {
  MlaAbsorbRoute r{};
  auto refuse = [&r](int code, const char* why) { return r.code = code, r.why = why, r; };
  const int64_t T = c.num_tokens, H = c.num_head;
  const int64_t x_width = unabsorb ? kMlaAbsorbLatent : kMlaAbsorbNope;
  const int64_t out_width = unabsorb ? kMlaAbsorbNope : kMlaAbsorbLatent;
  if (T < 0) return refuse(HPC_ERR_INVALID, "num_tokens is negative");
  if (H < 1 || H > kMlaAbsorbMaxHead) return refuse(HPC_ERR_UNSUPPORTED, "num_head must be 1 .. 128");
  if (!unabsorb && c.quant) return refuse(HPC_ERR_INVALID, "quant is not an option of absorb_q");
  if (unabsorb && !c.quant && c.out_scale) return refuse(HPC_ERR_INVALID, "output_scale given without quant");
  if ((c.x_row_stride | c.x_head_stride) & 7) return refuse(HPC_ERR_UNSUPPORTED, "an input stride is not a multiple of 8 elements");
  if ((c.w_head_stride | c.w_row_stride) & 7) return refuse(HPC_ERR_UNSUPPORTED, "a weight stride is not a multiple of 8 elements");
  if ((c.x_row_stride < x_width && T > 1) || (c.x_head_stride < x_width && H > 1))
    return refuse(HPC_ERR_UNSUPPORTED, "an input stride is below the width of a head");
  if (c.w_row_stride < kMlaAbsorbLatent || (c.w_head_stride < kMlaAbsorbLatent && H > 1))
    return refuse(HPC_ERR_UNSUPPORTED, "a weight stride is below 512");
  if (c.x_row_stride > kMlaAbsorbMaxSpan / 4 / (T > 0 ? T : 1) || c.x_head_stride > kMlaAbsorbMaxSpan / 1024 ||
      c.out_row_stride > kMlaAbsorbMaxSpan / 4 / (T > 0 ? T : 1) || c.out_head_stride > kMlaAbsorbMaxSpan / 1024 ||
      c.w_head_stride > kMlaAbsorbMaxSpan / 1024 || c.w_row_stride > kMlaAbsorbMaxSpan / 1024)
    return refuse(HPC_ERR_UNSUPPORTED, "a tensor spans more than 2^60 bytes");
  if (unabsorb && c.quant) {  // the (x, x_scale) pair of gemm_blockwise_fp8: contiguous
    if (c.out_row_stride != H * kMlaAbsorbNope) return refuse(HPC_ERR_UNSUPPORTED, "the quantised output must be contiguous");
  } else if (unabsorb) {
    if ((c.out_row_stride & 7) || (c.out_row_stride < H * kMlaAbsorbNope && T > 1))
      return refuse(HPC_ERR_UNSUPPORTED, "the output row stride must be a multiple of 8 and at least num_head * 128");
  } else {
    if ((c.out_row_stride | c.out_head_stride) & 7) return refuse(HPC_ERR_UNSUPPORTED, "an output stride is not a multiple of 8 elements");
    if ((c.out_head_stride < out_width && H > 1) || (c.out_row_stride < (H - 1) * c.out_head_stride + out_width && T > 1))
      return refuse(HPC_ERR_UNSUPPORTED, "the output strides let heads or rows overlap");
  }
  // absorb_q stages 32 KiB of weights per workgroup: once the 64-token tiles outnumber the chip, a workgroup takes 256 tokens
  const bool long_tile = !unabsorb && H * kMlaAbsorbSlices * ((T + kMlaAbsorbTokTile - 1) / kMlaAbsorbTokTile) > kMlaAbsorbFill;
  const int64_t tok_tile = long_tile ? kMlaAbsorbTokTileLong : kMlaAbsorbTokTile;
  const int64_t tiles = (T + tok_tile - 1) / tok_tile;
  const int64_t per_head = tiles * (unabsorb ? 1 : kMlaAbsorbSlices);
  const int64_t grid = (H + kMlaAbsorbXcds - 1) / kMlaAbsorbXcds * kMlaAbsorbXcds * per_head;
  if (grid > 0x7fffffffll) return refuse(HPC_ERR_UNSUPPORTED, "more workgroups than a grid holds");
  if (T == 0) return r.empty = 1, r;
  if (!c.out || !c.x || !c.w || (c.quant && !c.out_scale)) return refuse(HPC_ERR_INVALID, "a null pointer");
  if ((c.out | c.x | c.w) & 15) return refuse(HPC_ERR_UNSUPPORTED, "a base address is not 16-byte aligned");
  if (c.out_scale & 3) return refuse(HPC_ERR_UNSUPPORTED, "output_scale is not 4-byte aligned");
  // an output that shares bytes with an input: other workgroups still read what one overwrites
  const ByteSpan xs = byte_span(c.x, T, c.x_row_stride, H, c.x_head_stride, x_width, 2);
  const ByteSpan ws = byte_span(c.w, 1, 0, H, c.w_head_stride, (kMlaAbsorbNope - 1) * c.w_row_stride + kMlaAbsorbLatent, 2);
  const ByteSpan os = unabsorb ? byte_span(c.out, T, c.out_row_stride, 1, 0, H * kMlaAbsorbNope, c.quant ? 1 : 2)
                           : byte_span(c.out, T, c.out_row_stride, H, c.out_head_stride, out_width, 2);
  if (overlap(os, xs) || overlap(os, ws)) return refuse(HPC_ERR_UNSUPPORTED, "the output overlaps an input");
  if (c.quant) {
    const ByteSpan ss = byte_span(c.out_scale, T, H, 1, 0, H, 4);
    if (overlap(ss, xs) || overlap(ss, ws) || overlap(ss, os)) return refuse(HPC_ERR_UNSUPPORTED, "output_scale overlaps another tensor");
  }
  r.tok_tile = static_cast<int>(tok_tile);
  r.token_tiles = static_cast<int>(tiles);
  r.per_head = static_cast<int>(per_head);
  r.grid = grid;
  r.threads = kMlaAbsorbThreads;
  return r;
}

static inline MlaAbsorbRoute mla_absorb_q_route(const MlaAbsorbCall& c) { return mla_absorb_route(c, false); }
static inline MlaAbsorbRoute mla_unabsorb_o_route(const MlaAbsorbCall& c) { return mla_absorb_route(c, true); }

}  // namespace hpc
