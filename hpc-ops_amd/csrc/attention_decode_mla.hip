// MLA decode attention (weight-absorbed form) over the paged latent KV cache, bf16, gfx950.
//
//   z_j = scale * sum_{d < 576} q[row, d] * c[j, d]      out[row, :512] = sum_j softmax(z)_j * c[j, :512]
//
// One latent row of 576 bf16 per token is K (all 576 columns) and V (the first 512) of every head, so a KV tile is gathered
// through the page table ONCE into one LDS image and read twice: by rows (ds_read_b128) as the A operand of S^T = C Q^T, and
// through the transposing read (ds_read_b64_tr_b16) as the A operand of O^T = C^T P^T.  Computing S^T puts a q row on a lane
// (column l & 15) and four tokens in its accumulator registers, which after exp2 and a pack to bf16 ARE the B operand of the
// second product: the eight k-slots of lane group g hold tokens 16 tb + 4 g + 0..3 of two token blocks, and the transposing read
// fetches exactly those rows for the other operand, so the token permutation is the same on both sides and no lane moves.
//
// Workgroup = 256 threads = (request, row tile, piece).  Rows of a request are r = s * num_head + h.
//   wide   (rows > 16): a tile of 64 rows, wave w owns rows 16 w .. 16 w + 15 and all 64 tokens of every KV tile; a wave whose
//          rows do not exist (a 48-row tile) only helps to gather.
//   narrow (rows == 16: 16 heads at mtp 0): the four waves own the SAME 16 rows and wave w takes tokens 16 w .. 16 w + 15 of
//          every KV tile (the upper half of its k-slots is zero); the four (max, sum, O) states are merged through LDS at the end.
// KV tile: 64 tokens x 1,152 B in rows of kRowBytes = 1,184 B (296 dwords = 8 * 37: the 16 x 16-byte row read and the 8 rows x
// 32 bytes a 32-lane half takes in a transposing read both touch every bank once), two images = 148 KiB.  The next tile's rows
// are loaded into registers (18 x 16 B per thread) before the current tile is computed and stored to the other image after it;
// their page ids are looked up one tile ahead, so the row loads never wait for a dependent load.
// Rows of tokens at or past the piece's end are written as zeros, never loaded: 0 x NaN is NaN, and the entries of block_ids
// past a request's pages are never dereferenced.  Masking is by score.
//
// Split KV: piece p of request b covers tokens [p * len, min(L_b, (p + 1) * len)), len = ceil(L_b / splits) rounded up to 64,
// computed on the DEVICE from num_seq_kvcache (nothing on the host depends on the lengths).  A piece that starts at or past L_b
// writes nothing, and the merge kernel computes the same piece count and never reads it.  A piece stores its running maximum,
// its sum and its UNNORMALISED fp32 output; the merge sums exp2(m_p - M) * O_p in piece order and divides once (no float
// atomics, bit-identical from call to call; exact where the softmax is uniform and the length a power of two).
//
// FP8 latent cache (kFp8, hpc_attention_decode_mla_fp8_async): the row of mla_fp8_format.h - 512 e4m3 codes, four fp32 scales,
// the 64 RoPE columns in bf16, 656 B.  Only the gather differs: thread (rr, sub) stages per row the four 16-byte code chunks
// sub + 8 i (chunk sub + 8 i lies in scale group i), the scale quad and RoPE chunk sub - 12 quads where the bf16 form stages
// 18 - and the commit turns each code chunk into 16 bf16 (dequant16 of mla_fp8_format.h, which mla_gather.hip uses too: cvt to
// fp32, ONE fp32 multiply by the group's scale, RNE pack) stored as two 16-byte quads at element column 16 (sub + 8 i).  The
// LDS image is byte for byte what the bf16 form builds from the dequantised cache, and everything behind it is the same code:
// the two ops agree bit for bit on such a pair of caches.  The row's dimensions and the host rule for a cache: mla_cache.h.
#include <type_traits>

#include "attention_decode_mla_route.h"
#include "mla_fp8_format.h"
#include "hpc_amd.h"
#include "hpc_common.h"
#include "mla_indexer_dev.h"

namespace hpc {
namespace mla {

constexpr int kThreads = 256;
constexpr int kRowBytes = 1184;               // LDS pitch of a latent row (1,152 B of data)
constexpr int kBufBytes = kMlaKvTile * kRowBytes;
constexpr int kLds = 2 * kBufBytes;           // 151,552 B
constexpr int kKSteps = kMlaRow / 32;         // 18 MFMA k-steps over the 576 columns
constexpr int kColBlocks = kMlaLatent / 16;   // 32 output column blocks
constexpr float kLn2 = 0.693147180559945309f;
constexpr float kLog2e = 1.442695040888963407f;
static_assert(4 * 16 * kMlaLatent * 4 + 4 * 16 * 2 * 4 <= kLds, "the narrow form's merge fits the tile images");

struct Args {
  const uint8_t* q;
  const uint8_t* ckv;
  const int* block_ids;
  const int* num_seq;
  uint16_t* out;
  float* lse;     // may be null
  float* ws_o;    // [splits, total_rows, 512]
  float* ws_ml;   // [splits, total_rows, 2]
  int64_t block_stride_bytes, token_stride_bytes, total_rows;
  int num_head, num_seq_q, rows, row_tiles, splits, page_shift, max_blocks, new_kv_included;
  float scale_log2;  // softmax_scale * log2(e)
};

// The token-sparse form adds the lists: row b * num_seq_q + s of `indices` names the token positions q row (b, s) attends to
// Ragged (a prefill chunk, q_index given): unit r is row r of the chunk, its request and vis are the writers' row rule
// (mla_indexer_dev.h::row_sees over num_seq = num_seqlen_per_req), num_seq_q is 1 and block_ids has num_req rows.
struct SparseArgs : Args {
  const int* indices;  // [num_batch * num_seq_q, topk]
  const int* q_index;  // null: a decode step.  Given: [num_req + 1] of a ragged chunk
  int topk, plen, num_blocks, num_req;  // plen: list slots per piece, a multiple of kMlaKvTile (a host value, as topk is)
};
template <bool kSparse>
using ArgsOf = std::conditional_t<kSparse, SparseArgs, Args>;

// tokens of request b including the new ones, never beyond the page table's reach
__device__ __forceinline__ int request_len(const Args& a, int b) {
  const int64_t cap = static_cast<int64_t>(a.max_blocks) << a.page_shift;
  int64_t len = static_cast<int64_t>(a.num_seq[b]) + (a.new_kv_included ? 0 : a.num_seq_q);
  len = len < 0 ? 0 : (len > cap ? cap : len);
  return static_cast<int>(len);
}
__device__ __forceinline__ int piece_len(int len, int splits) {
  return ((len + splits - 1) / splits + kMlaKvTile - 1) & ~(kMlaKvTile - 1);
}
// positions a list entry of q row (b, s) may name: [0, vis), vis = L_b - num_seq_q + s + 1 from the UNCLAMPED length, never
// beyond the page table's reach (so idx < vis implies idx >> page_shift < max_blocks).  The decode-step row rule of
// mla_indexer_dev.h (step_len, step_sees) with the reach in 64 bits: calling those moves this kernel's assembly, so the rule
// stands here a second time
__device__ __forceinline__ int sparse_vis(const SparseArgs& a, int b, int s) {
  const int64_t cap = static_cast<int64_t>(a.max_blocks) << a.page_shift;
  int64_t vis = static_cast<int64_t>(a.num_seq[b]) + (a.new_kv_included ? 0 : a.num_seq_q) - a.num_seq_q + s + 1;
  vis = vis < 0 ? 0 : (vis > cap ? cap : vis);
  return static_cast<int>(vis);
}

// one result quad: the final bf16 output (one piece) or the piece's unnormalised fp32 partial
// kZeroRow (the sparse form): a row that saw no token (l == 0, every v 0) is written as zeros, not as 0 x inf
template <bool kZeroRow>
__device__ __forceinline__ void emit4(const Args& a, int piece, int64_t grow, int col, f32x4 v, float l) {
  if (a.splits == 1) {
    const float inv = kZeroRow && !(l > 0.f) ? 0.f : 1.0f / l;
    *reinterpret_cast<u32x2*>(a.out + grow * kMlaLatent + col) =
        u32x2{pack_bf16x2(v[0] * inv, v[1] * inv), pack_bf16x2(v[2] * inv, v[3] * inv)};
  } else {
    *reinterpret_cast<f32x4*>(a.ws_o + (piece * a.total_rows + grow) * kMlaLatent + col) = v;
  }
}
__device__ __forceinline__ void emit_ml(const Args& a, int piece, int64_t grow, float m, float l) {
  if (a.splits == 1) {
    if (a.lse) a.lse[grow] = (m + __builtin_log2f(l)) * kLn2;
  } else {
    *reinterpret_cast<f32x2*>(a.ws_ml + (piece * a.total_rows + grow) * 2) = f32x2{m, l};
  }
}

// kSparse: the token loop runs over the slots [piece * plen, min(topk, (piece + 1) * plen)) of the q row's list instead of a
// token range, and the workgroup's rows are the heads of ONE q row (b, s) - lists differ per s.  Thread (rr, sub) fetches the
// rows named by slots rr and rr + 32 of a tile.  A slot is valid when 0 <= idx < vis(b, s) and its page id lies in
// [0, num_blocks); an invalid slot (padding, a slot past topk) writes zeros into the image, is never loaded and is masked by
// score through a byte per slot beside the image.  The list entries are loaded two tiles ahead and the page ids one tile
// ahead, so neither the page lookup nor the row loads wait for a dependent load.  A tile without a valid slot issues no cache
// load and is not computed.  Everything behind the image is the dense code.
template <bool kNarrow, bool kFp8, bool kSparse>
__global__ __launch_bounds__(kThreads) void attention_decode_mla_kernel(const ArgsOf<kSparse> a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_mem[kLds];
  __shared__ __attribute__((aligned(16))) uint8_t s_valid[kSparse ? 2 * kMlaKvTile : 1];  // sparse: slot validity per image
  constexpr int kTB = kNarrow ? 1 : 4;  // 16-token blocks a wave takes of a tile
  constexpr int kKS = kNarrow ? 1 : 2;  // 32-token k-steps of the second product

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  int id = blockIdx.x;
  const int piece = id % a.splits;
  id /= a.splits;
  // unit: the request (dense) or the q row b * num_seq_q + s (sparse) whose a.rows rows this workgroup's tile is cut from
  const int tile = id % a.row_tiles, unit = id / a.row_tiles;
  int b = kSparse ? unit / a.num_seq_q : unit;

  int p0, p1, vis = 0;  // dense: the piece's tokens; sparse: the piece's list slots and the positions they may name
  [[maybe_unused]] int len = 0;
  if constexpr (kSparse) {
    p0 = piece * a.plen;  // < topk: the host launches no piece past the list
    p1 = p0 + a.plen < a.topk ? p0 + a.plen : a.topk;
    if (a.q_index) {  // a ragged chunk: the row rule gives the request (one of the call's) and what the row sees
      const hpc::mla_indexer::RowSees at =
          hpc::mla_indexer::row_sees(a.q_index, a.num_seq, a.num_req, unit, a.max_blocks << a.page_shift);
      b = at.req;
      vis = at.vis;
    } else {
      vis = sparse_vis(a, b, unit - b * a.num_seq_q);
    }
  } else {
    len = request_len(a, b);
    const int plen = piece_len(len, a.splits);
    p0 = piece * plen;
    if (p0 >= len) return;  // an empty piece writes nothing; the merge does not read it
    p1 = p0 + plen < len ? p0 + plen : len;
  }
  const int n_tiles = (p1 - p0 + kMlaKvTile - 1) / kMlaKvTile;

  const int rb = kNarrow ? 0 : tile * kMlaRowTile + 16 * wv;  // first q row of this wave
  const bool active = rb < a.rows;                           // rows is a multiple of 16: all 16 rows exist or none
  const int64_t grow = static_cast<int64_t>(unit) * a.rows + rb + c16;
  // causal limit of this lane's q row, cut at the piece's end (sparse: validity says it, slot by slot)
  [[maybe_unused]] int lim = 0;
  if constexpr (!kSparse) {
    lim = len - a.num_seq_q + (rb + c16) / a.num_head + 1;
    lim = lim < p1 ? lim : p1;
  }

  bf16x8 qf[kKSteps];
  if (active) {
    const uint8_t* qrow = a.q + grow * (kMlaRow * 2) + g * 16;
#pragma unroll
    for (int ks = 0; ks < kKSteps; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + ks * 64);
  }

  // ---- gather: thread (rr, sub) takes chunks sub + 8 i of rows rr and rr + 32 ----
  const int rr = tid >> 3, sub = tid & 7;
  const int* pages = a.block_ids + static_cast<int64_t>(b) * a.max_blocks;
  constexpr int kStage = kFp8 ? 6 : 9;  // 16-byte quads staged per row: 4 code chunks + the scales + 1 RoPE chunk, or 9 bf16 chunks
  u32x4 stg[2][kStage];
  // the page ids of the rows this thread loads next, looked up one tile ahead: the row loads do not wait for the page table
  int page[2];
  // sparse: the positions of the rows this thread loads next (-1: nothing to load), the list entries one tile further, and
  // whether the rows staged in stg are real
  [[maybe_unused]] int pos[2] = {-1, -1}, nidx[2] = {-1, -1};
  [[maybe_unused]] bool real[2] = {false, false};
  [[maybe_unused]] const int* list = nullptr;
  if constexpr (kSparse) list = a.indices + static_cast<int64_t>(unit) * a.topk;
  auto load_idx = [&](int t0) {  // sparse only: slots at or past the piece's end read nothing and are invalid
    if constexpr (kSparse) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int slot = t0 + rr + 32 * p;
        nidx[p] = slot < p1 ? list[slot] : -1;
      }
    }
  };
  auto lookup = [&](int t0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if constexpr (kSparse) {
        const int i = nidx[p];  // of tile t0, loaded a tile ago
        const bool ok = static_cast<unsigned>(i) < static_cast<unsigned>(vis);  // vis <= max_blocks << page_shift
        pos[p] = ok ? i : -1;
        page[p] = ok ? pages[i >> a.page_shift] : -1;  // checked against num_blocks where it is used, a tile later
      } else {
        const int tok = t0 + rr + 32 * p;
        page[p] = tok < p1 ? pages[tok >> a.page_shift] : 0;
      }
    }
    load_idx(t0 + kMlaKvTile);
  };
  auto gather_issue = [&](int t0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      int tok = t0 + rr + 32 * p;
      bool load = tok < p1;
      if constexpr (kSparse) {
        tok = pos[p];
        load = tok >= 0 && static_cast<unsigned>(page[p]) < static_cast<unsigned>(a.num_blocks);
        real[p] = load;
      }
      if (load) {
        const uint8_t* src = a.ckv + static_cast<int64_t>(page[p]) * a.block_stride_bytes +
                             static_cast<int64_t>(tok & ((1 << a.page_shift) - 1)) * a.token_stride_bytes + sub * 16;
        if constexpr (kFp8) {
#pragma unroll
          for (int i = 0; i < 4; ++i) stg[p][i] = ld16(src + kMlaFp8CodesAt + i * 128);
          stg[p][4] = ld16(src - sub * 16 + kMlaFp8ScalesAt);  // the same quad for the eight threads of a row
          stg[p][5] = ld16(src + kMlaFp8RopeAt);
        } else {
#pragma unroll
          for (int i = 0; i < 9; ++i) stg[p][i] = ld16(src + i * 128);
        }
      } else {  // codes 0 x scale 0: zeros in the image, like the bf16 form's
#pragma unroll
        for (int i = 0; i < kStage; ++i) stg[p][i] = u32x4{0, 0, 0, 0};
      }
    }
    lookup(t0 + kMlaKvTile);
  };
  auto gather_commit = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      uint8_t* dst = s_mem + buf * kBufBytes + (rr + 32 * p) * kRowBytes + sub * 16;
      if constexpr (kFp8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // chunk sub + 8 i: columns 16 (sub + 8 i) .. + 15, all in scale group i
          u32x4 lo, hi;
          dequant16(stg[p][i], __uint_as_float(stg[p][4][i]), lo, hi);
          *reinterpret_cast<u32x4*>(dst + sub * 16 + i * 256) = lo;
          *reinterpret_cast<u32x4*>(dst + sub * 16 + i * 256 + 16) = hi;
        }
        *reinterpret_cast<u32x4*>(dst + kMlaLatent * 2) = stg[p][5];
      } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) *reinterpret_cast<u32x4*>(dst + i * 128) = stg[p][i];
      }
      if constexpr (kSparse) {
        if (sub == 0) s_valid[buf * kMlaKvTile + rr + 32 * p] = real[p] ? 1 : 0;
      }
    }
  };

  f32x4 acc[kColBlocks];
#pragma unroll
  for (int cb = 0; cb < kColBlocks; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;  // running maximum (log2 units) and this lane's share of the sum

  // transposing-read address of this lane inside a 16-token block: row 4 g + (c16 >> 2), columns 4 (c16 & 3) ..
  const int tr_off = (4 * g + (c16 >> 2)) * kRowBytes + (c16 & 3) * 8;
  const int rd_off = c16 * kRowBytes + g * 16;

  load_idx(p0);
  lookup(p0);
  gather_issue(p0);
  gather_commit(0);
  __syncthreads();

  for (int it = 0; it < n_tiles; ++it) {
    const int t0 = p0 + it * kMlaKvTile;
    const int cur = it & 1;
    const bool more = it + 1 < n_tiles;
    if (more) gather_issue(t0 + kMlaKvTile);
    // sparse: a wave whose slots of this tile are all invalid (padding) has nothing to add - every score would be -inf, which
    // leaves (m, l, O) as they are.  Wave-uniform, read from the validity bytes: all 64 (wide) or the wave's own 16 (narrow)
    bool any_seen = true;
    if constexpr (kSparse) {
      const uint32_t* vb = reinterpret_cast<const uint32_t*>(s_valid) + cur * (kMlaKvTile / 4);
      any_seen = __any((kNarrow ? vb[4 * wv + (lane & 3)] : vb[lane & 15]) != 0);
    }
    if (active && any_seen) {
      const uint8_t* img = s_mem + cur * kBufBytes;
      // ---- S^T = C Q^T ----
      f32x4 s[kTB];
#pragma unroll
      for (int t = 0; t < kTB; ++t) {
        const int tb = kNarrow ? wv : t;
        s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < kKSteps; ++ks) {
          const bf16x8 c = *reinterpret_cast<const bf16x8*>(img + tb * 16 * kRowBytes + rd_off + ks * 64);
          s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c, qf[ks], s[t], 0, 0, 0);
        }
      }
      // ---- online softmax, masked by score ----
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < kTB; ++t) {
        const int tb = kNarrow ? wv : t;
        [[maybe_unused]] uint32_t vw = 0;  // sparse: the validity bytes of this lane's four slots
        if constexpr (kSparse) vw = *reinterpret_cast<const uint32_t*>(s_valid + cur * kMlaKvTile + 16 * tb + 4 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          bool seen;
          if constexpr (kSparse) {
            seen = (vw >> (8 * i)) & 1;
          } else {
            const int tok = t0 + 16 * tb + 4 * g + i;
            seen = tok < lim;
          }
          s[t][i] = seen ? s[t][i] * a.scale_log2 : -INFINITY;
          mx = fmaxf(mx, s[t][i]);
        }
      }
      mx = row4_max(mx);
      const float m_new = fmaxf(m, mx);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m - m_use);
      m = m_new;
      float psum = 0.f;
#pragma unroll
      for (int t = 0; t < kTB; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[t][i] = __builtin_amdgcn_exp2f(s[t][i] - m_use);
          psum += s[t][i];
        }
      l = l * alpha + psum;
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int cb = 0; cb < kColBlocks; ++cb) acc[cb] *= alpha;
      }
      // ---- O^T += C^T P^T ----
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) {
        u32x4 pw;
        pw[0] = pack_bf16x2(s[kNarrow ? 0 : 2 * ks][0], s[kNarrow ? 0 : 2 * ks][1]);
        pw[1] = pack_bf16x2(s[kNarrow ? 0 : 2 * ks][2], s[kNarrow ? 0 : 2 * ks][3]);
        pw[2] = kNarrow ? 0u : pack_bf16x2(s[kNarrow ? 0 : 2 * ks + 1][0], s[kNarrow ? 0 : 2 * ks + 1][1]);
        pw[3] = kNarrow ? 0u : pack_bf16x2(s[kNarrow ? 0 : 2 * ks + 1][2], s[kNarrow ? 0 : 2 * ks + 1][3]);
        const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
        const int tb0 = kNarrow ? wv : 2 * ks;
#pragma unroll
        for (int cb = 0; cb < kColBlocks; ++cb) {
          u32x4 vw = u32x4{0, 0, 0, 0};
          const uint8_t* p_lo = img + tb0 * 16 * kRowBytes + tr_off + cb * 32;
          const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              reinterpret_cast<lds_v4i16*>(static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_u8*)p_lo))));
          const u32x2 lo2 = __builtin_bit_cast(u32x2, lo);
          vw[0] = lo2[0], vw[1] = lo2[1];
          if constexpr (!kNarrow) {
            const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_v4i16*>(
                static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_u8*)(p_lo + 16 * kRowBytes)))));
            const u32x2 hi2 = __builtin_bit_cast(u32x2, hi);
            vw[2] = hi2[0], vw[3] = hi2[1];
          }
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vw), pf, acc[cb], 0, 0, 0);
        }
      }
    }
    if (more) gather_commit(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: lane (c16, g) holds columns 16 cb + 4 g + 0..3 of q row c16 ----
  if constexpr (!kNarrow) {
    if (!active) return;
    l = row4_sum(l);
#pragma unroll
    for (int cb = 0; cb < kColBlocks; ++cb) emit4<kSparse>(a, piece, grow, 16 * cb + 4 * g, acc[cb], l);
    if (g == 0) emit_ml(a, piece, grow, m, l);
  } else {
    // the four waves' states of the same 16 rows: scale to the common maximum, sum in wave order
    float* s_f = reinterpret_cast<float*>(s_mem);      // [4][16][512]
    float* s_ml = s_f + 4 * 16 * kMlaLatent;           // [4][16][2]
    l = row4_sum(l);
    if (g == 0) {
      s_ml[(wv * 16 + c16) * 2] = m;
      s_ml[(wv * 16 + c16) * 2 + 1] = l;
    }
    __syncthreads();
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) mm = fmaxf(mm, s_ml[(w * 16 + c16) * 2]);
    const float f = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mm);
#pragma unroll
    for (int cb = 0; cb < kColBlocks; ++cb)
      *reinterpret_cast<f32x4*>(s_f + (wv * 16 + c16) * kMlaLatent + 16 * cb + 4 * g) = acc[cb] * f;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int idx = tid + kThreads * e, row = idx >> 7, col = (idx & 127) * 4;
      float mr = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w) mr = fmaxf(mr, s_ml[(w * 16 + row) * 2]);
      float lt = 0.f;
      f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float mw = s_ml[(w * 16 + row) * 2], lw = s_ml[(w * 16 + row) * 2 + 1];
        lt += (mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - mr)) * lw;
        sum += *reinterpret_cast<const f32x4*>(s_f + (w * 16 + row) * kMlaLatent + col);
      }
      const int64_t gr = static_cast<int64_t>(unit) * a.rows + row;
      emit4<kSparse>(a, piece, gr, col, sum, lt);
      if (col == 0) emit_ml(a, piece, gr, mr, lt);
    }
  }
}

// Sums the pieces of one output row in piece order.  Pieces at or past the request's end were never written and are not read;
// a piece in which this row saw no token (its sum is 0) is skipped.
// kSparse: every launched piece wrote (the host launches none past the list), and a row whose pieces all saw no token is
// written as zeros with lse = -inf.
template <bool kSparse>
__global__ __launch_bounds__(128) void attention_decode_mla_merge_kernel(const ArgsOf<kSparse> a) {
  const int64_t grow = blockIdx.x;
  int np = a.splits;
  if constexpr (!kSparse) {
    const int b = static_cast<int>(grow / a.rows);
    const int len = request_len(a, b);
    if (len == 0) return;
    const int plen = piece_len(len, a.splits);
    np = (len + plen - 1) / plen;  // <= splits
  }
  const int col = threadIdx.x * 4;
  float mm = -INFINITY;
  for (int p = 0; p < np; ++p) {
    const f32x2 ml = *reinterpret_cast<const f32x2*>(a.ws_ml + (p * a.total_rows + grow) * 2);
    if (ml[1] > 0.f) mm = fmaxf(mm, ml[0]);
  }
  float lt = 0.f;
  f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < np; ++p) {
    const f32x2 ml = *reinterpret_cast<const f32x2*>(a.ws_ml + (p * a.total_rows + grow) * 2);
    if (ml[1] > 0.f) {
      const float f = __builtin_amdgcn_exp2f(ml[0] - mm);
      lt += f * ml[1];
      sum += *reinterpret_cast<const f32x4*>(a.ws_o + (p * a.total_rows + grow) * kMlaLatent + col) * f;
    }
  }
  const float inv = kSparse && !(lt > 0.f) ? 0.f : 1.0f / lt;
  *reinterpret_cast<u32x2*>(a.out + grow * kMlaLatent + col) =
      u32x2{pack_bf16x2(sum[0] * inv, sum[1] * inv), pack_bf16x2(sum[2] * inv, sum[3] * inv)};
  if (a.lse && threadIdx.x == 0) a.lse[grow] = (mm + __builtin_log2f(lt)) * kLn2;
}

}  // namespace mla
}  // namespace hpc

// ---- host side: dense and token-sparse share the route (mla_route() of attention_decode_mla_route.h), the plan sequence and
// the launcher; the form is the template argument kSparse, and the list's checks and members stand beside the shared ones -------
namespace {
using hpc::MlaRows;

// Both plan entries: refusals first, on the host alone; only a call that leaves both the split count and the CU count open asks
// the device.  num_cu <= 0: the current device's (256 without a device).
hpc::MlaRoute mla_plan_route(int num_batch, int num_seq_q, int num_head, bool sparse, int topk, int splits_wanted, int num_cu) {
  hpc::MlaRoute r = hpc::mla_route(num_batch, num_seq_q, num_head, sparse, topk, splits_wanted, num_cu > 0 ? num_cu : 256);
  if (r.code == HPC_OK && num_cu <= 0 && splits_wanted == 0 && num_batch > 0)
    r = hpc::mla_route(num_batch, num_seq_q, num_head, sparse, topk, 0, hpc::current_cu_count());
  return r;
}

// the arguments of the six launchers, in the sparse entries' order; dense: indices null, topk and num_blocks 0
struct MlaDecodeCall {
  void* out;
  float* lse;
  const void* q;
  const void* ckv;
  const int* block_ids;
  MlaRows rows;  // a decode step or, the ragged entries, a prefill chunk (mla_indexer_route.h)
  const int* indices;
  int num_head, topk, block_size, max_blocks, num_blocks;
  int64_t ckv_block_stride, ckv_token_stride;  // in the kind's units: bf16 elements or FP8 bytes
  float softmax_scale;
  int splits;
  void* workspace;
  int64_t workspace_bytes;
  hipStream_t stream;
};

// All six launchers: the checks, the route and the launches.  What a valid cache is - its page size, its strides in the kind's
// units and its alignment - is mla_cache_check() of mla_cache.h.
template <bool kFp8, bool kSparse>
int mla_decode_launch(const MlaDecodeCall& c) {
  using namespace hpc::mla;
  constexpr hpc::MlaCacheKind kind = kFp8 ? hpc::kMlaCacheFp8 : hpc::kMlaCacheBf16;
  // A ragged chunk is routed as num_rows requests of one q row each (hpc_attention_decode_mla_sparse_plan sizes its scratch so);
  // without requests every row is a row of no request and the call is an empty one
  const MlaRows& rows = c.rows;
  if (rows.ragged && (!rows.q_index || rows.num_req < 0)) return HPC_ERR_INVALID;
  const int num_batch = !rows.ragged ? rows.num_batch : rows.num_req == 0 && rows.num_rows > 0 ? 0 : rows.num_rows;
  if (!c.out || !c.q || !c.ckv || !c.block_ids || !rows.lens || (kSparse && !c.indices)) return HPC_ERR_INVALID;
  // the cache's invalid argument (a negative block stride) is refused here with the others, what it does not support behind
  // the shapes: a call with two faults keeps the code of the earlier check
  const hpc::MlaCacheCheck cache =
      hpc::mla_cache_check(kind, reinterpret_cast<uintptr_t>(c.ckv), c.block_size, c.ckv_block_stride, c.ckv_token_stride);
  if (c.splits < 0 || c.max_blocks < 0 || (kSparse && c.num_blocks < 0) || cache.code == HPC_ERR_INVALID)
    return HPC_ERR_INVALID;
  // the split count is the caller's, or with 0 the route's for this device; shapes are refused before the device is asked
  const hpc::MlaRoute shape =
      hpc::mla_route(num_batch, rows.num_seq_q, c.num_head, kSparse, c.topk, c.splits > 0 ? c.splits : 1, 256);
  if (shape.code != HPC_OK) return shape.code;
  if (cache.code != HPC_OK) return cache.code;
  if (static_cast<int64_t>(c.max_blocks) * c.block_size > (1ll << 30)) return HPC_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(c.q) & 15) return HPC_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(c.out) & 7) || (reinterpret_cast<uintptr_t>(c.lse) & 3) ||
      (kSparse && (reinterpret_cast<uintptr_t>(c.indices) & 3)))
    return HPC_ERR_UNSUPPORTED;
  if (num_batch == 0) return HPC_OK;
  if (c.max_blocks == 0) return HPC_ERR_INVALID;
  if (rows.ragged && rows.num_req == INT32_MAX) return HPC_ERR_INVALID;  // num_req + 1 entries of q_index
  const hpc::MlaRoute r =
      c.splits > 0 ? shape : hpc::mla_route(num_batch, rows.num_seq_q, c.num_head, kSparse, c.topk, 0, hpc::current_cu_count());
  if (r.code != HPC_OK) return r.code;
  if (r.splits > 1) {
    if (!c.workspace || c.workspace_bytes < r.workspace_bytes) return HPC_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(c.workspace) & 15) return HPC_ERR_UNSUPPORTED;
  }
  ArgsOf<kSparse> a;
  a.q = static_cast<const uint8_t*>(c.q);
  a.ckv = static_cast<const uint8_t*>(c.ckv);
  a.block_ids = c.block_ids;
  a.num_seq = rows.lens;
  a.out = static_cast<uint16_t*>(c.out);
  a.lse = c.lse;
  a.ws_o = static_cast<float*>(c.workspace);
  a.ws_ml = reinterpret_cast<float*>(static_cast<uint8_t*>(c.workspace) + r.ml_offset);
  a.block_stride_bytes = c.ckv_block_stride * kind.unit;
  a.token_stride_bytes = c.ckv_token_stride * kind.unit;
  a.total_rows = r.total_rows;
  a.num_head = c.num_head;
  a.num_seq_q = rows.num_seq_q;
  a.rows = r.rows;
  a.row_tiles = r.row_tiles;
  a.splits = r.splits;
  a.page_shift = hpc::mla_page_shift(c.block_size);
  a.max_blocks = c.max_blocks;
  a.new_kv_included = rows.new_kv_included ? 1 : 0;
  a.scale_log2 = c.softmax_scale * kLog2e;
  if constexpr (kSparse) {
    a.indices = c.indices;
    a.q_index = rows.q_index;
    a.num_req = rows.num_req;
    a.topk = c.topk;
    a.plen = r.plen;
    a.num_blocks = c.num_blocks;
  }
  if (r.narrow)
    attention_decode_mla_kernel<true, kFp8, kSparse><<<dim3(r.grid), kThreads, 0, c.stream>>>(a);
  else
    attention_decode_mla_kernel<false, kFp8, kSparse><<<dim3(r.grid), kThreads, 0, c.stream>>>(a);
  HPC_CHECK_LAUNCH();
  if (r.splits > 1) {
    attention_decode_mla_merge_kernel<kSparse><<<dim3(r.merge_grid), 128, 0, c.stream>>>(a);
    HPC_CHECK_LAUNCH();
  }
  return HPC_OK;
}
}  // namespace

// What a call of hpc_attention_decode_mla_{bf16,fp8}_async with this `splits_wanted` runs with and needs
extern "C" int hpc_attention_decode_mla_plan(int num_batch, int num_seq_q, int num_head, int splits_wanted, int num_cu,
                                             int* splits, int* max_splits, int64_t* workspace_bytes) {
  if (!splits || !max_splits || !workspace_bytes) return HPC_ERR_INVALID;
  const hpc::MlaRoute r = mla_plan_route(num_batch, num_seq_q, num_head, false, 0, splits_wanted, num_cu);
  *splits = r.splits, *max_splits = r.max_splits, *workspace_bytes = r.workspace_bytes;
  return r.code;
}

extern "C" int hpc_attention_decode_mla_bf16_async(void* out_ptr, float* lse_ptr, const void* q_ptr, const void* ckv_ptr,
                                                   const int* block_ids_ptr, const int* num_seq_kvcache_ptr, int num_batch,
                                                   int num_seq_q, int num_head, int block_size, int max_blocks,
                                                   int64_t ckv_block_stride, int64_t ckv_token_stride, float softmax_scale,
                                                   int new_kv_included, int splits, void* workspace_ptr,
                                                   int64_t workspace_bytes, hipStream_t stream) {
  return mla_decode_launch<false, false>({out_ptr, lse_ptr, q_ptr, ckv_ptr, block_ids_ptr,
                                          MlaRows::step(num_seq_kvcache_ptr, num_batch, num_seq_q, new_kv_included), nullptr, num_head,
                                          0, block_size, max_blocks, 0, ckv_block_stride, ckv_token_stride, softmax_scale, splits,
                                          workspace_ptr, workspace_bytes, stream});
}

// the same over the FP8 latent cache (mla_fp8_format.h); the cache's strides in bytes
extern "C" int hpc_attention_decode_mla_fp8_async(void* out_ptr, float* lse_ptr, const void* q_ptr, const void* ckv_ptr,
                                                  const int* block_ids_ptr, const int* num_seq_kvcache_ptr, int num_batch,
                                                  int num_seq_q, int num_head, int block_size, int max_blocks,
                                                  int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes,
                                                  float softmax_scale, int new_kv_included, int splits, void* workspace_ptr,
                                                  int64_t workspace_bytes, hipStream_t stream) {
  return mla_decode_launch<true, false>({out_ptr, lse_ptr, q_ptr, ckv_ptr, block_ids_ptr,
                                         MlaRows::step(num_seq_kvcache_ptr, num_batch, num_seq_q, new_kv_included), nullptr, num_head,
                                         0, block_size, max_blocks, 0, ckv_block_stride_bytes, ckv_token_stride_bytes, softmax_scale,
                                         splits, workspace_ptr, workspace_bytes, stream});
}

// ---- the token-sparse form: each q row attends to the tokens its list names --------------------------------------------------
// What a call of hpc_attention_decode_mla_sparse_{bf16,fp8}_async with this `splits_wanted` runs with and needs.  *splits is
// the EFFECTIVE piece count; grid (workgroups of the attention launch) and narrow (1: the 16-head form) may be null.
extern "C" int hpc_attention_decode_mla_sparse_plan(int num_batch, int num_seq_q, int num_head, int topk, int splits_wanted,
                                                    int num_cu, int* splits, int* max_splits, int64_t* workspace_bytes,
                                                    int* grid, int* narrow) {
  if (!splits || !max_splits || !workspace_bytes) return HPC_ERR_INVALID;
  const hpc::MlaRoute r = mla_plan_route(num_batch, num_seq_q, num_head, true, topk, splits_wanted, num_cu);
  *splits = r.splits, *max_splits = r.max_splits, *workspace_bytes = r.workspace_bytes;
  if (grid) *grid = r.grid;
  if (narrow) *narrow = r.narrow;
  return r.code;
}

extern "C" int hpc_attention_decode_mla_sparse_bf16_async(void* out_ptr, float* lse_ptr, const void* q_ptr, const void* ckv_ptr,
                                                          const int* block_ids_ptr, const int* num_seq_kvcache_ptr,
                                                          const int* indices_ptr, int num_batch, int num_seq_q, int num_head,
                                                          int topk, int block_size, int max_blocks, int num_blocks,
                                                          int64_t ckv_block_stride, int64_t ckv_token_stride, float softmax_scale,
                                                          int new_kv_included, int splits, void* workspace_ptr,
                                                          int64_t workspace_bytes, hipStream_t stream) {
  return mla_decode_launch<false, true>({out_ptr, lse_ptr, q_ptr, ckv_ptr, block_ids_ptr,
                                         MlaRows::step(num_seq_kvcache_ptr, num_batch, num_seq_q, new_kv_included), indices_ptr,
                                         num_head, topk, block_size, max_blocks, num_blocks, ckv_block_stride, ckv_token_stride,
                                         softmax_scale, splits, workspace_ptr, workspace_bytes, stream});
}

// the same over the FP8 latent cache (mla_fp8_format.h); the cache's strides in bytes
extern "C" int hpc_attention_decode_mla_sparse_fp8_async(void* out_ptr, float* lse_ptr, const void* q_ptr, const void* ckv_ptr,
                                                         const int* block_ids_ptr, const int* num_seq_kvcache_ptr,
                                                         const int* indices_ptr, int num_batch, int num_seq_q, int num_head,
                                                         int topk, int block_size, int max_blocks, int num_blocks,
                                                         int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes,
                                                         float softmax_scale, int new_kv_included, int splits,
                                                         void* workspace_ptr, int64_t workspace_bytes, hipStream_t stream) {
  return mla_decode_launch<true, true>({out_ptr, lse_ptr, q_ptr, ckv_ptr, block_ids_ptr,
                                        MlaRows::step(num_seq_kvcache_ptr, num_batch, num_seq_q, new_kv_included), indices_ptr,
                                        num_head, topk, block_size, max_blocks, num_blocks, ckv_block_stride_bytes,
                                        ckv_token_stride_bytes, softmax_scale, splits, workspace_ptr, workspace_bytes, stream});
}

// ---- the token-sparse form over a ragged prefill chunk: row r of the chunk is a unit, its request and what it sees come from the
// row rule on the device (num_seqlen_per_req: total lengths including the chunk's tokens; q_index [num_req + 1]); everything
// else - route, launcher, kernel, merge - is the decode form's, and what a chunk's rows ask beyond a step's is the launcher's.
// num_rows == 0 or num_req == 0 launches nothing.
extern "C" int hpc_attention_prefill_mla_sparse_bf16_async(void* out_ptr, float* lse_ptr, const void* q_ptr, const void* ckv_ptr,
                                                           const int* block_ids_ptr, const int* num_seqlen_per_req_ptr,
                                                           const int* q_index_ptr, const int* indices_ptr, int num_rows, int num_req,
                                                           int num_head, int topk, int block_size, int max_blocks, int num_blocks,
                                                           int64_t ckv_block_stride, int64_t ckv_token_stride, float softmax_scale,
                                                           int splits, void* workspace_ptr, int64_t workspace_bytes,
                                                           hipStream_t stream) {
  return mla_decode_launch<false, true>({out_ptr, lse_ptr, q_ptr, ckv_ptr, block_ids_ptr,
                                         MlaRows::chunk(num_seqlen_per_req_ptr, q_index_ptr, num_rows, num_req, 0), indices_ptr,
                                         num_head, topk, block_size, max_blocks, num_blocks, ckv_block_stride, ckv_token_stride,
                                         softmax_scale, splits, workspace_ptr, workspace_bytes, stream});
}

extern "C" int hpc_attention_prefill_mla_sparse_fp8_async(void* out_ptr, float* lse_ptr, const void* q_ptr, const void* ckv_ptr,
                                                          const int* block_ids_ptr, const int* num_seqlen_per_req_ptr,
                                                          const int* q_index_ptr, const int* indices_ptr, int num_rows, int num_req,
                                                          int num_head, int topk, int block_size, int max_blocks, int num_blocks,
                                                          int64_t ckv_block_stride_bytes, int64_t ckv_token_stride_bytes,
                                                          float softmax_scale, int splits, void* workspace_ptr,
                                                          int64_t workspace_bytes, hipStream_t stream) {
  return mla_decode_launch<true, true>({out_ptr, lse_ptr, q_ptr, ckv_ptr, block_ids_ptr,
                                        MlaRows::chunk(num_seqlen_per_req_ptr, q_index_ptr, num_rows, num_req, 0), indices_ptr,
                                        num_head, topk, block_size, max_blocks, num_blocks, ckv_block_stride_bytes,
                                        ckv_token_stride_bytes, softmax_scale, splits, workspace_ptr, workspace_bytes, stream});
}
