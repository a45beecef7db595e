// Dense FP8 linear with 128-block scales for decode batches - gfx950.  Ours only: no reference counterpart (the reference
// runs such layers through its grouped GEMM); the statement is tests/linear_fp8_ref.py:
//
//   y[m, n] = bf16( sum_kb  xs[m, kb] * ws[n / 128, kb] * sum_{k in block kb} float(x[m, k]) * float(w[n, k]) )
//
// x e4m3 [M, K] with one fp32 scale per row and 128 columns (what blockwise_fp8_quant writes), w e4m3 [N, K] with one fp32
// scale per 128 x 128 block, 1 <= M <= 256.  The Q/KV/O projections, dense and shared-expert MLPs and the LM head of a
// block-scaled FP8 model.
//
// It is a stream of the weights (N * K bytes against at most 256 tokens), so the design is the streaming grouped kernel's
// (group_gemm_blockwise.hip) without the groups, and with K split over workgroups where N / 64 tiles alone leave CUs idle:
//  * weights on the MFMA M axis, tokens on N.  A workgroup owns 64 weight rows (four waves x 16) x up to 64 tokens x one K slice;
//  * a wave fetches its 16 rows straight into A-operand registers - 16-byte non-temporal buffer loads, two per 128-wide k-block
//    (lane (r16, g4) holds chunks g4 and g4 + 4 of row r16, the operand convention of the grouped kernels), kDepth k-blocks in
//    flight, refilled as soon as a block's MFMAs are issued; loads past the slice's end use an empty descriptor (read zeros,
//    fetch nothing), so the loop has no branch around a load and runs whole rounds of kDepth steps (an exit inside a round
//    makes hipcc drain the memory counter at the loop's head);
//  * the four waves share the activations: per k-block the workgroup stages [tokens][128 B] (full lines, 16-byte chunks
//    XOR-swizzled with the token index) and the tokens' scales into a double-buffered LDS tile, requested as far ahead as
//    the weights; one barrier per k-block;
//  * a k-block is a chain of FOUR v_mfma_f32_16x16x32_f16 per 16-token block, on operands converted e4m3 -> f16 in registers
//    (exact; two codes per v_cvt_scalef32_pk_f16_fp8); its fp32 partial is rescaled by xs * ws and accumulated (fmaf).  Not
//    the fp8 matrix instruction: that one sums the products of a lane's operand chunk in a window of about 15 bits below
//    the largest (measured: up to 2^-11 of the block's largest product lost per block, against 6 x 2^-23 on the f16 form),
//    which misses the statement's fp32 bar wherever a block's products cancel (profiles/linear_fp8.txt).  The
//    price against the fp8 instruction, measured: 0 - 5 % at M <= 16, up to 12 % at M = 64 and 22 % at M = 256;
//  * M > 64 runs as further token tiles on the grid (lgemm_route: m_tiles): every tile streams the weights again, as a further
//    pass inside the workgroup would, but the tiles run side by side on CUs that the N / 64 tiles leave idle and the kernel
//    keeps one accumulator set;
//  * splits > 1: every K slice writes its fp32 partial to plane [split][M][N] of the workspace with write-through 16-byte
//    stores and publishes it: every wave waits for its stores' acknowledgement, workgroup barrier, ONE lane draws a ticket with
//    a relaxed agent-scope fetch_add on the tile's counter.  The workgroup that draws the last ticket sets the counter back to
//    zero and sums the planes - read around the caches - in split order 0 .. S - 1, never in arrival order, no float atomics:
//    bit-identical from call to call.  Nobody waits on a counter: no spin anywhere in this file, a lost arrival can leave a
//    tile unwritten but cannot hang.  (First build: plain stores behind an agent-scope release fence, an acquire fence in the
//    reducer - the fences' L2 write-back and invalidate cost 4-12 us per call: profiles/linear_fp8.txt.)
#include "hpc_common.h"
#include "../../include/hpc_amd.h"
#include "gemm_blockwise_fp8_route.h"

namespace hpc {
namespace lgemm {

struct Args {
  const uint8_t* x;   // [m, k] e4m3
  const float* xs;    // [m, k / 128]
  const uint8_t* w;   // [n, k] e4m3
  const float* ws;    // [ceil(n / 128), k / 128], row stride ws_row_stride floats
  uint16_t* y;        // [m, n] bf16
  float* planes;      // [splits, m, n] fp32 (splits > 1)
  int* counters;      // [m_tiles * n_tiles] int32, zero on entry and on exit (splits > 1)
  int m, n, k, kb, splits, n_tiles;
  long ws_row_stride;
};

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// Eight e4m3 codes (two dwords, in byte order) as f16: exact, every e4m3 value is an f16 value.
__device__ __forceinline__ f16x8 e4m3x8_to_f16(unsigned lo, unsigned hi) {
  const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false);
  const f16x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
  const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false);
  const f16x2 e = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
  return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], e[0], e[1]};
}

constexpr int kThreads = 256;
constexpr int kDepth = 4;  // k-blocks in flight per wave (4 x 2 KB of weights); the loop runs whole rounds of kDepth steps

template <int kMT>
__global__ __launch_bounds__(kThreads, 2) void gemm_blockwise_fp8_kernel(const Args a) {
  constexpr int kXQ = (16 * kMT + 31) / 32;  // 16-byte chunks a thread stages per k-block: 32 tokens x 8 chunks per instruction
  constexpr int kRows = 32 * kXQ;
  __shared__ u32x4 s_x[2][kRows * 8];
  __shared__ float s_xs[2][kThreads];  // the first 64 are read; every thread stores (no branch around a load's use)
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g4 = lane >> 4;
  const int bid = blockIdx.x;
  const int split = bid % a.splits, tile = bid / a.splits;
  const int n0 = (tile % a.n_tiles) * 64 + wave * 16, m0 = (tile / a.n_tiles) * 64;
  const int K = a.k;
  const int c_begin = static_cast<int>(static_cast<long>(a.kb) * split / a.splits);
  const int c_end = static_cast<int>(static_cast<long>(a.kb) * (split + 1) / a.splits);

  // weights: the wave's 16 rows behind a descriptor of their own
  const uint8_t* wbase = a.w + static_cast<long>(n0) * K;
  const unsigned w_bytes = 16u * static_cast<unsigned>(K);
  const int w_voff = r16 * K + g4 * 16;
  const cfloat_ptr ws_row = as_constf(a.ws) + static_cast<long>(n0 >> 7) * a.ws_row_stride;
  // activations: thread t stages chunk t % 8 of tokens t / 8 + 32 q; tokens past m read row m - 1 (never stored)
  const unsigned x_bytes = static_cast<unsigned>(a.m) * static_cast<unsigned>(K);
  unsigned xg_off[kXQ];
  int xs_idx[kXQ];
#pragma unroll
  for (int q = 0; q < kXQ; ++q) {
    const int tl = (tid >> 3) + 32 * q, t = m0 + tl;
    xg_off[q] = static_cast<unsigned>(t < a.m ? t : a.m - 1) * static_cast<unsigned>(K) + (tid & 7) * 16;
    xs_idx[q] = tl * 8 + ((tid & 7) ^ (tl & 7));
  }
  const unsigned xsc_bytes = static_cast<unsigned>(a.m) * static_cast<unsigned>(a.kb) * 4u;
  const int ts = m0 + lane;  // every wave loads and stores the 64 tokens' scales (branch-free), wave 0's copy is read
  const unsigned xsc_off = static_cast<unsigned>(ts < a.m ? ts : a.m - 1) * static_cast<unsigned>(a.kb) * 4u;
  // operand reads: token q * 16 + r16, chunks g4 and g4 + 4
  int xr_idx[kMT];
#pragma unroll
  for (int q = 0; q < kMT; ++q) {
    const int tl = q * 16 + r16;
    xr_idx[q] = tl * 8 + (g4 ^ (tl & 7));
  }

  u32x4 wb[kDepth][2];
  auto issue_w = [&](int d, int c) {
    const auto rw = make_rsrc(wbase, c < c_end ? w_bytes : 0u);
    wb[d][0] = buf_ld16<2>(rw, w_voff, c * 128);
    wb[d][1] = buf_ld16<2>(rw, w_voff, c * 128 + 64);
  };
  u32x4 xr[kDepth][kXQ];
  float xsr[kDepth];
  auto load_x = [&](int rb, int c) {
    const bool on = c < c_end;
    const auto rx = make_rsrc(a.x, on ? x_bytes : 0u);
    const auto rs = make_rsrc(a.xs, on ? xsc_bytes : 0u);
#pragma unroll
    for (int q = 0; q < kXQ; ++q) xr[rb][q] = buf_ld16<0>(rx, xg_off[q], c * 128);
    xsr[rb] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xsc_off, c * 4, 0));
  };
  auto stage = [&](int sb, int rb) {
#pragma unroll
    for (int q = 0; q < kXQ; ++q) s_x[sb][xs_idx[q]] = xr[rb][q];
    s_xs[sb][tid] = xsr[rb];
  };

  f32x4 tot[kMT];
#pragma unroll
  for (int q = 0; q < kMT; ++q) tot[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](int sb, int d, int c) {
    const float wsv = ws_row[c < c_end ? c : c_end - 1];  // a round's steps past the slice multiply zeros
    f16x8 av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) av[j] = e4m3x8_to_f16(wb[d][j >> 1][(j & 1) * 2], wb[d][j >> 1][(j & 1) * 2 + 1]);
#pragma unroll
    for (int q = 0; q < kMT; ++q) {
      const u32x4 b0 = s_x[sb][xr_idx[q]], b1 = s_x[sb][xr_idx[q] ^ 4];
      const float f = s_xs[sb][q * 16 + r16] * wsv;
      f32x4 part = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x4 b = j < 2 ? b0 : b1;
        part = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[j], e4m3x8_to_f16(b[(j & 1) * 2], b[(j & 1) * 2 + 1]), part, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) tot[q][i] = fmaf(part[i], f, tot[q][i]);
    }
  };

  // Step s (k-block c_begin + s) lives in ring slot s % kDepth: its activation chunks (staging registers) and its weights are
  // requested together, kDepth steps ahead and the activations first - the memory counter retires in order, so waiting for a
  // step's activations must not wait for younger weight loads.  The activations go to LDS buffer s & 1 one step ahead (that
  // buffer was last read two steps earlier, behind a barrier).
#pragma unroll
  for (int d = 0; d < kDepth; ++d) {
    load_x(d, c_begin + d);
    issue_w(d, c_begin + d);
  }
  stage(0, 0);
  __syncthreads();
  for (int c = c_begin; c < c_end; c += kDepth) {
#pragma unroll
    for (int d = 0; d < kDepth; ++d) {
      stage((d + 1) & 1, (d + 1) % kDepth);
      compute(d & 1, d, c + d);
      load_x(d, c + d + kDepth);
      issue_w(d, c + d + kDepth);
      __syncthreads();
    }
  }
  // lane holds weight rows nn + 0 .. 3 of token m0 + q * 16 + r16
  const int nn = n0 + g4 * 4;
  auto emit = [&](int t, const f32x4 v) {
    u32x2 pk;
    pk[0] = pack_bf16x2(v[0], v[1]);
    pk[1] = pack_bf16x2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(a.y + static_cast<long>(t) * a.n + nn) = pk;
  };
  if (a.splits == 1) {
#pragma unroll
    for (int q = 0; q < kMT; ++q) {
      const int t = m0 + q * 16 + r16;
      if (t < a.m) emit(t, tot[q]);
    }
    return;
  }

  // ---- split-K: park the partial, publish it, draw a ticket; the last arriver of the tile reduces -------------------------------
  // The planes travel write-through (sc0 sc1 stores, acknowledged before the ticket) and are read around the caches (sc0 sc1
  // loads, EVERY load of them): no L2 write-back / invalidate fence, which costs more than the GEMM here (measured:
  // profiles/linear_fp8.txt, "publish recipe").
  const unsigned plane = static_cast<unsigned>(a.m) * static_cast<unsigned>(a.n) * 4u;  // plane * splits <= 0xfffffff0 (route)
  const auto rp = make_rsrc(a.planes, plane * static_cast<unsigned>(a.splits));
#pragma unroll
  for (int q = 0; q < kMT; ++q) {
    const int t = m0 + q * 16 + r16;
    if (t < a.m)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, tot[q]), rp,
                                             (static_cast<unsigned>(t) * a.n + nn) * 4u, split * plane, 17);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave: its write-through stores are acknowledged
  __syncthreads();
  if (tid == 0) {
    int* cnt = a.counters + tile;
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == a.splits - 1;
    // every slice has arrived: nobody touches the counter again in this launch - zero for the next call
    if (last) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  // One token block at a time, all of its (up to 16) plane loads in flight at once - a serial load -> add chain costs a memory
  // round trip per split.  Planes past a.splits use an empty descriptor (read 0, add nothing).  Sum in split order.
  const auto rnull = make_rsrc(a.planes, 0u);
#pragma unroll
  for (int q = 0; q < kMT; ++q) {
    const int t = m0 + q * 16 + r16;
    const unsigned off = (static_cast<unsigned>(t < a.m ? t : 0) * a.n + nn) * 4u;
    u32x4 part[kLgemmMaxSplits];
#pragma unroll
    for (int sp = 0; sp < kLgemmMaxSplits; ++sp) part[sp] = buf_ld16<17>(sp < a.splits ? rp : rnull, off, sp * plane);
    f32x4 sum = __builtin_bit_cast(f32x4, part[0]);
#pragma unroll
    for (int sp = 1; sp < kLgemmMaxSplits; ++sp) sum += __builtin_bit_cast(f32x4, part[sp]);
    if (t < a.m) emit(t, sum);
  }
}

}  // namespace lgemm
}  // namespace hpc

// What a call of hpc_gemm_blockwise_fp8_async with this `splits_wanted` runs with and needs: lgemm_route()
// (gemm_blockwise_fp8_route.h).  cu_count <= 0: the current device's (256 without a device).
extern "C" int hpc_gemm_blockwise_fp8_plan(int m, int n, int k, int splits_wanted, int cu_count, int* splits, int* max_splits,
                                           int64_t* workspace_bytes, int* counters) {
  if (!splits || !max_splits || !workspace_bytes || !counters) return HPC_ERR_INVALID;
  const hpc::LgemmRoute r = hpc::lgemm_route(m, n, k, splits_wanted, cu_count > 0 ? cu_count : hpc::current_cu_count());
  *splits = r.splits, *max_splits = r.max_splits, *workspace_bytes = r.workspace_bytes, *counters = r.counters;
  return r.code;
}

extern "C" int hpc_gemm_blockwise_fp8_async(void* y_ptr, const void* x_ptr, const float* x_scale_ptr, const void* weight_ptr,
                                            const float* weight_scale_ptr, int m, int n, int k, int64_t ws_row_stride, int splits,
                                            void* workspace_ptr, int64_t workspace_bytes, void* counters_ptr,
                                            hipStream_t stream) {
  using namespace hpc::lgemm;
  if (!y_ptr || !x_ptr || !x_scale_ptr || !weight_ptr || !weight_scale_ptr) return HPC_ERR_INVALID;
  if (splits < 0) return HPC_ERR_INVALID;
  // the split count is the caller's, or with 0 the route's for this device; shapes are refused before the device is asked
  const hpc::LgemmRoute shape = hpc::lgemm_route(m, n, k, splits > 0 ? splits : 1, 256);
  if (shape.code != HPC_OK) return shape.code;
  if (ws_row_stride < (k >> 7)) return HPC_ERR_INVALID;
  if ((reinterpret_cast<uintptr_t>(x_ptr) | reinterpret_cast<uintptr_t>(weight_ptr)) & 15) return HPC_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(y_ptr) & 7) return HPC_ERR_UNSUPPORTED;
  if (m == 0) return HPC_OK;
  const hpc::LgemmRoute r = splits > 0 ? shape : hpc::lgemm_route(m, n, k, 0, hpc::current_cu_count());
  if (r.code != HPC_OK) return r.code;
  if (r.splits > 1) {
    if (!workspace_ptr || !counters_ptr || workspace_bytes < r.workspace_bytes) return HPC_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(workspace_ptr) & 15) || (reinterpret_cast<uintptr_t>(counters_ptr) & 3))
      return HPC_ERR_UNSUPPORTED;
  }
  Args a;
  a.x = static_cast<const uint8_t*>(x_ptr);
  a.xs = x_scale_ptr;
  a.w = static_cast<const uint8_t*>(weight_ptr);
  a.ws = weight_scale_ptr;
  a.y = static_cast<uint16_t*>(y_ptr);
  a.planes = static_cast<float*>(workspace_ptr);
  a.counters = static_cast<int*>(counters_ptr);
  a.m = m;
  a.n = n;
  a.k = k;
  a.kb = k >> 7;
  a.splits = r.splits;
  a.n_tiles = r.n_tiles;
  a.ws_row_stride = ws_row_stride;
  const dim3 grid(r.grid);
  if (r.mt == 1)
    gemm_blockwise_fp8_kernel<1><<<grid, kThreads, 0, stream>>>(a);
  else if (r.mt == 2)
    gemm_blockwise_fp8_kernel<2><<<grid, kThreads, 0, stream>>>(a);
  else
    gemm_blockwise_fp8_kernel<4><<<grid, kThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
