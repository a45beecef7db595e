// Grouped GEMM with OCP MXFP4 weights and e4m3 activations (W4A8), weight-streaming form for decode steps - gfx950.
//
// The arithmetic, for the rows r of group (expert) g - x[r] is row row_index[r] of x when a row_index is given, and so is xs[r]:
//
//   P[r, n, kb] = sum over the 128 k of block kb of  x[r, k] * e2m1(w[g, n, k]) * 2^(s[g, n, k / 32] - 127)
//                 one scaled MFMA into a zero accumulator, A = FP4 weights with their e8m0 scales in hardware,
//                 B = e4m3 activations with scale byte 127
//   tot = fmaf(P[r, n, kb], xs[r, kb], tot)      kb ascending, fp32
//   y[r, n] = bf16_rne(tot)
//
// x e4m3 [rows, K], xs f32 [rows, K / 128] row-major (what hpc_blockwise_fp8_quant_async writes); w uint8 [G, N, K / 2], two e2m1
// codes per byte, even k in the low nibble; s uint8 [G, N, K / 32], e8m0 (a scale byte 255 is NaN: unspecified); y bf16 [M, N].
// The weights stay in checkpoint layout: there is no re-laid-out copy.
//
// A sibling of gemm_blockwise_stream2_kernel (group_gemm_blockwise.hip): grid (N / 64, G), four waves of 16 weight rows, the
// activation tile of the pass (16 / 32 / 48 tokens) shared through a double-buffered LDS tile fetched at the weights' prefetch
// depth, one barrier per stage of two k-blocks.  What differs is the weights' path.  As probed (tools/probes/probe_mfma_fp4.hip,
// DESIGN.md), v_mfma_scale_f32_16x16x128_f8f6f4 gives lane l of an FP4 operand row l % 16 and the 32 CONSECUTIVE k of group l / 16 -
// one MX block, which the lane's scale byte multiplies and nothing else - while lane l of an 8-bit operand holds the 16 k of group
// l / 16 and the 16 that lie 64 further on.  So
//  * a lane's A operand of a k-block is the 16 bytes at row * K / 2 + kb * 64 + (l / 16) * 16 of the checkpoint layout: it is loaded
//    straight into the operand registers, with no LDS tile in between, and its scale is byte l / 16 of the dword at
//    row * K / 32 + kb * 4;
//  * the e4m3 side keeps the FP8 kernels' read pattern, 16-byte chunks g4 and g4 + 4 of its token's 128 bytes: that is the
//    hardware's order of an 8-bit operand, not a permutation the two sides merely had to share.
#include "hpc_common.h"
#include "../../include/hpc_amd.h"
#include "group_gemm_mxfp4_route.h"

namespace hpc {
namespace mxfp4 {

struct Args {
  const uint8_t* x;    // e4m3 [x_rows, K]
  const float* xs;     // [x_rows, KB]
  const uint8_t* w;    // [G, N, K / 2]
  const uint8_t* ws;   // [G, N, K / 32]
  uint16_t* y;         // bf16 [M, N]
  const int* seqlens;  // [G]
  const int* cu_seqlens;
  const int* row_index;  // null: row r of the output reads row r of x and xs
  int N, K, KB;          // KB = K / 128
  unsigned x_bytes, xs_bytes;
};

constexpr int kXRow = 272;  // LDS bytes per staged activation row (256 + 16: conflict-free b128 reads)

// kMT = token blocks of 16 served per pass over the weights; kDepth = stages (two k-blocks: 128 bytes per weight row, 256 per
// token) in flight per wave.
template <int kMT, int kDepth>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_stream_kernel(const Args a) {
  constexpr int kTok = 16 * kMT;
  constexpr int kXI = kMT;  // activation staging instructions (4 rows x 256 B each) per wave
  __shared__ __attribute__((aligned(16))) uint8_t s_x[2][kTok * kXRow];
  __shared__ float s_xs[2][2][kTok];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g4 = lane >> 4;
  const int e = blockIdx.y;
  const int m_cnt = as_const(a.seqlens)[e];
  if (m_cnt <= 0) return;
  const int n0 = (blockIdx.x * 4 + wave) * 16;
  const int m0 = as_const(a.cu_seqlens)[e];
  const int K = a.K, KB = a.KB;
  const int KH = K >> 1, KS = K >> 5;  // bytes per weight row, per scale row
  const int nstage = (KB + 1) >> 1;

  const uint8_t* wbase = a.w + (static_cast<long>(e) * a.N + n0) * KH;
  const uint8_t* sbase = a.ws + (static_cast<long>(e) * a.N + n0) * KS;
  const unsigned w_bytes = 16u * static_cast<unsigned>(KH), s_bytes = 16u * static_cast<unsigned>(KS);
  const int w_voff = r16 * KH + g4 * 16;  // the lane's row, its MX block of a k-block
  const int s_voff = r16 * KS;            // the lane's row: one dword = the four scale bytes of a k-block
  const int s_shift = 8 * g4;

  const int npass = (m_cnt + kTok - 1) / kTok;
  for (int p = 0; p < npass; ++p) {
    // the weight loads of the first kDepth stages go out before the lane's activation roles are known (they hang on row_index)
    u32x4 wb[kDepth][2];
    int sb[kDepth][2];
    auto issue_w = [&](int d, int st) {
      // whole stage on / off (a descriptor with num_records = 0 fetches nothing).  With an odd number of k-blocks the second half
      // of the last stage reads into the next weight row (or, behind the wave's last row, zero): never used, see below.
      const unsigned on = st < nstage ? 1u : 0u;
      const auto rw = make_rsrc(wbase, on * w_bytes);
      const auto rs = make_rsrc(sbase, on * s_bytes);
#pragma unroll
      for (int kbl = 0; kbl < 2; ++kbl) {
        wb[d][kbl] = buf_ld16<2>(rw, w_voff, st * 128 + kbl * 64);
        sb[d][kbl] = __builtin_amdgcn_raw_buffer_load_b32(rs, s_voff, (2 * st + kbl) * 4, 0);
      }
    };
    int xrow_j[kXI], xrow_s;
#pragma unroll
    for (int j = 0; j < kXI; ++j) {
      const int slot = p * kTok + 4 * (wave * kXI + j) + g4;
      const int sc = slot < m_cnt ? slot : m_cnt - 1;  // rows past the group: its last row again, never stored
      xrow_j[j] = a.row_index ? a.row_index[m0 + sc] : m0 + sc;
    }
    {
      const int slot = p * kTok + (lane < kTok ? lane : 0);
      const int sc = slot < m_cnt ? slot : m_cnt - 1;
      xrow_s = a.row_index ? a.row_index[m0 + sc] : m0 + sc;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = 0; d < kDepth; ++d) issue_w(d, d);
    __builtin_amdgcn_sched_barrier(0);
    // x rows: instruction i = wave * kXI + j loads tile rows 4 i .. 4 i + 3, lane -> (row 4 i + g4, 16-byte chunk r16)
    unsigned x_voff[kXI];
    int x_lds[kXI];
#pragma unroll
    for (int j = 0; j < kXI; ++j) {
      x_voff[j] = static_cast<unsigned>(xrow_j[j]) * static_cast<unsigned>(K) + r16 * 16;
      x_lds[j] = (4 * (wave * kXI + j) + g4) * kXRow + r16 * 16;
    }
    // scales: waves 0 / 1 load k-block 0 / 1 of the stage, lane -> token `lane` (lanes past the tile: token 0, never stored)
    const bool xs_role = wave < 2 && lane < kTok;
    const unsigned xs_voff = static_cast<unsigned>(xrow_s) * static_cast<unsigned>(KB) * 4u;
    const int xs_wave = wave < 2 ? wave : 0;

    u32x4 xb[kDepth][kXI];
    float xsb[kDepth];
    auto issue_x = [&](int d, int st) {
      const int kb0 = 2 * st;
      // (chunks at k >= K, in the second half of an odd last stage, read the next row or zero: never used)
      const auto rx = make_rsrc(a.x, st < nstage ? a.x_bytes : 0u);
#pragma unroll
      for (int j = 0; j < kXI; ++j) xb[d][j] = buf_ld16<0>(rx, x_voff[j], kb0 * 128);
      // wave-uniform, and pinned so that hipcc sees it (a descriptor it cannot prove uniform costs a waterfall loop per load)
      const auto rs = make_rsrc(a.xs, __builtin_amdgcn_readfirstlane((wave < 2 && kb0 + xs_wave < KB) ? a.xs_bytes : 0u));
      xsb[d] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xs_voff, (kb0 + xs_wave) * 4, 0));
    };
#pragma unroll
    for (int d = 0; d < kDepth; ++d) {
      issue_x(d, d);
      __builtin_amdgcn_sched_barrier(0);  // keep issue order = consumption order (in-order vmcnt)
    }

    f32x4 tot[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) tot[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int st0 = 0; st0 < nstage; st0 += kDepth) {
#pragma unroll
      for (int d = 0; d < kDepth; ++d) {
        const int st = st0 + d;
        if (st < nstage) {  // the same for every wave of the workgroup: the barrier below is met by all or by none
          const int buf = (kDepth & 1) ? (st & 1) : (d & 1);
#pragma unroll
          for (int j = 0; j < kXI; ++j) *reinterpret_cast<u32x4*>(&s_x[buf][x_lds[j]]) = xb[d][j];
          if (xs_role) s_xs[buf][wave][lane] = xsb[d];
          // the stage's operands move to registers of their own, and its slot is refilled now: the loads travel while the
          // stage is computed
          const u32x4 wa[2] = {wb[d][0], wb[d][1]};
          const int sa[2] = {sb[d][0], sb[d][1]};
          __builtin_amdgcn_sched_barrier(0);
          issue_w(d, st + kDepth);
          issue_x(d, st + kDepth);
          __builtin_amdgcn_sched_barrier(0);
          __syncthreads();
#pragma unroll
          for (int kbl = 0; kbl < 2; ++kbl) {
            if (2 * st + kbl < KB) {  // the k-block behind an odd count's last one is not computed at all
              const i32x8 av = {static_cast<int>(wa[kbl][0]), static_cast<int>(wa[kbl][1]), static_cast<int>(wa[kbl][2]),
                                static_cast<int>(wa[kbl][3]), 0, 0, 0, 0};
              const int scale_a = (sa[kbl] >> s_shift) & 0xff;
#pragma unroll
              for (int q = 0; q < kMT; ++q) {
                const uint8_t* xp = &s_x[buf][(q * 16 + r16) * kXRow + kbl * 128 + g4 * 16];
                const u32x4 b0 = *reinterpret_cast<const u32x4*>(xp);
                const u32x4 b1 = *reinterpret_cast<const u32x4*>(xp + 64);
                const float f = s_xs[buf][kbl][q * 16 + r16];
                const i32x8 bv = {static_cast<int>(b0[0]), static_cast<int>(b0[1]), static_cast<int>(b0[2]), static_cast<int>(b0[3]),
                                  static_cast<int>(b1[0]), static_cast<int>(b1[1]), static_cast<int>(b1[2]), static_cast<int>(b1[3])};
                const f32x4 part = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                    av, bv, f32x4{0.f, 0.f, 0.f, 0.f}, /*cbsz: A is e2m1*/ 4, /*blgp: B is e4m3*/ 0, /*op_sel_a*/ 0, scale_a,
                    /*op_sel_b*/ 0, 0x7f7f7f7f);
#pragma unroll
                for (int i = 0; i < 4; ++i) tot[q][i] = fmaf(part[i], f, tot[q][i]);
              }
            }
          }
        }
      }
    }

    // D: column = lane & 15 = the token, row = 4 (lane >> 4) + i = the weight row
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
      const int slot = p * kTok + mt * 16 + r16;
      if (slot < m_cnt) {
        u32x2 pk;
        pk[0] = pack_bf16x2(tot[mt][0], tot[mt][1]);
        pk[1] = pack_bf16x2(tot[mt][2], tot[mt][3]);
        *reinterpret_cast<u32x2*>(a.y + static_cast<long>(m0 + slot) * a.N + n0 + g4 * 4) = pk;
      }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // retire stores before the next pass (see attention_decode.hip)
    __syncthreads();
  }
}

}  // namespace mxfp4
}  // namespace hpc

// What a call of hpc_group_gemm_mxfp4_async with these shapes runs with: mxfp4_route().  Any out pointer may be null.
extern "C" int hpc_group_gemm_mxfp4_plan(int num_group, int m, int x_rows, int n, int k, int* tokens_per_pass, int* grid_x,
                                         int* grid_y) {
  const hpc::Mxfp4Route r = hpc::mxfp4_route(num_group, m, x_rows, n, k);
  if (tokens_per_pass) *tokens_per_pass = 16 * r.mt;
  if (grid_x) *grid_x = r.grid_x;
  if (grid_y) *grid_y = r.grid_y;
  return r.code;
}

extern "C" int hpc_group_gemm_mxfp4_async(void* y_ptr, const void* x_ptr, const float* x_scale_ptr, const void* weight_ptr,
                                          const void* weight_scale_ptr, const int* seqlens_ptr, const int* cu_seqlens_ptr,
                                          const int* row_index_ptr, int num_group, int m, int x_rows, int n, int k,
                                          hipStream_t stream) {
  using namespace hpc::mxfp4;
  if (!y_ptr || !x_ptr || !x_scale_ptr || !weight_ptr || !weight_scale_ptr || !seqlens_ptr || !cu_seqlens_ptr)
    return HPC_ERR_INVALID;
  const hpc::Mxfp4Route r = hpc::mxfp4_route(num_group, m, x_rows, n, k);
  if (r.code) return r.code;
  if (!row_index_ptr && x_rows < m) return HPC_ERR_INVALID;  // row r of the output reads row r of x
  if (m > 0 && x_rows == 0) return HPC_ERR_INVALID;
  const auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if (misaligned(y_ptr) || misaligned(x_ptr) || misaligned(x_scale_ptr) || misaligned(weight_ptr) || misaligned(weight_scale_ptr))
    return HPC_ERR_UNSUPPORTED;
  if (m == 0) return HPC_OK;
  Args a{};
  a.x = static_cast<const uint8_t*>(x_ptr);
  a.xs = x_scale_ptr;
  a.w = static_cast<const uint8_t*>(weight_ptr);
  a.ws = static_cast<const uint8_t*>(weight_scale_ptr);
  a.y = static_cast<uint16_t*>(y_ptr);
  a.seqlens = seqlens_ptr;
  a.cu_seqlens = cu_seqlens_ptr;
  a.row_index = row_index_ptr;
  a.N = n;
  a.K = k;
  a.KB = k / 128;
  a.x_bytes = static_cast<unsigned>(static_cast<int64_t>(x_rows) * k);
  a.xs_bytes = static_cast<unsigned>(static_cast<int64_t>(x_rows) * (k / 128) * 4);
  const dim3 grid(r.grid_x, r.grid_y);
  if (r.mt == 1)
    gemm_mxfp4_stream_kernel<1, 8><<<grid, 256, 0, stream>>>(a);
  else if (r.mt == 2)
    gemm_mxfp4_stream_kernel<2, 8><<<grid, 256, 0, stream>>>(a);
  else
    gemm_mxfp4_stream_kernel<3, 6><<<grid, 256, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
