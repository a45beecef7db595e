// MLA prefill attention in bf16, non-absorbed form, contiguous varlen q / k / v with an lse output (attention_prefill_mla_bf16) -
// gfx950.  No reference kernel; the statement is tests/mla_prefill_ref.py.
//
// The structure of attention_prefill_bf16.hip: 64 KV tokens on the MFMA M axis, q rows on N (S^T = K Q^T, O^T = V^T P^T with
// v_mfma_f32_16x16x32_bf16), a wave owns 32 q positions of ONE head and finishes alone, a workgroup = 4 waves = 128 consecutive
// positions that walk the KV tiles together; every 64-token tile is fetched once per workgroup - wave w loads token block w, one
// tile ahead - into a double-buffered LDS stage, one barrier per tile; V^T operands come out of LDS through ds_read_b64_tr_b16;
// masked and unmasked tile bodies chosen at compile time; q tiles handed out last-first.  What differs:
//   * six 32-column k-steps for S: a K row in LDS is 384 bytes - 256 from k_nope[token, head] and 128 from k_pe[token], the one
//     RoPE'd head every head shares, fetched once per tile as a third staged operand; no [Tk, H, 192] tensor exists anywhere;
//   * the K image is not padded but XOR-swizzled (16-byte chunk c of row t in slot c ^ ((t >> 1) & 7): stays inside its group of
//     eight chunks, so 24 chunks a row work), which makes two K and two V images 81,920 bytes: two workgroups fit a CU's 160 KiB;
//   * lse = (m + log2 l) ln 2 in fp32 from the epilogue; a row that sees no key writes zeros and -inf;
//   * a non-causal form (the context pass of a chunked prefill): every tile but a partial last one takes the unmasked body;
//   * the grid's y axis is the head (group 1).
// Host side: the grid and every refusal are attention_prefill_mla_route.h::mla_prefill_route().
#include "attention_prefill_mla_route.h"
#include "attention_prefill_tile.h"
#include "hpc_common.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace prefill_mla {

struct Args {
  const void* q;
  const void* k_nope;
  const void* k_pe;
  const void* v;
  const int* cu_seqlens_q;
  const int* cu_seqlens_k;
  uint16_t* y;
  float* lse;  // null: not wanted
  int num_head, causal;
  long q_row_stride, q_head_stride;  // elements
  int k_row_stride, k_pe_row_stride, v_row_stride;
  long k_head_stride, v_head_stride;
  float scale_log2;
};

using namespace prefill_tile;
static_assert(kWgRows == kMlaPrefillRowTile && kThreads == kMlaPrefillThreads, "the grid of mla_prefill_route() counts these row tiles");
constexpr int kKSteps = kMlaPrefillDimQk / 32;  // 6
constexpr int kKRow = kMlaPrefillDimQk * 2;     // 384 bytes, no pad: chunks swizzled
constexpr int kKTileBytes = 64 * kKRow;
constexpr int kVTileBytes = 64 * 256;           // unpadded 256-byte rows, chunks XOR-swizzled for the transposing reads
constexpr int kStageBytes = 2 * kKTileBytes + 2 * kVTileBytes;
constexpr int kEpiBytes = kWaves * 16 * (128 + 4) * 4 + kWaves * 16 * 4;
static_assert(kStageBytes == 81920 && kEpiBytes <= kStageBytes, "two workgroups share 160 KiB");
constexpr float kLn2 = 0.6931471805599453f;

union Frag16 {
  u32x4 u;
  bf16x8 b;
};

__global__ __launch_bounds__(kThreads, 2) void prefill_mla_bf16_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[kStageBytes];
  uint8_t* s_k = s_raw;                    // [2][64 * 384], chunk c of token row t in slot c ^ ((t >> 1) & 7)
  uint8_t* s_v = s_raw + 2 * kKTileBytes;  // [2][64 * 256], chunk c of token row t in slot c ^ (2 * (t & 7))

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int q0 = as_const(a.cu_seqlens_q)[b];
  const int Sq = as_const(a.cu_seqlens_q)[b + 1] - q0;
  const int k0 = as_const(a.cu_seqlens_k)[b];
  const int L = as_const(a.cu_seqlens_k)[b + 1] - k0;
  // q tiles are handed out last-first: a late tile walks the most KV (causal), so the longest workgroups start first
  const int wg_pos0 = (gridDim.x - 1 - blockIdx.x) * kWgRows;
  if (wg_pos0 >= Sq) return;
  const int row0 = wave * kRowsPerWave;
  const int pos_first = wg_pos0 + row0;
  const int past = L - Sq;  // causal, bottom-right aligned: row s sees keys j <= past + s (none when that is negative)
  const int wg_pos_last = min(Sq - 1, wg_pos0 + kWgRows - 1);
  const int num_seqkv = a.causal ? past + wg_pos_last + 1 : L;  // keys the workgroup walks (<= L)
  const int ntile = num_seqkv > 0 ? (num_seqkv + 63) >> 6 : 0;
  const int ntile_full = a.causal ? max(past + pos_first + 1, 0) >> 6 : L >> 6;  // tiles every row of the wave sees in full
  const uint8_t* qbase = static_cast<const uint8_t*>(a.q);
  const uint8_t* kbase = static_cast<const uint8_t*>(a.k_nope);
  const uint8_t* pbase = static_cast<const uint8_t*>(a.k_pe);
  const uint8_t* vbase = static_cast<const uint8_t*>(a.v);

  // ---- Q fragments: lane (n, g) holds columns (4j + g) * 8 .. + 7 of row n for k-step j (j = 4, 5: the RoPE columns) ----
  u32x4 qf[kNB][kKSteps];
#pragma unroll
  for (int nb = 0; nb < kNB; ++nb) {
    const int pos = wg_pos0 + row0 + nb * 16 + n;
    const bool ok = pos < Sq;
    const long qoff = (static_cast<long>(q0 + pos) * a.q_row_stride + h * a.q_head_stride) * 2;
#pragma unroll
    for (int j = 0; j < kKSteps; ++j) {
      qf[nb][j] = u32x4{0u, 0u, 0u, 0u};
      if (ok) qf[nb][j] = ld16(qbase + qoff + (4 * j + g) * 16);
    }
  }

  // ---- staging role: token block `wave` of each tile.  k_nope and v: lane -> (row lane / 16 (+ 4 c), chunk lane % 16), four
  // 16-byte loads each; k_pe: lane -> (row lane / 8 (+ 8 c), chunk lane % 8), two loads.  Every read is bounded by the rows of the
  // request that exist (buffer limits: reads beyond return zero and fetch nothing) ----
  const int last_blk16 = (num_seqkv - 1) >> 4;
  const int st_chunk = lane & 15, st_rsub = lane >> 4;
  const int pe_chunk = lane & 7, pe_rsub = lane >> 3;
  const int k_voff = st_rsub * a.k_row_stride * 2 + st_chunk * 16;
  const int v_voff = st_rsub * a.v_row_stride * 2 + st_chunk * 16;
  const int p_voff = pe_rsub * a.k_pe_row_stride * 2 + pe_chunk * 16;
  const int k_ld_bytes = 4 * a.k_row_stride * 2, v_ld_bytes = 4 * a.v_row_stride * 2, p_ld_bytes = 8 * a.k_pe_row_stride * 2;
  u32x4 kst[4], pst[2], vst[4];
  long nx_tok = 0;
  unsigned nx_rows = 0;
  auto fetch_k = [&](int t) {
    int blk = t * 4 + wave;
    blk = blk < last_blk16 ? blk : last_blk16;
    const int gtok = blk << 4;
    nx_tok = static_cast<long>(k0 + gtok);
    nx_rows = static_cast<unsigned>(min(16, L - gtok));
    const auto rk = make_rsrc(kbase + (nx_tok * a.k_row_stride + h * a.k_head_stride) * 2, nx_rows * static_cast<unsigned>(a.k_row_stride) * 2u);
#pragma unroll
    for (int c = 0; c < 4; ++c) kst[c] = buf_ld16<0>(rk, k_voff, c * k_ld_bytes);
    const auto rp = make_rsrc(pbase + nx_tok * a.k_pe_row_stride * 2, nx_rows * static_cast<unsigned>(a.k_pe_row_stride) * 2u);
#pragma unroll
    for (int c = 0; c < 2; ++c) pst[c] = buf_ld16<0>(rp, p_voff, c * p_ld_bytes);
  };
  auto fetch_v = [&]() {  // the tile fetch_k was last called for
    const auto rv = make_rsrc(vbase + (nx_tok * a.v_row_stride + h * a.v_head_stride) * 2, nx_rows * static_cast<unsigned>(a.v_row_stride) * 2u);
#pragma unroll
    for (int c = 0; c < 4; ++c) vst[c] = buf_ld16<0>(rv, v_voff, c * v_ld_bytes);
  };
  // K stage: rows c * 4 + st_rsub (nope) and c * 8 + pe_rsub (pe) of the wave's block; the swizzle key of row t is (t >> 1) & 7
  auto stash_k = [&](int buf) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int t = c * 4 + st_rsub;
      *reinterpret_cast<u32x4*>(s_k + buf * kKTileBytes + (wave * 16 + t) * kKRow + ((st_chunk ^ ((t >> 1) & 7)) * 16)) = kst[c];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int t = c * 8 + pe_rsub;
      *reinterpret_cast<u32x4*>(s_k + buf * kKTileBytes + (wave * 16 + t) * kKRow + 256 + ((pe_chunk ^ ((t >> 1) & 7)) * 16)) = pst[c];
    }
  };
  const int vkey_e = (2 * st_rsub) * 16, vkey_o = (8 + 2 * st_rsub) * 16;  // rows c * 4 + st_rsub: (t & 7) = 4 (c & 1) + st_rsub
  auto stash_v = [&](int buf) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<u32x4*>(s_v + buf * kVTileBytes + (wave * 16 + c * 4 + st_rsub) * 256 +
                                ((st_chunk * 16) ^ ((c & 1) ? vkey_o : vkey_e))) = vst[c];
  };

  // K reads: lane (n, g) takes chunk (4j + g) ^ key of token row 16 tb + n, key = n >> 1
  // (key < 8 touches bit 2 of the chunk index at most: even k-steps are chunk 4j + (g ^ key), odd ones 4 (j - 1) + ((4 | g) ^ key) -
  //  two lane addresses with the k-step as an immediate offset, not six)
  const int kr_key = n >> 1;
  const int kr_even = n * kKRow + ((g ^ kr_key) * 16), kr_odd = n * kKRow + (((4 | g) ^ kr_key) * 16);
  // transposing V reads: as in attention_prefill_bf16.hip
  const int vtr_j = (lane & 15) >> 2, vtr_c = lane & 3;
  const int vtr_row = (4 * g + vtr_j) * 256 + (vtr_c >> 1) * 16 + (vtr_c & 1) * 8;
  const int vtr_key = (2 * ((4 * g + vtr_j) & 7)) * 16;
  f32x4 o[kNB][8];
  float m_run[kNB], l_run[kNB];
#pragma unroll
  for (int nb = 0; nb < kNB; ++nb) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) o[nb][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    m_run[nb] = kNegInf;
    l_run[nb] = 0.f;
  }

  if (ntile > 0) {  // (a workgroup whose rows see no key - an empty context, a chunk longer than its keys - fetches nothing)
    fetch_k(0);
    fetch_v();
    stash_k(0);
    stash_v(0);
  }
  __syncthreads();
  int row_lim[kNB] = {0, 0};  // the last key a row sees; only the masked body reads it
  auto tile = [&](int t, auto masked_c) {
    constexpr bool masked = decltype(masked_c)::value != 0;
    const int buf = t & 1;
    const bool more = t + 1 < ntile;
    if (more) fetch_k(t + 1);
    const uint8_t* kt = s_k + buf * kKTileBytes;
    const uint8_t* vt = s_v + buf * kVTileBytes;

    // ---- S^T = K Q^T: six k-steps, the last two on the shared RoPE columns ----
    f32x4 s[kNB][4];
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) {
      Frag16 ka[kKSteps];
#pragma unroll
      for (int j = 0; j < kKSteps; ++j)
        ka[j].u = *reinterpret_cast<const u32x4*>(kt + tb * 16 * kKRow + ((j & 1) ? kr_odd + (j - 1) * 64 : kr_even + j * 64));
#pragma unroll
      for (int nb = 0; nb < kNB; ++nb) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kKSteps; ++j) {
          Frag16 qa;
          qa.u = qf[nb][j];
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[j].b, qa.b, acc, 0, 0, 0);
        }
        s[nb][tb] = acc;
      }
    }

    if (more) fetch_v();

    // ---- online softmax, base 2 ----
    uint32_t pf[kNB][2][4];
#pragma unroll
    for (int nb = 0; nb < kNB; ++nb) {
      float mt = kNegInf;
#pragma unroll
      for (int tb = 0; tb < 4; ++tb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = s[nb][tb][r];
          if (masked) {
            const int tok = t * 64 + tb * 16 + g * 4 + r;
            x = tok <= row_lim[nb] ? x : kNegInf;
            s[nb][tb][r] = x;
          }
          mt = fmaxf(mt, x);
        }
      mt *= a.scale_log2;  // scale > 0: max commutes with it
      mt = row4_max(mt);
      const float m_new = fmaxf(m_run[nb], mt);
      const float m_use = m_new == kNegInf ? 0.f : m_new;
      float psum = 0.f;
#pragma unroll
      for (int tb = 0; tb < 4; ++tb) {
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[r] = __builtin_amdgcn_exp2f(fmaf(s[nb][tb][r], a.scale_log2, -m_use));
          psum += p[r];
        }
        pf[nb][tb >> 1][(tb & 1) * 2] = pack_bf16x2(p[0], p[1]);
        pf[nb][tb >> 1][(tb & 1) * 2 + 1] = pack_bf16x2(p[2], p[3]);
      }
      rescale_if_max_moved(m_new, m_use, m_run[nb], l_run[nb], o[nb]);
      l_run[nb] += psum;
    }

    if (more) stash_k(buf ^ 1);

    // ---- O^T += V^T P^T: V^T operands straight out of LDS through ds_read_b64_tr_b16 ----
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        Frag16 va;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          const v4i16 tr = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_v4i16*>(
              static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_u8*)(vt + (2 * ks + hb) * 16 * 256 + vtr_row + ((u * 32) ^ vtr_key))))));
          const u32x2 t2 = __builtin_bit_cast(u32x2, tr);
          va.u[2 * hb] = t2[0];
          va.u[2 * hb + 1] = t2[1];
        }
#pragma unroll
        for (int nb = 0; nb < kNB; ++nb) {
          Frag16 pa;
          pa.u = u32x4{pf[nb][ks][0], pf[nb][ks][1], pf[nb][ks][2], pf[nb][ks][3]};
          o[nb][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va.b, pa.b, o[nb][u], 0, 0, 0);
        }
      }
    }
    if (more) stash_v(buf ^ 1);
    __syncthreads();
  };
  const int n_plain = min(ntile_full, ntile);
  for (int t = 0; t < n_plain; ++t) tile(t, IntC<0>{});
  {  // formed behind the unmasked loop from a lane id the compiler cannot trace back, so that nothing of it is carried (and
     // spilled) around that loop
    int lane_m = lane;
    asm volatile("" : "+v"(lane_m));
#pragma unroll
    for (int nb = 0; nb < kNB; ++nb) {
      const int pos = wg_pos0 + row0 + nb * 16 + (lane_m & 15);
      row_lim[nb] = pos < Sq ? (a.causal ? past + pos : L - 1) : -1;
    }
  }
  for (int t = n_plain; t < ntile; ++t) tile(t, IntC<1>{});

  // ---- finish (the staging LDS is free now: reuse it for the row-major re-read).  The lane's coordinates are taken afresh from
  // a lane id the compiler cannot trace back: the store addresses are then formed here, not hoisted above the tile loops and
  // spilled around them (0 scratch bytes) ----
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int n_e = lane_e & 15, g_e = lane_e >> 4;
  float (*s_o)[16][128 + 4] = reinterpret_cast<float (*)[16][128 + 4]>(s_raw);
  float (*s_l)[16] = reinterpret_cast<float (*)[16]>(s_raw + kWaves * 16 * (128 + 4) * 4);
#pragma unroll
  for (int nb = 0; nb < kNB; ++nb) {
    const float l = row4_sum(l_run[nb]);
    if (g_e == 0) {
      s_l[wave][n_e] = l;
      const int pos = wg_pos0 + row0 + nb * 16 + n_e;
      // m_run is the row's maximum in base-2 units on all four lanes of the row; l == 0 only when no key was seen (m = -inf)
      if (a.lse && pos < Sq)
        a.lse[static_cast<long>(q0 + pos) * a.num_head + h] = l > 0.f ? (m_run[nb] + __builtin_amdgcn_logf(l)) * kLn2 : kNegInf;
    }
#pragma unroll
    for (int jj = 0; jj < 8; ++jj)
#pragma unroll
      for (int r = 0; r < 4; ++r) s_o[wave][n_e][16 * jj + g_e * 4 + r] = o[nb][jj][r];
#pragma unroll 1
    for (int it = 0; it < 4; ++it) {
      const int row16 = it * 4 + g_e, c8 = n_e;
      const int pos = wg_pos0 + row0 + nb * 16 + row16;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(&s_o[wave][row16][c8 * 8]);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(&s_o[wave][row16][c8 * 8 + 4]);
      const float L2 = s_l[wave][row16];
      const float inv = L2 > 0.f ? 1.0f / L2 : 0.f;
      if (pos < Sq) {
        u32x4 pk;
        pk[0] = pack_bf16x2(x0[0] * inv, x0[1] * inv);
        pk[1] = pack_bf16x2(x0[2] * inv, x0[3] * inv);
        pk[2] = pack_bf16x2(x1[0] * inv, x1[1] * inv);
        pk[3] = pack_bf16x2(x1[2] * inv, x1[3] * inv);
        st16(a.y + (static_cast<long>(q0 + pos) * a.num_head + h) * 128 + c8 * 8, pk);
      }
    }
  }
}

}  // namespace prefill_mla
}  // namespace hpc

using namespace hpc;

// no reference kernel; the statement is tests/mla_prefill_ref.py
extern "C" int hpc_attention_prefill_mla_bf16_async(void* out, float* lse, const void* q, const void* k_nope, const void* k_pe,
                                                    const void* v, const int* cu_seqlens_q, const int* cu_seqlens_k, int num_batch,
                                                    int num_head, int max_seqlens_q, int max_seqlens_k, int64_t q_row_stride,
                                                    int64_t q_head_stride, int64_t k_row_stride, int64_t k_head_stride,
                                                    int64_t k_pe_row_stride, int64_t v_row_stride, int64_t v_head_stride,
                                                    float softmax_scale, int causal, hipStream_t stream) {
  using namespace hpc::prefill_mla;
  const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  const MlaPrefillRoute r = mla_prefill_route({addr(out), addr(q), addr(k_nope), addr(k_pe), addr(v), addr(cu_seqlens_q), addr(lse),
                                               addr(cu_seqlens_k), num_batch, num_head, max_seqlens_q, max_seqlens_k, q_row_stride,
                                               q_head_stride, k_row_stride, k_head_stride, k_pe_row_stride, v_row_stride, v_head_stride,
                                               softmax_scale});
  if (r.code != HPC_OK || r.empty) return r.code;
  const Args a{q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k ? cu_seqlens_k : cu_seqlens_q, static_cast<uint16_t*>(out), lse,
               num_head, causal ? 1 : 0, q_row_stride, q_head_stride, static_cast<int>(k_row_stride), static_cast<int>(k_pe_row_stride),
               static_cast<int>(v_row_stride), k_head_stride, v_head_stride, softmax_scale * 1.4426950408889634f};
  prefill_mla_bf16_kernel<<<dim3(r.grid_x, r.grid_y, r.grid_z), r.threads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
