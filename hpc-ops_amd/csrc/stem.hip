// Stem block-sparse mask generation for gfx950: the four stages that turn a paged FP8 prompt into the uint8 block mask
// of the block-sparse prefill (csrc/attention_prefill.hip).
//
//   prep_paged_kv  K: per (request, kv head, 128-token stem block) 16 strided group sums (tokens g, g+16, ..., g+112)
//                  of kscale * K, stored in REVERSED group order -> kflat bf16 [B, Hkv, max_Kb, 2048];
//                  V: per 16-token window the max row norm of vscale * V -> v_norm scratch, then a second small launch
//                  turns the per-(request, kv head) log-norm statistics into vbias f32 [B, Hkv, max_Kb].
//   prep_varlen_q  the same group sums of qscale * Q (natural group order) -> qflat bf16 [B, Hq, max_Qb, 2048].
//   oam_gemm       logits = qflat . kflat^T / 64 + vbias (K = 2048, bf16 MFMA, 128 x 128 tiles staged through LDS),
//                  -inf outside the request and above the causal block diagonal -> bf16 [B, Hq, max_Qb, max_Kb].
//   tpd            per row: budget, exact top-k threshold over 16-bit order keys (16-round bitwise search with
//                  ballot counts), fixed patterns -> uint8 mask [B, Hq, max_Qb, max_Kb].
//
// Replaces the reference's src/stem/stem_oam_prep_paged_kv_dim128.cu, stem_oam_prep_varlen_q_dim128.cu,
// stem_oam_gemm_dim128.cu and stem_tpd.cu (TMA / WGMMA / 32-lane warps there; wave64, LDS and MFMA here).
// Every output element is written by these kernels, padding included (zeros in kflat / qflat / vbias / mask, -inf in
// the logits), so no allocation needs a fill launch and the results are byte-deterministic.
#include "hpc_amd.h"
#include "hpc_common.h"

using namespace hpc;

namespace {

constexpr int kS = 128;           // stem block (tokens)
constexpr int kR = 16;            // stride = number of groups
constexpr int kN = kS / kR;       // samples per group (8)
constexpr int kD = 128;           // head dim
constexpr int kFlat = kR * kD;    // 2048: row length of qflat / kflat

__host__ __device__ __forceinline__ int cdiv(int a, int b) { return (a + b - 1) / b; }

// 16 e4m3 bytes times `sc`, accumulated into acc[0..15]
__device__ __forceinline__ void acc16(float (&acc)[16], u32x4 v, float sc) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    acc[4 * w + 0] += sc * e4m3_to_f32<0>(v[w]);
    acc[4 * w + 1] += sc * e4m3_to_f32<1>(v[w]);
    acc[4 * w + 2] += sc * e4m3_to_f32<2>(v[w]);
    acc[4 * w + 3] += sc * e4m3_to_f32<3>(v[w]);
  }
}

__device__ __forceinline__ void store_bf16x16(uint16_t* dst, const float (&acc)[16]) {
  u32x4 lo, hi;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lo[i] = pack_bf16x2(acc[2 * i], acc[2 * i + 1]);
    hi[i] = pack_bf16x2(acc[8 + 2 * i], acc[8 + 2 * i + 1]);
  }
  st16(dst, lo);
  st16(dst + 8, hi);
}

// ---- prep_paged_kv ------------------------------------------------------------------------------------------------
struct PrepKvArgs {
  uint16_t* kflat;
  float* v_norm;  // [B, Hkv, max_Kb * 8]
  const uint8_t* kcache;
  const uint8_t* vcache;
  const float* kscale;
  const float* vscale;
  const int* kv_indices;
  const int* kv_seq_lens;
  int quant_type, num_head_kv, page, ld_indices, max_kb;
  int64_t kbs, kts, khs, vbs, vts, vhs;  // cache strides (bytes = elements)
  int64_t ksb, ksr, ksh;                 // per-token kscale strides (fp32 elements), quant_type 0
};

// grid (max_Kb, Hkv, B), 256 threads: waves 0-1 build the 16 K group sums (lane = group-in-wave x 16-byte chunk),
// waves 2-3 the 8 window maxima of the V row norms (lane = token-in-8 x 16-byte chunk).  Every cache byte of the block
// is read once with 16-byte loads; tokens at or past kv_len read a clamped (valid) address and are zeroed.
__global__ __launch_bounds__(256) void stem_prep_kv_kernel(const PrepKvArgs a) {
  const int kb = blockIdx.x, h = blockIdx.y, req = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kv_len = a.kv_seq_lens[req];
  const int64_t row = (static_cast<int64_t>(req) * a.num_head_kv + h) * a.max_kb + kb;
  uint16_t* out = a.kflat + row * kFlat;
  if (kb >= cdiv(kv_len, kS)) {  // padding block: zeros (its v_norm entries are never read)
    st16(out + tid * 8, u32x4{0, 0, 0, 0});
    return;
  }
  const int* ids = a.kv_indices + static_cast<int64_t>(req) * a.ld_indices;
  const int c = lane & 7;
  if (wave < 2) {
    const int g = wave * 8 + (lane >> 3);
    u32x4 v[kN];
    float sc[kN];
#pragma unroll
    for (int s = 0; s < kN; ++s) {
      const int t = kb * kS + g + s * kR;
      const int tc = t < kv_len ? t : kv_len - 1;
      const int p = tc / a.page, r = tc - p * a.page;
      const int64_t phys = ids[p];
      v[s] = ld16(a.kcache + phys * a.kbs + r * a.kts + h * a.khs + c * 16);
      const float ks = a.quant_type == 1 ? a.kscale[0] : a.kscale[phys * a.ksb + (r >> 5) * a.ksr + h * a.ksh + (r & 31)];
      sc[s] = t < kv_len ? ks : 0.0f;
      if (t >= kv_len) v[s] = u32x4{0, 0, 0, 0};  // 0 * NaN must not leak from a clamped row
    }
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int s = 0; s < kN; ++s) acc16(acc, v[s], sc[s]);
    store_bf16x16(out + (kR - 1 - g) * kD + c * 16, acc);
  } else {
    const float vs = a.quant_type == 1 ? a.vscale[0] : a.vscale[h];
    const int tin = lane >> 3;
    float* vn = a.v_norm + row * kN;
#pragma unroll
    for (int wi = 0; wi < 4; ++wi) {
      const int w = (wave - 2) + 2 * wi;  // window: tokens [w*16, w*16+16) of the block
      u32x4 v[2];
      bool ok[2];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int t = kb * kS + w * kR + half * 8 + tin;
        const int tc = t < kv_len ? t : kv_len - 1;
        const int p = tc / a.page, r = tc - p * a.page;
        const int64_t phys = ids[p];
        v[half] = ld16(a.vcache + phys * a.vbs + r * a.vts + h * a.vhs + c * 16);
        ok[half] = t < kv_len;
      }
      float m = 0.0f;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        float ss = 0.0f;
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4) {
          const float x0 = vs * e4m3_to_f32<0>(v[half][w4]), x1 = vs * e4m3_to_f32<1>(v[half][w4]);
          const float x2 = vs * e4m3_to_f32<2>(v[half][w4]), x3 = vs * e4m3_to_f32<3>(v[half][w4]);
          ss += x0 * x0 + x1 * x1 + x2 * x2 + x3 * x3;
        }
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        ss += __shfl_xor(ss, 4, 64);
        m = fmaxf(m, ok[half] ? sqrtf(ss) : 0.0f);
      }
      m = wave_max(m);
      if (lane == 0) vn[w] = m;
    }
  }
}

// grid (Hkv, B), 256 threads: mean / sample std of l = log(v_norm + 1e-6) over the request's Kb*8 windows, then
// vbias[b] = lambda/8 * sum_s relu((l[8b+s] - mean) / (std + 1e-6)); zeros past the request's blocks.
__global__ __launch_bounds__(256) void stem_vbias_kernel(float* __restrict__ vbias, const float* __restrict__ v_norm,
                                                         const int* __restrict__ kv_seq_lens, int num_head_kv, int max_kb,
                                                         float lambda_mag) {
  __shared__ float red[4];
  const int h = blockIdx.x, req = blockIdx.y, tid = threadIdx.x;
  const int nkb = min(cdiv(kv_seq_lens[req], kS), max_kb), n = nkb * kN;
  const int64_t row = static_cast<int64_t>(req) * num_head_kv + h;
  const float* vn = v_norm + row * max_kb * kN;
  float* vb = vbias + row * max_kb;
  float s = 0.0f;
  for (int i = tid; i < n; i += 256) s += logf(vn[i] + 1e-6f);
  const float mean = n > 0 ? block_sum(s, red) / static_cast<float>(n) : 0.0f;
  float q = 0.0f;
  for (int i = tid; i < n; i += 256) {
    const float d = logf(vn[i] + 1e-6f) - mean;
    q += d * d;
  }
  q = n > 0 ? block_sum(q, red) : 0.0f;
  const float sd = n > 1 ? sqrtf(q / static_cast<float>(n - 1)) : 0.0f;
  const float inv = 1.0f / (sd + 1e-6f);
  for (int b = tid; b < max_kb; b += 256) {
    float acc = 0.0f;
    if (b < nkb) {
#pragma unroll
      for (int j = 0; j < kN; ++j) acc += fmaxf((logf(vn[b * kN + j] + 1e-6f) - mean) * inv, 0.0f);
      acc *= lambda_mag / static_cast<float>(kN);
    }
    vb[b] = acc;
  }
}

// ---- prep_varlen_q -------------------------------------------------------------------------------------------------
struct PrepQArgs {
  uint16_t* qflat;
  const uint8_t* q;
  const float* qscale;
  const int* q_seq_lens;
  const int* cu_seqlens_q;
  int num_head_q, max_qb;
  int64_t ldq, qsb, qsh;  // q row stride (bytes), qscale batch / head strides (fp32 elements)
};

// grid (max_Qb, Hq, B), 128 threads: lane = group (16) x 16-byte chunk (8); eight 16-byte loads in flight per lane.
__global__ __launch_bounds__(128) void stem_prep_q_kernel(const PrepQArgs a) {
  const int qb = blockIdx.x, h = blockIdx.y, req = blockIdx.z, tid = threadIdx.x;
  const int q_len = a.q_seq_lens[req];
  uint16_t* out = a.qflat + ((static_cast<int64_t>(req) * a.num_head_q + h) * a.max_qb + qb) * kFlat;
  if (qb >= cdiv(q_len, kS)) {
    st16(out + tid * 16, u32x4{0, 0, 0, 0});
    st16(out + tid * 16 + 8, u32x4{0, 0, 0, 0});
    return;
  }
  const int g = tid >> 3, c = tid & 7;
  const int64_t base = a.cu_seqlens_q[req];
  const float* qs = a.qscale + req * a.qsb + h * a.qsh;
  u32x4 v[kN];
  float sc[kN];
#pragma unroll
  for (int s = 0; s < kN; ++s) {
    const int t = qb * kS + g + s * kR;
    const int tc = t < q_len ? t : q_len - 1;
    v[s] = ld16(a.q + (base + tc) * a.ldq + h * kD + c * 16);
    sc[s] = t < q_len ? qs[tc] : 0.0f;
    if (t >= q_len) v[s] = u32x4{0, 0, 0, 0};
  }
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
  for (int s = 0; s < kN; ++s) acc16(acc, v[s], sc[s]);
  store_bf16x16(out + g * kD + c * 16, acc);
}

// ---- oam_gemm ------------------------------------------------------------------------------------------------------
constexpr int kTM = 128, kTN = 128, kBK = 64, kLdsRow = kBK + 8;  // +16 B per LDS row: conflict-free ds_read_b128

struct GemmArgs {
  uint16_t* logits;
  const uint16_t* qflat;
  const uint16_t* kflat;
  const float* vbias;
  const int* q_seq_lens;
  const int* kv_seq_lens;
  int num_head_q, num_head_kv, max_qb, max_kb, causal;
};

// grid (ceil(max_Kb/128), ceil(max_Qb/128), B*Hq), 256 threads = 2 x 2 waves of 64 x 64 (2 x 2 mfma 32x32x16 bf16).
// A = qflat rows (q blocks), B = kflat rows (kv blocks); both tiles are [128 rows][64 k] bf16 per k-step, loaded as
// 16-byte row chunks into registers one step ahead and written to LDS behind the step's MFMAs.  A tile with no valid
// element (outside the request, or entirely above the causal block diagonal) skips the k-loop and stores -inf.
__global__ __launch_bounds__(256) void stem_oam_gemm_kernel(const GemmArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * kTM * kLdsRow];
  uint16_t* As = lds;
  uint16_t* Bs = lds + kTM * kLdsRow;
  const int tn = blockIdx.x, tm = blockIdx.y, bh = blockIdx.z;
  const int req = bh / a.num_head_q, hq = bh - req * a.num_head_q;
  const int hkv = hq / (a.num_head_q / a.num_head_kv);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int q_len = a.q_seq_lens[req], kv_len = a.kv_seq_lens[req];
  const int nqb = cdiv(q_len, kS), nkb = cdiv(kv_len, kS);
  const int off = (kv_len - q_len + kS - 1) / kS;
  const int m0 = tm * kTM, n0 = tn * kTN;
  uint16_t* out = a.logits + static_cast<int64_t>(bh) * a.max_qb * a.max_kb;
  const bool skip = m0 >= nqb || n0 >= nkb || (a.causal && min(m0 + kTM - 1, nqb - 1) + off < n0);
  constexpr uint16_t kNegInf = 0xff80;
  if (skip) {
    for (int i = tid; i < kTM * kTN; i += 256) {
      const int r = m0 + (i >> 7), cc = n0 + (i & 127);
      if (r < a.max_qb && cc < a.max_kb) out[static_cast<int64_t>(r) * a.max_kb + cc] = kNegInf;
    }
    return;
  }
  const uint16_t* Ag = a.qflat + (static_cast<int64_t>(bh) * a.max_qb) * kFlat;
  const uint16_t* Bg = a.kflat + ((static_cast<int64_t>(req) * a.num_head_kv + hkv) * a.max_kb) * kFlat;
  // staging: 128 rows x 8 chunks of 16 B per operand = 1024 chunks, 4 per thread
  u32x4 ra[4], rb[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + 256 * i, r = id >> 3, c = id & 7;
      const int qa = m0 + r, kbb = n0 + r;
      ra[i] = qa < a.max_qb ? ld16(Ag + static_cast<int64_t>(qa) * kFlat + k0 + c * 8) : u32x4{0, 0, 0, 0};
      rb[i] = kbb < a.max_kb ? ld16(Bg + static_cast<int64_t>(kbb) * kFlat + k0 + c * 8) : u32x4{0, 0, 0, 0};
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = tid + 256 * i, r = id >> 3, c = id & 7;
      st16(As + r * kLdsRow + c * 8, ra[i]);
      st16(Bs + r * kLdsRow + c * 8, rb[i]);
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
  const int fr = lane & 31, fh = lane >> 5;
  load(0);
  for (int k0 = 0; k0 < kFlat; k0 += kBK) {
    __syncthreads();  // previous step's fragment reads are done
    stage();
    __syncthreads();
    if (k0 + kBK < kFlat) load(k0 + kBK);
#pragma unroll
    for (int ks = 0; ks < kBK / 16; ++ks) {
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(As + (wm * 64 + i * 32 + fr) * kLdsRow + ks * 16 + fh * 8));
        bf[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(Bs + (wn * 64 + i * 32 + fr) * kLdsRow + ks * 16 + fh * 8));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }
  // epilogue: C/D of 32x32: column = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
  const float* vb = a.vbias + (static_cast<int64_t>(req) * a.num_head_kv + hkv) * a.max_kb;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wn * 64 + j * 32 + fr;
    if (col >= a.max_kb) continue;
    const float bias = col < nkb ? vb[col] : 0.0f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
        if (r >= a.max_qb) continue;
        const bool valid = r < nqb && col < nkb && !(a.causal && r + off < col);
        const uint16_t v = valid ? static_cast<uint16_t>(pack_bf16x2(acc[i][j][e] * (1.0f / 64.0f) + bias, 0.0f) & 0xffffu)
                                 : kNegInf;
        out[static_cast<int64_t>(r) * a.max_kb + col] = v;
      }
  }
}

// ---- tpd -----------------------------------------------------------------------------------------------------------
struct TpdArgs {
  uint8_t* mask;
  const uint16_t* logits;
  const int* q_seq_lens;
  const int* kv_seq_lens;
  const int* num_prompt_tokens;
  int num_heads, max_qb, max_kb, block_size, initial_blocks, window_size, bias_medium, bias_large;
  float alpha, rate_medium, rate_large;
  int64_t rows;
};

// Per-row budget; float32 operations one at a time (no contraction), in the order the contract states.
__device__ __forceinline__ int tpd_budget(int q_pos, int P, const TpdArgs& a) {
  int k;
  if (P < 56) k = P;
  else if (P < 160) k = static_cast<int>(__fmul_rn(static_cast<float>(P), a.rate_medium)) + a.bias_medium;
  else k = static_cast<int>(__fmul_rn(static_cast<float>(P), a.rate_large)) + a.bias_large;
  const int decay = P - k;
  if (q_pos < k || decay <= 1) return k;
  const float kf = static_cast<float>(k);
  const float k_end = __fmul_rn(kf, a.alpha);
  const float t = __fdiv_rn(static_cast<float>(q_pos - k), static_cast<float>(decay - 1));
  const int b = static_cast<int>(floorf(__fadd_rn(kf, __fmul_rn(t, __fsub_rn(k_end, kf)))));
  return b < 1 ? 1 : (b > k ? k : b);
}

// bf16 bits -> 16-bit order key; non-finite -> 0x007f (below every finite key, which are >= 0x0080)
__device__ __forceinline__ uint32_t order_key(uint32_t bits) {
  if ((bits & 0x7f80u) == 0x7f80u) return 0x7fu;
  return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits ^ 0x8000u);
}

// kWaves waves per row (one row per wave when 1, four rows per 256-thread block); element j of thread i is column
// j * (64 * kWaves) + i.  Counts are ballots: one wave-uniform popcount per element, summed over the waves in LDS.
template <int kEPT, int kWaves>
__global__ __launch_bounds__(kWaves == 1 ? 256 : 64 * kWaves) void stem_tpd_kernel(const TpdArgs a) {
  __shared__ int red[2][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row_id = kWaves == 1 ? static_cast<int64_t>(blockIdx.x) * 4 + wave : blockIdx.x;
  if (row_id >= a.rows) return;  // kWaves == 1 only (whole waves; no block barrier there)
  const int tid = kWaves == 1 ? lane : threadIdx.x;
  constexpr int kThr = 64 * kWaves;
  const int req = static_cast<int>(row_id / (static_cast<int64_t>(a.num_heads) * a.max_qb));
  const int row = static_cast<int>(row_id % a.max_qb);
  const uint16_t* lrow = a.logits + row_id * a.max_kb;
  uint8_t* mrow = a.mask + row_id * a.max_kb;
  const int q_len = a.q_seq_lens[req], kv_len = a.kv_seq_lens[req];
  const int nqb = cdiv(q_len, a.block_size), nkb = min(cdiv(kv_len, a.block_size), a.max_kb);
  if (row >= nqb) {
#pragma unroll
    for (int j = 0; j < kEPT; ++j) {
      const int col = j * kThr + tid;
      if (col < a.max_kb) mrow[col] = 0;
    }
    return;
  }
  uint32_t key[kEPT];
#pragma unroll
  for (int j = 0; j < kEPT; ++j) {
    const int col = j * kThr + tid;
    key[j] = col < nkb ? order_key(lrow[col]) : 0u;
  }
  auto count_ge = [&](uint32_t cand, int round) -> int {
    int n = 0;
#pragma unroll
    for (int j = 0; j < kEPT; ++j) n += __popcll(__ballot(key[j] >= cand));
    if (kWaves == 1) return n;
    if (lane == 0) red[round & 1][wave] = n;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) tot += red[round & 1][w];
    return tot;
  };
  const int nfinite = count_ge(0x80u, 0);
  const int off = (kv_len - q_len + a.block_size - 1) / a.block_size;
  const int P = cdiv(a.num_prompt_tokens[req], a.block_size);
  const int budget = tpd_budget(row + off, P, a);
  uint32_t T = 0x80u;
  if (budget < nfinite) {
    T = 0;
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t cand = T | (1u << bit);
      if (count_ge(cand, 16 - bit) >= budget) T = cand;
    }
  }
  const int diag = min(row + off, nkb - 1);
#pragma unroll
  for (int j = 0; j < kEPT; ++j) {
    const int col = j * kThr + tid;
    if (col < a.max_kb) {
      const bool sel = col < nkb && (key[j] >= T || col < a.initial_blocks ||
                                     (col > diag - a.window_size && col <= diag) || col == diag);
      mrow[col] = sel ? 1 : 0;
    }
  }
}

template <int kEPT, int kWaves>
void launch_tpd(const TpdArgs& a, hipStream_t st) {
  const unsigned grid = kWaves == 1 ? static_cast<unsigned>((a.rows + 3) / 4) : static_cast<unsigned>(a.rows);
  stem_tpd_kernel<kEPT, kWaves><<<grid, kWaves == 1 ? 256 : 64 * kWaves, 0, st>>>(a);
}

}  // namespace

extern "C" int hpc_stem_oam_prep_paged_kv_async(
    void* kflat, void* vbias, void* v_norm, const void* kcache, const void* vcache, const void* kscale,
    const void* vscale, const void* kv_indices, const void* kv_seq_lens, int quant_type, int num_batch, int num_dim_qk,
    int num_dim_v, int num_head_kv, int block_size, int num_seq_max_blocks, int stem_block_size, int stem_stride,
    int max_num_stem_blocks, float lambda_mag, int64_t kcache_block_stride, int64_t kcache_token_stride,
    int64_t kcache_head_stride, int64_t vcache_block_stride, int64_t vcache_token_stride, int64_t vcache_head_stride,
    int64_t kscale_block_stride, int64_t kscale_row_stride, int64_t kscale_head_stride, hpc_stream_t stream) {
  if (stem_block_size != kS || stem_stride != kR || num_dim_qk != kD || num_dim_v != kD) return HPC_ERR_UNSUPPORTED;
  if ((block_size != 32 && block_size != 64) || (quant_type != 0 && quant_type != 1)) return HPC_ERR_UNSUPPORTED;
  if (!kflat || !vbias || !v_norm || !kcache || !vcache || !kscale || !vscale || !kv_indices || !kv_seq_lens ||
      num_batch < 0 || num_head_kv <= 0 || max_num_stem_blocks < 0)
    return HPC_ERR_INVALID;
  if (num_batch == 0 || max_num_stem_blocks == 0) return HPC_OK;
  PrepKvArgs a{static_cast<uint16_t*>(kflat), static_cast<float*>(v_norm), static_cast<const uint8_t*>(kcache),
               static_cast<const uint8_t*>(vcache), static_cast<const float*>(kscale), static_cast<const float*>(vscale),
               static_cast<const int*>(kv_indices), static_cast<const int*>(kv_seq_lens), quant_type, num_head_kv,
               block_size, num_seq_max_blocks, max_num_stem_blocks, kcache_block_stride, kcache_token_stride,
               kcache_head_stride, vcache_block_stride, vcache_token_stride, vcache_head_stride, kscale_block_stride,
               kscale_row_stride, kscale_head_stride};
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  stem_prep_kv_kernel<<<dim3(max_num_stem_blocks, num_head_kv, num_batch), 256, 0, st>>>(a);
  stem_vbias_kernel<<<dim3(num_head_kv, num_batch), 256, 0, st>>>(static_cast<float*>(vbias), a.v_norm, a.kv_seq_lens,
                                                                 num_head_kv, max_num_stem_blocks, lambda_mag);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

extern "C" int hpc_stem_oam_prep_varlen_q_async(void* qflat, const void* q_fp8, const void* qscale,
                                                const void* q_seq_lens, const void* cu_seqlens_q, int num_batch,
                                                int num_head_q, int num_dim_qk, int stem_block_size, int stem_stride,
                                                int max_num_q_blocks, int64_t ldQ, int64_t qscale_batch_stride,
                                                int64_t qscale_head_stride, hpc_stream_t stream) {
  if (stem_block_size != kS || stem_stride != kR || num_dim_qk != kD) return HPC_ERR_UNSUPPORTED;
  if (!qflat || !q_fp8 || !qscale || !q_seq_lens || !cu_seqlens_q || num_batch < 0 || num_head_q <= 0 ||
      max_num_q_blocks < 0 || ldQ % 16 != 0)
    return HPC_ERR_INVALID;
  if (num_batch == 0 || max_num_q_blocks == 0) return HPC_OK;
  PrepQArgs a{static_cast<uint16_t*>(qflat), static_cast<const uint8_t*>(q_fp8), static_cast<const float*>(qscale),
              static_cast<const int*>(q_seq_lens), static_cast<const int*>(cu_seqlens_q), num_head_q, max_num_q_blocks,
              ldQ, qscale_batch_stride, qscale_head_stride};
  stem_prep_q_kernel<<<dim3(max_num_q_blocks, num_head_q, num_batch), 128, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

extern "C" int hpc_stem_oam_gemm_async(void* block_logits, const void* qflat, const void* kflat, const void* vbias,
                                       const void* q_seq_lens, const void* kv_seq_lens, int num_batch, int num_head_q,
                                       int num_head_kv, int max_num_qb, int max_num_kb, int stem_block_size,
                                       int stem_stride, int causal, hpc_stream_t stream) {
  if (stem_block_size != kS || stem_stride != kR) return HPC_ERR_UNSUPPORTED;
  if (!block_logits || !qflat || !kflat || !vbias || !q_seq_lens || !kv_seq_lens || num_batch < 0 || num_head_q <= 0 ||
      num_head_kv <= 0 || num_head_q % num_head_kv != 0 || max_num_qb < 0 || max_num_kb < 0)
    return HPC_ERR_INVALID;
  if (num_batch == 0 || max_num_qb == 0 || max_num_kb == 0) return HPC_OK;
  GemmArgs a{static_cast<uint16_t*>(block_logits), static_cast<const uint16_t*>(qflat),
             static_cast<const uint16_t*>(kflat), static_cast<const float*>(vbias),
             static_cast<const int*>(q_seq_lens), static_cast<const int*>(kv_seq_lens), num_head_q, num_head_kv,
             max_num_qb, max_num_kb, causal ? 1 : 0};
  const dim3 grid(cdiv(max_num_kb, kTN), cdiv(max_num_qb, kTM), num_batch * num_head_q);
  stem_oam_gemm_kernel<<<grid, 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

extern "C" int hpc_stem_tpd_async(void* mask, const void* block_logits, const void* q_seq_lens, const void* kv_seq_lens,
                                  const void* num_prompt_tokens, int num_batch, int num_heads, int max_Qb, int max_Kb,
                                  int block_size, float alpha, int initial_blocks, int window_size,
                                  float k_block_num_rate_medium, int k_block_num_bias_medium,
                                  float k_block_num_rate_large, int k_block_num_bias_large, hpc_stream_t stream) {
  if (max_Kb > 32768) return HPC_ERR_UNSUPPORTED;
  if (!mask || !block_logits || !q_seq_lens || !kv_seq_lens || !num_prompt_tokens || num_batch < 0 || num_heads < 0 ||
      max_Qb < 0 || max_Kb < 0 || block_size <= 0)
    return HPC_ERR_INVALID;
  const int64_t rows = static_cast<int64_t>(num_batch) * num_heads * max_Qb;
  if (rows == 0 || max_Kb == 0) return HPC_OK;
  TpdArgs a{static_cast<uint8_t*>(mask), static_cast<const uint16_t*>(block_logits),
            static_cast<const int*>(q_seq_lens), static_cast<const int*>(kv_seq_lens),
            static_cast<const int*>(num_prompt_tokens), num_heads, max_Qb, max_Kb, block_size, initial_blocks,
            window_size, k_block_num_bias_medium, k_block_num_bias_large, alpha, k_block_num_rate_medium,
            k_block_num_rate_large, rows};
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (max_Kb <= 64) launch_tpd<1, 1>(a, st);
  else if (max_Kb <= 128) launch_tpd<2, 1>(a, st);
  else if (max_Kb <= 256) launch_tpd<4, 1>(a, st);
  else if (max_Kb <= 512) launch_tpd<8, 1>(a, st);
  else if (max_Kb <= 1024) launch_tpd<16, 1>(a, st);
  else if (max_Kb <= 2048) launch_tpd<8, 4>(a, st);
  else if (max_Kb <= 4096) launch_tpd<16, 4>(a, st);
  else if (max_Kb <= 8192) launch_tpd<32, 4>(a, st);
  else if (max_Kb <= 16384) launch_tpd<16, 16>(a, st);
  else launch_tpd<32, 16>(a, st);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
