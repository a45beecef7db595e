// Fused sampler: repetition penalty -> temperature -> [softmax] -> top-k -> [softmax] -> top-p ->
// Gumbel-max -> penalty write-back, and the temperature-only fast path - gfx950.
//
// Replaces reference src/sampler/fused_sampler.cu (cluster-cooperative BlockRadixSort top-K, :161-296,
// launcher :700-775), src/sampler/fused_sampler_temperature.cu and src/sampler/sampler_rng.cuh.
//
// MI355X design.  A decode step samples B <= a few hundred rows of V ~ 1.2e5 logits: 0.5 MB per row,
// nowhere near an HBM problem - it is a latency problem, so a row is spread over S >= 16 workgroups
// and the selection is EXACT but cheap:
//   phase 1 (grid S x B): each thread keeps its <= 32 elements of the segment in registers as
//     order-preserving integer keys.  The K-th largest of the 256 per-thread maxima is a lower bound
//     of the segment's K-th largest element, so only the (typically ~K..2K) elements above it are
//     compacted into an LDS list; a byte-wise radix select over 52-bit composites (key << 20 | ~index -
//     all distinct, ties resolved towards the smaller token id) picks the segment's top K.  There is
//     no sort and no atomics storm: histograms only ever see the short lists.
//   phase 2 (grid B): radix select over the S*K candidates, one wave bitonic-sorts the K winners (one
//     per lane) and runs softmax / top-p / Gumbel-max / tie-break exactly in the order of the
//     reference's PyTorch model (tests/test_sampler.py:47-165); lane 0 writes the token and ORs the
//     penalty bit.
// The fast path (temperature only) is a two-step arg-max of logits / T + Gumbel noise.
// Self-drawn noise: Philox-4x32-10 keyed by the caller's seed, counter = (token, row, launch offset).
// Draft-token verification of a speculative step (hpc_speculative_verify_async) is the fast path's segment pass plus the
// segment's softmax statistics, and a one-wave accept scan per request.  Both passes score a token with score_composite,
// so speculative_verify returns bit for bit the token the fast path returns for the same row, noise and draft.
// The log-probability, rank and top-N of a row's token (hpc_token_logprobs_async) are the verification's segment pass
// without the noise plus a count of larger composites, and the top-k selection above on torch_topk_key composites.
// Ordered keys, (key, index) composites and the 64-bit wave operations: ordered_key.h.
#include "ordered_key.h"
#include "../../include/hpc_amd.h"

#include <atomic>

namespace hpc {
namespace sampler {

constexpr int kThreads = 256;
constexpr int kSegMax = 8192;   // elements of one segment (32 per thread)
constexpr int kElems = kSegMax / kThreads;
constexpr int kIdxBits = 20;    // token ids < 2^20
constexpr uint64_t kIdxMask = (1ull << kIdxBits) - 1;
constexpr int kSelBytes = 7;    // 52-bit composites
constexpr float kNegInf = -__builtin_inff();

struct Args {
  const void* logits;
  int dtype;  // 0 fp32, 1 bf16
  long row_stride;
  int B, V, S, seg;
  uint8_t* mask;
  long mask_stride;
  const int* slot;
  const float* rp_arr;
  float rp_val;
  const float* t_arr;
  float t_val;
  int policy;
  const void* topk_ptr;
  int topk_bytes, topk_val;
  const float* topp_arr;
  float topp_val;
  const float* noise;
  const int64_t* draft;
  int max_topk;
  uint64_t seed, offset;
  int* out;
  uint64_t* cand;    // [B][S][K] composites
  float* seg_stat;   // [B][S][2]: max, sum exp(x - max)   (softmax-before-topk only)
};

__device__ __forceinline__ uint64_t comp_of(uint32_t key, uint32_t idx) {
  return (static_cast<uint64_t>(key) << kIdxBits) | (kIdxMask - idx);
}

// ---- Philox-4x32-10 ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t philox_word0(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}
// Gumbel(0) noise for (row, token): g = -log(max(-log(U), 1e-20)), U in (0, 1]  (reference sampler_rng.cuh:34-38)
__device__ __forceinline__ float own_gumbel(const Args& a, int b, int idx) {
  const uint32_t w = philox_word0(a.seed, static_cast<uint32_t>(idx), static_cast<uint32_t>(b),
                                  static_cast<uint32_t>(a.offset), static_cast<uint32_t>(a.offset >> 32));
  const float u = (static_cast<float>(w >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
  return -logf(fmaxf(-logf(u), 1e-20f));
}

__device__ __forceinline__ float load_logit(const Args& a, int b, int i) {
  if (a.dtype == 0) return static_cast<const float*>(a.logits)[static_cast<long>(b) * a.row_stride + i];
  const uint16_t h = static_cast<const uint16_t*>(a.logits)[static_cast<long>(b) * a.row_stride + i];
  return __uint_as_float(static_cast<uint32_t>(h) << 16);
}

// The fast path's score of token i of row `row` as a composite: x = logit / T (the logit itself when greedy), the row's
// draft at -inf, plus Gumbel noise unless greedy.  temperature_segment_kernel and verify_segment_kernel both take their
// arg-max over THIS function, which is what makes speculative_verify return exactly the token that
// fused_sampler_temperature_sample(..., draft_token_ids = d) returns.
__device__ __forceinline__ void score_composite(const Args& a, int row, int i, float x, bool is_draft, bool greedy, uint64_t& c) {
  if (is_draft) x = kNegInf;
  if (!greedy) x += a.noise ? a.noise[static_cast<long>(row) * a.V + i] : own_gumbel(a, row, i);
  c = composite_of(ieee_key(x), static_cast<uint32_t>(i));
}

// ---- byte-wise radix select: the K-th largest of n distinct composites in `list` (LDS) ---------------
// All 256 threads call it; n > K.  hist: 256 counters, misc: ints 0, 1 and 4 are used here.
__device__ uint64_t select_kth(const uint64_t* list, int n, int K, unsigned* hist, int* misc) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint64_t prefix = 0, mask = 0;
  int need = K;
  for (int p = kSelBytes - 1; p >= 0; --p) {
    hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      const uint64_t c = list[i];
      if ((c & mask) == prefix) atomicAdd(&hist[(c >> (8 * p)) & 255], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // digit d with count(> d) < need <= count(>= d)
      unsigned h[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) h[j] = hist[4 * lane + j];
      const unsigned mine = h[0] + h[1] + h[2] + h[3];
      unsigned incl = mine;  // sum over lanes >= lane
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl += v;
      }
      unsigned gt = incl - mine;  // elements in higher lanes
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        if (gt < static_cast<unsigned>(need) && static_cast<unsigned>(need) <= gt + h[j]) {
          misc[0] = 4 * lane + j;
          misc[1] = need - static_cast<int>(gt);
          misc[4] = static_cast<unsigned>(need) == gt + h[j];  // the whole bin is wanted: no need to refine it
        }
        gt += h[j];
      }
    }
    __syncthreads();
    prefix |= static_cast<uint64_t>(misc[0]) << (8 * p);
    mask |= 255ull << (8 * p);
    need = misc[1];
    // early exit (the usual case after the 3-4 bytes that carry the float value): every element of the
    // chosen bin belongs to the top K, so the bin's lower bound is already the threshold
    if (misc[4]) break;
  }
  return prefix;
}

// ---- phase 1: per-segment top-K candidates ------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sampler_segment_kernel(const Args a) {
  __shared__ uint64_t s_list[kSegMax];
  __shared__ unsigned s_hist[256];
  __shared__ int s_misc[6];
  __shared__ float s_red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, b = blockIdx.y;
  const int K = a.max_topk;
  const int i0 = s * a.seg, i1 = min(a.V, i0 + a.seg);
  const int n = max(i1 - i0, 0);

  float rp = a.rp_arr ? a.rp_arr[b] : a.rp_val;
  const bool has_rp = a.mask && rp > 0.f;
  const float inv_rp = has_rp ? static_cast<float>(1.0 / static_cast<double>(rp)) : 1.f;
  const float temp = a.t_arr ? a.t_arr[b] : a.t_val;
  const uint8_t* mrow = a.mask ? a.mask + static_cast<long>(a.slot[b]) * a.mask_stride : nullptr;

  uint32_t key[kElems];
  uint32_t best = 0;
#pragma unroll
  for (int j = 0; j < kElems; ++j) {
    const int i = i0 + j * kThreads + tid;
    key[j] = 0;
    if (i < i1) {
      float x = load_logit(a, b, i);
      if (has_rp && ((mrow[i >> 3] >> (i & 7)) & 1)) x = x > 0.f ? x * inv_rp : x * rp;
      if (temp > 0.f) x = x / temp;
      key[j] = ieee_key(x);
      best = max(best, key[j]);
    }
  }

  // softmax-before-topk statistics of the segment (max, sum exp(x - max))
  if (a.policy == 1) {
    float m = best ? ieee_key_value(best) : kNegInf;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) s_red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    // a segment whose logits are all -inf (grammar / vocabulary masks) must contribute (max = -inf,
    // sum = 0), not exp(-inf - (-inf)) = NaN: subtract 0 instead of the -inf maximum
    const float m_sub = m == kNegInf ? 0.f : m;
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < kElems; ++j)
      if (key[j]) e += expf(ieee_key_value(key[j]) - m_sub);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
    if (lane == 0) s_red[4 + wave] = e;
    __syncthreads();
    if (tid == 0) {
      float* st = a.seg_stat + (static_cast<long>(b) * a.S + s) * 2;
      st[0] = m;
      st[1] = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
    }
  }

  // lower bound of the K-th largest element: the K-th largest per-thread maximum
  uint32_t bound = 0;
  if (n > K) {
    s_list[tid] = comp_of(best, tid);
    __syncthreads();
    bound = static_cast<uint32_t>(select_kth(s_list, kThreads, K, s_hist, s_misc) >> kIdxBits);
  }
  if (tid == 0) s_misc[2] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kElems; ++j) {
    if (key[j] && key[j] >= bound) {
      const int pos = atomicAdd(&s_misc[2], 1);
      s_list[pos] = comp_of(key[j], i0 + j * kThreads + tid);
    }
  }
  __syncthreads();
  const int cnt = s_misc[2];
  uint64_t thr = 0;
  if (cnt > K) thr = select_kth(s_list, cnt, K, s_hist, s_misc);
  if (tid == 0) s_misc[3] = 0;
  __syncthreads();
  uint64_t* out = a.cand + (static_cast<long>(b) * a.S + s) * K;
  for (int i = tid; i < cnt; i += kThreads) {
    const uint64_t c = s_list[i];
    if (c >= thr) out[atomicAdd(&s_misc[3], 1)] = c;
  }
  __syncthreads();
  // fewer than K elements: pad with distinct composites below every real one (key part 0)
  for (int i = min(cnt, K) + tid; i < K; i += kThreads) out[i] = static_cast<uint64_t>(s * K + i);
}

// ---- phase 2: merge, sort the K winners, sample ---------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sampler_final_kernel(const Args a) {
  __shared__ uint64_t s_list[kSegMax];
  __shared__ uint64_t s_sel[64];
  __shared__ unsigned s_hist[256];
  __shared__ int s_misc[6];
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x;
  const int K = a.max_topk;
  const int n = a.S * K;
  const uint64_t* cand = a.cand + static_cast<long>(b) * n;
  for (int i = tid; i < n; i += kThreads) s_list[i] = cand[i];
  if (tid < 64) s_sel[tid] = 0;
  if (tid == 0) s_misc[2] = 0;
  __syncthreads();
  uint64_t thr = 0;
  if (n > K) thr = select_kth(s_list, n, K, s_hist, s_misc);
  for (int i = tid; i < n; i += kThreads) {
    const uint64_t c = s_list[i];
    if (c >= thr) s_sel[atomicAdd(&s_misc[2], 1)] = c;
  }
  __syncthreads();
  if (tid >= 64) return;

  // ---- one wave: bitonic sort (descending) of one composite per lane --------------------------------------
  uint64_t c = s_sel[lane];
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint64_t o = shfl_xor_u64(c, j);
      const bool up = (lane & k) != 0;       // this block sorts ascending
      const bool lower = (lane & j) == 0;    // lane holds the lower position of the pair
      const bool take_max = (lower != up);   // descending blocks keep the max in the lower lane
      c = take_max ? (c > o ? c : o) : (c < o ? c : o);
    }
  const uint32_t key = static_cast<uint32_t>(c >> kIdxBits);
  const int tok = static_cast<int>(kIdxMask - (c & kIdxMask));
  const bool real = key != 0;
  const float x = real ? ieee_key_value(key) : kNegInf;

  int kb = a.topk_ptr ? (a.topk_bytes == 8 ? static_cast<int>(static_cast<const int64_t*>(a.topk_ptr)[b])
                                           : static_cast<const int*>(a.topk_ptr)[b])
                      : a.topk_val;
  if (kb <= 0 || kb > K) kb = K;
  const bool in_k = lane < kb && real;
  const float tp = a.topp_arr ? a.topp_arr[b] : a.topp_val;

  float p = 0.f, g = x;
  if (a.policy == 2) {  // softmax over the surviving top-k
    const float m = __shfl(x, 0, 64);
    float e = in_k ? expf(x - m) : 0.f;
    float sum = e;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    p = e / sum;
    g = logf(p);
  } else if (a.policy == 1) {  // probabilities of the full-vocabulary softmax
    float gm = kNegInf;
    for (int s = 0; s < a.S; ++s) gm = fmaxf(gm, a.seg_stat[(static_cast<long>(b) * a.S + s) * 2]);
    float gs = 0.f;
    for (int s = 0; s < a.S; ++s) {
      const float* st = a.seg_stat + (static_cast<long>(b) * a.S + s) * 2;
      gs += st[1] * expf(st[0] - gm);
    }
    p = in_k ? expf(x - gm) / gs : 0.f;
    g = p > 0.f ? logf(p) : kNegInf;
  }
  bool keep = in_k;
  if (tp > 0.f) {
    // cumulative probability in rank order, summed serially like the PyTorch model (cumsum - p)
    float cum = 0.f, mine_excl = 0.f;
    for (int i = 0; i < kb; ++i) {
      const float pi = __shfl(p, i, 64);
      cum += pi;
      if (lane == i) mine_excl = cum - pi;
    }
    keep = in_k && (lane == 0 || mine_excl < tp);
  }
  const float noise = in_k ? (a.noise ? a.noise[static_cast<long>(b) * a.V + tok] : own_gumbel(a, b, tok)) : 0.f;
  float score = keep ? g + noise : kNegInf;
  float best = score;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
  // ties (and the all -inf row) resolve towards the smaller token id among the top-k entries
  int cand_tok = (in_k && score == best) ? tok : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cand_tok = min(cand_tok, __shfl_xor(cand_tok, o, 64));
  if (cand_tok == 0x7fffffff) cand_tok = __shfl(tok, 0, 64);
  if (lane == 0) {
    a.out[b] = cand_tok;
    if (a.mask) {
      uint8_t* row = a.mask + static_cast<long>(a.slot[b]) * a.mask_stride;
      const uintptr_t addr = reinterpret_cast<uintptr_t>(row + (cand_tok >> 3));
      atomicOr(reinterpret_cast<unsigned*>(addr & ~uintptr_t(3)), (1u << (cand_tok & 7)) << (8 * (addr & 3)));
    }
  }
}

// ---- temperature-only fast path: argmax(logits / T + gumbel) ---------------------------------------------
// The wave maxima of these two kernels are wave_max_u64 spelled out: as a call the registers are allocated differently.
__global__ __launch_bounds__(kThreads) void temperature_segment_kernel(const Args a) {
  __shared__ uint64_t s_red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, b = blockIdx.y;
  const int i0 = s * a.seg, i1 = min(a.V, i0 + a.seg);
  const float temp = a.t_arr ? a.t_arr[b] : a.t_val;
  const int64_t dr = a.draft ? a.draft[b] : -1;
  uint64_t best = 0;
  for (int i = i0 + tid; i < i1; i += kThreads) {
    uint64_t c;
    score_composite(a, b, i, load_logit(a, b, i) / temp, static_cast<int64_t>(i) == dr, false, c);
    best = c > best ? c : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(best), o, 64);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(best >> 32), o, 64);
    const uint64_t v = (static_cast<uint64_t>(hi) << 32) | lo;
    best = v > best ? v : best;
  }
  if (lane == 0) s_red[wave] = best;
  __syncthreads();
  if (tid == 0) {
    uint64_t m = s_red[0];
    for (int w = 1; w < 4; ++w) m = s_red[w] > m ? s_red[w] : m;
    a.cand[static_cast<long>(b) * a.S + s] = m;
  }
}

__global__ __launch_bounds__(64) void temperature_final_kernel(const Args a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  uint64_t best = 0;
  for (int s = lane; s < a.S; s += 64) {
    const uint64_t c = a.cand[static_cast<long>(b) * a.S + s];
    best = c > best ? c : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(best), o, 64);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(best >> 32), o, 64);
    const uint64_t v = (static_cast<uint64_t>(hi) << 32) | lo;
    best = v > best ? v : best;
  }
  if (lane == 0) a.out[b] = static_cast<int>(index_of(best));
}

// ---- draft-token verification of a speculative decode step (ours: no reference counterpart) -------------------------
// Rows are positions: row r = b * (K + 1) + j is position j of request b, and the temperature is per REQUEST.  Phase 1 is
// the fast path's segment pass - score_composite of x / T, the row's draft masked - that
// also keeps the segment's softmax statistics of x / T and the scaled logit at the draft; phase 2, one wave per request,
// folds the segments of every position, forms p = softmax(x / T)[draft] and finds the first rejection.  No atomics, no
// scratch, LDS only for the cross-wave reduction.
struct VerifyStat {  // one per (row, segment)
  uint64_t best;     // fast-path composite of the best score, draft masked
  float m, sum;      // max of x / T, sum exp(x / T - m)
};
struct VerifyArgs {
  Args a;                 // logits, dtype, row_stride, B = rows, V, S, seg, t_arr / t_val, noise, seed, offset, out
  const int64_t* draft;   // [requests][K]
  const float* uniform;   // [requests][K], null: drawn
  int K;
  int* num_accepted;      // [requests]
  VerifyStat* stat;       // [rows][S]
  float* xd;              // [rows]: x / T at the row's draft (x when greedy), written by the segment that owns it
};

// the uniform of row r: counter word 0 is all ones, a token id (< 2^20) never is
__device__ __forceinline__ float own_uniform(const Args& a, int r) {
  const uint32_t w = philox_word0(a.seed, 0xffffffffu, static_cast<uint32_t>(r), static_cast<uint32_t>(a.offset),
                                  static_cast<uint32_t>(a.offset >> 32));
  return static_cast<float>(w >> 8) * (1.0f / 16777216.0f);  // [0, 1)
}
// (m, s) <- the softmax statistics of the union of two sets; an empty set is (-inf, 0)
__device__ __forceinline__ void stat_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  const float sub = mx == kNegInf ? 0.f : mx;
  s = s * __expf(m - sub) + s2 * __expf(m2 - sub);
  m = mx;
}

__global__ __launch_bounds__(kThreads) void verify_segment_kernel(const VerifyArgs v) {
  __shared__ uint64_t s_best[4];
  __shared__ float s_m[4], s_s[4];
  const Args& a = v.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, r = blockIdx.y;
  const int b = r / (v.K + 1), j = r - b * (v.K + 1);
  // a row past the request's first invalid draft is not read (block-uniform)
  const int64_t* drow = v.draft + static_cast<long>(b) * v.K;
  for (int t = 0; t < j; ++t) {
    const int64_t d = drow[t];
    if (d < 0 || d >= a.V) return;
  }
  int64_t dr = -1;  // the bonus row (j == n_b) has no mask
  if (j < v.K) {
    const int64_t d = drow[j];
    if (d >= 0 && d < a.V) dr = d;
  }
  const float temp = a.t_arr ? a.t_arr[b] : a.t_val;
  const bool greedy = !(temp > 0.f);
  const int i0 = s * a.seg, i1 = min(a.V, i0 + a.seg);

  // every load of the segment is issued before the first use: a decode step has few rows, and a thread that waited for
  // each element in turn would spend the pass on memory latency.  Out-of-range slots read the segment's last element
  // (an empty segment reads nothing) and are set to -inf.
  float xs[kElems];
  const int last = i1 - 1;
  if (i0 >= i1) {
#pragma unroll
    for (int e = 0; e < kElems; ++e) xs[e] = 0.f;
  } else if (a.dtype == 0) {  // one branch per dtype, so that no load waits for a conversion
#pragma unroll
    for (int e = 0; e < kElems; ++e) xs[e] = load_logit(a, r, min(i0 + e * kThreads + tid, last));
  } else {
#pragma unroll
    for (int e = 0; e < kElems; ++e) xs[e] = load_logit(a, r, min(i0 + e * kThreads + tid, last));
  }
  float m = kNegInf;
  uint64_t best = 0;
  float xd = 0.f;
  bool owns = false;
#pragma unroll
  for (int e = 0; e < kElems; ++e) {
    const int i = i0 + e * kThreads + tid;
    float x = greedy ? xs[e] : xs[e] / temp;
    xs[e] = i < i1 ? x : kNegInf;
    if (i < i1) {
      m = fmaxf(m, x);
      const bool is_draft = static_cast<int64_t>(i) == dr;
      if (is_draft) {
        xd = x;
        owns = true;
      }
      uint64_t c;
      score_composite(a, r, i, x, is_draft, greedy, c);
      best = c > best ? c : best;
    }
  }
  if (owns) v.xd[r] = xd;  // one thread of one segment
  float sum = 0.f;
  if (!greedy) {
    const float sub = m == kNegInf ? 0.f : m;
#pragma unroll
    for (int e = 0; e < kElems; ++e) sum += __expf(xs[e] - sub);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t c = shfl_xor_u64(best, o);
    best = c > best ? c : best;
    stat_merge(m, sum, __shfl_xor(m, o, 64), __shfl_xor(sum, o, 64));
  }
  if (lane == 0) {
    s_best[wave] = best;
    s_m[wave] = m;
    s_s[wave] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      best = s_best[w] > best ? s_best[w] : best;
      stat_merge(m, sum, s_m[w], s_s[w]);
    }
    VerifyStat* st = v.stat + static_cast<long>(r) * a.S + s;
    st->best = best;
    st->m = m;
    st->sum = sum;
  }
}

// One wave per request.  Position j (K + 1 <= 16 of them) belongs to the four lanes 4 j .. 4 j + 3: they fold its segments,
// lane 4 j decides it, and two ballots replace the scan: the leading valid drafts give n_b, the leading accepted ones the
// position of the sampled token.
__global__ __launch_bounds__(64) void verify_final_kernel(const VerifyArgs v) {
  constexpr uint64_t kHeads = 0x1111111111111111ull;  // lane 4 j of every position
  const Args& a = v.a;
  const int b = blockIdx.x, lane = threadIdx.x, K = v.K;
  const int j = lane >> 2, sub = lane & 3;
  const float temp = a.t_arr ? a.t_arr[b] : a.t_val;
  const bool greedy = !(temp > 0.f);
  const int r = b * (K + 1) + j;
  int64_t d = -1;
  if (j < K) {
    d = v.draft[static_cast<long>(b) * K + j];
    if (d < 0 || d >= a.V) d = -1;
  }
  // positions K .. 15 count as invalid, so a clear bit exists; rows past n_b were not written by the segment pass
  const int nb = __builtin_ctzll(~__ballot(d >= 0) & kHeads) >> 2;
  const bool live = j <= nb;
  float m = kNegInf, sum = 0.f;
  uint64_t best = 0;
  if (live) {
    for (int s = sub; s < a.S; s += 4) {
      const VerifyStat st = v.stat[static_cast<long>(r) * a.S + s];
      best = st.best > best ? st.best : best;
      stat_merge(m, sum, st.m, st.sum);
    }
  }
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {
    const uint64_t c = shfl_xor_u64(best, o);
    best = c > best ? c : best;
    stat_merge(m, sum, __shfl_xor(m, o, 64), __shfl_xor(sum, o, 64));
  }
  bool accept = false;
  if (live && d >= 0) {
    const float xd = v.xd[r];
    if (greedy) {  // d is the arg-max iff its composite beats the best of the others
      accept = composite_of(ieee_key(xd), static_cast<uint32_t>(d)) > best;
    } else {
      const float p = __expf(xd - m) / sum;
      const float u = v.uniform ? v.uniform[static_cast<long>(b) * K + j] : own_uniform(a, r);
      accept = u < p;
    }
  }
  // only lane 4 j's verdict counts (the lanes of a position add their statistics in different orders); position n_b has
  // no draft and is never accepted, so the first clear bit is at most n_b
  const int jr = __builtin_ctzll(~__ballot(accept) & kHeads) >> 2;
  if (sub == 0 && j <= K) {
    int* out = a.out + static_cast<long>(b) * (K + 1);
    out[j] = j < jr ? static_cast<int>(d) : (j == jr ? static_cast<int>(index_of(best)) : -1);
  }
  if (lane == 0) v.num_accepted[b] = jr;
}

// ---- log-probability, rank and top-N of a given token per row (ours: no reference counterpart) ------------------------
// The third reader of the logits a step ends in, after the sampler and the verification: row r has a token t_r (what one
// of them emitted, or a prompt token), and the answer is y[t] - logsumexp(y) with y = x / T (x when T == 0), the token's
// 1-based rank in the order of the RAW logits, and the first num_top entries of that order with their log-probabilities.
// The order is torch_topk_key's (-0.0 == +0.0, ties to the smaller id) as 52-bit composites, so a rank is a count of
// larger composites and the top list is the sampler's threshold / compaction / select_kth selection.  Phase 1 (grid S x
// rows) is verify_segment_kernel's pass - every load issued first, the same y, the same statistics - plus the count and,
// with num_top > 0, the segment's candidates; phase 2 (one workgroup per row) folds, selects, sorts and writes.  A row
// whose token is outside [0, V) is dead: neither phase reads its logits.
struct LogprobStat {  // one per (row, segment)
  float m, sum;       // max of y, sum exp(y - m)
  int above, pad;     // elements of the segment whose composite is larger than the token's
};
struct LogprobArgs {
  Args a;             // logits, dtype, row_stride, B = rows, V, S, seg, t_arr / t_val
  const void* tok;    // [rows] int32 or int64
  int tok_bytes;
  int rows_per_temp;  // row r uses t_arr[r / rows_per_temp]
  int row0;           // first row of this launch pair (a grid's y extent is 65535)
  int K;              // num_top
  float* lp;          // [rows]
  int* rank;          // [rows]
  int* top_ids;       // [rows][K]
  float* top_lp;      // [rows][K]
  LogprobStat* stat;  // [rows][S]
  uint64_t* cand;     // [rows][S][K] composites
};

// the row's token, -1 when the row is dead
__device__ __forceinline__ int logprob_token(const LogprobArgs& g, int r) {
  const int64_t t = g.tok_bytes == 8 ? static_cast<const int64_t*>(g.tok)[r] : static_cast<const int*>(g.tok)[r];
  return (t < 0 || t >= g.a.V) ? -1 : static_cast<int>(t);
}
__device__ __forceinline__ float logprob_temp(const LogprobArgs& g, int r) {
  return g.a.t_arr ? g.a.t_arr[r / g.rows_per_temp] : g.a.t_val;
}
// The one expression behind token_logprobs and top_logprobs: the element's value decoded from its order key (so -0.0 has
// become +0.0 for both), scaled as phase 1 scaled it, minus the row's maximum first - |y - m| <= |result|, so the
// subtraction costs one rounding of the result and not one of m + log(sum) - then minus log(sum).
__device__ __forceinline__ float logprob_value(uint32_t key, float temp, float m, float log_sum) {
  const float x = ieee_key_value(key);
  const float y = temp > 0.f ? x / temp : x;
  return (y - m) - log_sum;
}

template <bool kTop>
__global__ __launch_bounds__(kThreads) void logprobs_segment_kernel(const LogprobArgs g) {
  __shared__ uint64_t s_list[kTop ? kSegMax : 1];
  __shared__ unsigned s_hist[256];
  __shared__ int s_misc[6];
  __shared__ float s_m[4], s_s[4];
  __shared__ int s_c[4];
  const Args& a = g.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, r = g.row0 + blockIdx.y;
  const int tok = logprob_token(g, r);
  if (tok < 0) return;  // block-uniform
  const float temp = logprob_temp(g, r);
  const bool greedy = !(temp > 0.f);
  const uint64_t ctok = comp_of(torch_topk_key(load_logit(a, r, tok)), static_cast<uint32_t>(tok));
  const int i0 = s * a.seg, i1 = min(a.V, i0 + a.seg);

  // as verify_segment_kernel: all loads first; out-of-range slots read the segment's last element and are set to -inf
  float xs[kElems];
  const int last = i1 - 1;
  if (i0 >= i1) {
#pragma unroll
    for (int e = 0; e < kElems; ++e) xs[e] = 0.f;
  } else if (a.dtype == 0) {
#pragma unroll
    for (int e = 0; e < kElems; ++e) xs[e] = load_logit(a, r, min(i0 + e * kThreads + tid, last));
  } else {
#pragma unroll
    for (int e = 0; e < kElems; ++e) xs[e] = load_logit(a, r, min(i0 + e * kThreads + tid, last));
  }
  uint32_t key[kTop ? kElems : 1];
  uint32_t best = 0;
  float m = kNegInf;
  int above = 0;
#pragma unroll
  for (int e = 0; e < kElems; ++e) {
    const int i = i0 + e * kThreads + tid;
    const bool in = i < i1;
    const uint32_t k = in ? torch_topk_key(xs[e]) : 0u;
    above += in && comp_of(k, static_cast<uint32_t>(i)) > ctok;
    if (kTop) {
      key[e] = k;
      best = max(best, k);
    }
    const float y = greedy ? xs[e] : xs[e] / temp;
    xs[e] = in ? y : kNegInf;
    m = fmaxf(m, xs[e]);
  }
  float sum = 0.f;
  {
    const float sub = m == kNegInf ? 0.f : m;
#pragma unroll
    for (int e = 0; e < kElems; ++e) sum += __expf(xs[e] - sub);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    above += __shfl_xor(above, o, 64);
    stat_merge(m, sum, __shfl_xor(m, o, 64), __shfl_xor(sum, o, 64));
  }
  if (lane == 0) {
    s_m[wave] = m;
    s_s[wave] = sum;
    s_c[wave] = above;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) {
      stat_merge(m, sum, s_m[w], s_s[w]);
      above += s_c[w];
    }
    LogprobStat* st = g.stat + static_cast<long>(r) * a.S + s;
    st->m = m;
    st->sum = sum;
    st->above = above;
  }
  if constexpr (kTop) {
    // the segment's top K composites, as sampler_segment_kernel selects them
    const int K = g.K;
    const int n = max(i1 - i0, 0);
    uint32_t bound = 0;
    if (n > K) {
      s_list[tid] = comp_of(best, tid);
      __syncthreads();
      bound = static_cast<uint32_t>(select_kth(s_list, kThreads, K, s_hist, s_misc) >> kIdxBits);
    }
    if (tid == 0) s_misc[2] = 0;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kElems; ++e) {
      if (key[e] && key[e] >= bound) {
        const int pos = atomicAdd(&s_misc[2], 1);
        s_list[pos] = comp_of(key[e], i0 + e * kThreads + tid);
      }
    }
    __syncthreads();
    const int cnt = s_misc[2];
    uint64_t thr = 0;
    if (cnt > K) thr = select_kth(s_list, cnt, K, s_hist, s_misc);
    if (tid == 0) s_misc[3] = 0;
    __syncthreads();
    uint64_t* out = g.cand + (static_cast<long>(r) * a.S + s) * K;
    for (int i = tid; i < cnt; i += kThreads) {
      const uint64_t c = s_list[i];
      if (c >= thr) out[atomicAdd(&s_misc[3], 1)] = c;
    }
    __syncthreads();
    // fewer than K elements: pad with distinct composites below every real one (key part 0)
    for (int i = min(cnt, K) + tid; i < K; i += kThreads) out[i] = static_cast<uint64_t>(s * K + i);
  }
}

// kTop: 256 threads select the K winners out of S * K, then wave 0 sorts them; otherwise one wave.
template <bool kTop>
__global__ __launch_bounds__(kTop ? kThreads : 64) void logprobs_final_kernel(const LogprobArgs g) {
  constexpr int kListMax = (1 << kIdxBits) / kSegMax * 32;  // S <= 128 segments of K <= 32 candidates
  __shared__ uint64_t s_list[kTop ? kListMax : 1];
  __shared__ uint64_t s_sel[64];
  __shared__ unsigned s_hist[256];
  __shared__ int s_misc[6];
  const Args& a = g.a;
  const int tid = threadIdx.x, lane = tid & 63;
  const int r = g.row0 + blockIdx.x;
  const int K = g.K;
  const int tok = logprob_token(g, r);
  if (tok < 0) {  // block-uniform
    if (tid == 0) {
      g.lp[r] = 0.f;
      g.rank[r] = 0;
    }
    for (int i = tid; i < K; i += blockDim.x) {
      g.top_ids[static_cast<long>(r) * K + i] = -1;
      g.top_lp[static_cast<long>(r) * K + i] = 0.f;
    }
    return;
  }
  uint64_t c = 0;
  if (kTop) {
    const int n = a.S * K;  // > K: S >= 16
    const uint64_t* cand = g.cand + static_cast<long>(r) * n;
    for (int i = tid; i < n; i += kThreads) s_list[i] = cand[i];
    if (tid < 64) s_sel[tid] = 0;
    if (tid == 0) s_misc[2] = 0;
    __syncthreads();
    const uint64_t thr = select_kth(s_list, n, K, s_hist, s_misc);
    for (int i = tid; i < n; i += kThreads) {
      const uint64_t v = s_list[i];
      if (v >= thr) s_sel[atomicAdd(&s_misc[2], 1)] = v;
    }
    __syncthreads();
    if (tid >= 64) return;
    // bitonic sort (descending) of one composite per lane, as sampler_final_kernel's
    c = s_sel[lane];
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
      for (int j = k >> 1; j > 0; j >>= 1) {
        const uint64_t o = shfl_xor_u64(c, j);
        const bool up = (lane & k) != 0;
        const bool lower = (lane & j) == 0;
        const bool take_max = (lower != up);
        c = take_max ? (c > o ? c : o) : (c < o ? c : o);
      }
  }
  float m = kNegInf, sum = 0.f;
  int above = 0;
  for (int s = lane; s < a.S; s += 64) {
    const LogprobStat st = g.stat[static_cast<long>(r) * a.S + s];
    stat_merge(m, sum, st.m, st.sum);
    above += st.above;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    above += __shfl_xor(above, o, 64);
    stat_merge(m, sum, __shfl_xor(m, o, 64), __shfl_xor(sum, o, 64));
  }
  // lane 0's fold for every lane: the token's value and its slot of the top list must see the same bits
  m = __shfl(m, 0, 64);
  const float log_sum = logf(__shfl(sum, 0, 64));
  const float temp = logprob_temp(g, r);
  if (lane == 0) {
    g.lp[r] = logprob_value(torch_topk_key(load_logit(a, r, tok)), temp, m, log_sum);
    g.rank[r] = above + 1;
  }
  if (kTop && lane < K) {
    const uint32_t key = static_cast<uint32_t>(c >> kIdxBits);
    const bool real = key != 0;  // num_top <= V: always
    g.top_ids[static_cast<long>(r) * K + lane] = real ? static_cast<int>(kIdxMask - (c & kIdxMask)) : -1;
    g.top_lp[static_cast<long>(r) * K + lane] = real ? logprob_value(key, temp, m, log_sum) : 0.f;
  }
}

// launch counter: the same seed gives fresh noise on every launch (reference sampler_rng.cuh:41-52)
std::atomic<uint64_t> g_launch_offset{0};
inline uint64_t next_offset() { return g_launch_offset.fetch_add(128, std::memory_order_relaxed); }

inline int segments_of(int V) {
  const int s = (V + kSegMax - 1) / kSegMax;
  return s < 16 ? 16 : s;
}

// The refusals the fast path and verification share, wrong arguments (INVALID) before the sizes the kernels do not cover (UNSUPPORTED:
// a vocabulary that is no multiple of 8 or has token ids of 2^20 and up, more logits rows than a grid's y extent).
inline int check_common(bool pointers, int dtype, int64_t rows, int V) {
  if (!pointers) return HPC_ERR_INVALID;
  if (rows < 0 || V <= 0 || (dtype != 0 && dtype != 1)) return HPC_ERR_INVALID;
  if ((V & 7) || V >= (1 << kIdxBits)) return HPC_ERR_UNSUPPORTED;
  if (rows > 65535) return HPC_ERR_UNSUPPORTED;
  return HPC_OK;
}

// The part of Args every entry fills.  A segment is ceil(V / S) elements rounded up to seg_round: kThreads for the top-k
// path (its threads stride the segment), 1 for the fast path and verification (<= kSegMax, the kElems registers of a thread).
inline void fill_common(Args& a, const void* logits, int dtype, int64_t row_stride, int rows, int V, int seg_round,
                        const void* temp_arr, float temp_val, const void* gumbel_noise, uint64_t seed, void* out) {
  a.logits = logits;
  a.dtype = dtype;
  a.row_stride = row_stride;
  a.B = rows;
  a.V = V;
  a.S = segments_of(V);
  a.seg = ((V + a.S - 1) / a.S + seg_round - 1) / seg_round * seg_round;
  a.t_arr = static_cast<const float*>(temp_arr);
  a.t_val = temp_val;
  a.noise = static_cast<const float*>(gumbel_noise);
  a.seed = seed;
  a.offset = gumbel_noise ? 0 : next_offset();
  a.out = static_cast<int*>(out);
}

}  // namespace sampler
}  // namespace hpc

extern "C" int hpc_sampler_segments(int vocab_size) { return hpc::sampler::segments_of(vocab_size); }

// workspace: candidates [B][S][max_topk] u64 + segment softmax statistics [B][S][2] f32
extern "C" int64_t hpc_fused_sampler_workspace_bytes(int batch_size, int vocab_size, int max_topk) {
  const int64_t S = hpc::sampler::segments_of(vocab_size);
  return static_cast<int64_t>(batch_size) * S * max_topk * 8 + static_cast<int64_t>(batch_size) * S * 8;
}

// reference: fused_sampler_async (src/sampler/sampler.h:17-31, src/sampler/fused_sampler.cu:700-775)
extern "C" int hpc_fused_sampler_async(
    void* token_ids, void* workspace, const void* logits, int logits_dtype, void* penalty_mask,
    int64_t penalty_mask_row_bytes, const void* slot_id, const void* rp_arr, float rp_val, const void* temp_arr,
    float temp_val, int softmax_policy, const void* topk_ptr, int topk_int_bytes, int topk_val,
    const void* topp_arr, float topp_val, const void* gumbel_noise, int batch_size, int vocab_size,
    int64_t logits_row_stride, int max_topk, uint64_t rng_seed, hipStream_t stream) {
  using namespace hpc::sampler;
  // check_common's checks in this entry's own order (the dtype after the vocabulary, the batch limit last): an input that
  // is wrong in two ways keeps the code it has always got
  if (!token_ids || !workspace || !logits) return HPC_ERR_INVALID;
  if (batch_size < 0 || vocab_size <= 0 || (max_topk != 32 && max_topk != 64)) return HPC_ERR_INVALID;
  if (batch_size == 0) return HPC_OK;
  if ((vocab_size & 7) || vocab_size >= (1 << kIdxBits)) return HPC_ERR_UNSUPPORTED;
  if ((penalty_mask == nullptr) != (slot_id == nullptr)) return HPC_ERR_INVALID;
  if (softmax_policy < 0 || softmax_policy > 2 || (logits_dtype != 0 && logits_dtype != 1)) return HPC_ERR_INVALID;
  if (batch_size > 65535) return HPC_ERR_UNSUPPORTED;
  Args a{};
  fill_common(a, logits, logits_dtype, logits_row_stride, batch_size, vocab_size, kThreads, temp_arr, temp_val, gumbel_noise,
              rng_seed, token_ids);
  a.mask = static_cast<uint8_t*>(penalty_mask);
  a.mask_stride = penalty_mask_row_bytes;
  a.slot = static_cast<const int*>(slot_id);
  a.rp_arr = static_cast<const float*>(rp_arr);
  a.rp_val = rp_val;
  a.policy = softmax_policy;
  a.topk_ptr = topk_ptr;
  a.topk_bytes = topk_int_bytes;
  a.topk_val = topk_val;
  a.topp_arr = static_cast<const float*>(topp_arr);
  a.topp_val = topp_val;
  a.max_topk = max_topk;
  a.cand = static_cast<uint64_t*>(workspace);
  a.seg_stat = reinterpret_cast<float*>(a.cand + static_cast<int64_t>(batch_size) * a.S * max_topk);
  sampler_segment_kernel<<<dim3(a.S, batch_size), kThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  sampler_final_kernel<<<batch_size, kThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

// reference: fused_sampler_temperature_async (src/sampler/sampler.h:33-45,
// src/sampler/fused_sampler_temperature.cu:480-574).  workspace: batch_size * segments u64.
extern "C" int hpc_fused_sampler_temperature_async(void* token_ids, void* workspace, const void* logits,
                                                   int logits_dtype, int64_t logits_row_stride,
                                                   const void* temp_arr, float temp_val,
                                                   const void* gumbel_noise, const void* draft_token_ids,
                                                   int batch_size, int vocab_size, uint64_t rng_seed,
                                                   hipStream_t stream) {
  using namespace hpc::sampler;
  const int rc = check_common(token_ids && workspace && logits, logits_dtype, batch_size, vocab_size);
  if (rc == HPC_ERR_INVALID) return rc;
  if (batch_size == 0) return HPC_OK;  // an empty batch is accepted ahead of the size limits
  if (rc != HPC_OK) return rc;
  Args a{};
  fill_common(a, logits, logits_dtype, logits_row_stride, batch_size, vocab_size, 1, temp_arr, temp_val, gumbel_noise, rng_seed,
              token_ids);
  a.draft = static_cast<const int64_t*>(draft_token_ids);
  a.cand = static_cast<uint64_t*>(workspace);
  temperature_segment_kernel<<<dim3(a.S, batch_size), kThreads, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  temperature_final_kernel<<<batch_size, 64, 0, stream>>>(a);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

// workspace: segment statistics [rows][S] of 16 bytes + the scaled logit at each row's draft [rows] f32
extern "C" int64_t hpc_speculative_verify_workspace_bytes(int batch_size, int num_draft, int vocab_size) {
  if (batch_size < 0 || num_draft < 0 || vocab_size <= 0) return 0;
  const int64_t rows = static_cast<int64_t>(batch_size) * (num_draft + 1);
  return rows * hpc::sampler::segments_of(vocab_size) * static_cast<int64_t>(sizeof(hpc::sampler::VerifyStat)) + rows * 4;
}

// semantics: include/hpc_amd.h.  Every check runs before the batch_size == 0 return, so none can reach a launch.
extern "C" int hpc_speculative_verify_async(void* output_token_ids, void* num_accepted, void* workspace, const void* logits,
                                            int logits_dtype, int64_t logits_row_stride, const void* draft_token_ids,
                                            const void* temperature, float temperature_val, const void* uniform_samples,
                                            const void* gumbel_noise, int batch_size, int num_draft, int vocab_size,
                                            uint64_t rng_seed, hipStream_t stream) {
  using namespace hpc::sampler;
  if (batch_size < 0 || num_draft < 0) return HPC_ERR_INVALID;
  const int64_t rows = static_cast<int64_t>(batch_size) * (num_draft + 1);
  const int rc = check_common(output_token_ids && num_accepted && workspace && logits, logits_dtype, rows, vocab_size);
  if (rc == HPC_ERR_INVALID) return rc;
  if (num_draft > 0 && !draft_token_ids) return HPC_ERR_INVALID;
  if (logits_row_stride < vocab_size) return HPC_ERR_INVALID;
  // no draft, no uniform: with num_draft == 0 uniform_samples is [batch_size, 0] and is not looked at
  if (num_draft > 0 && (uniform_samples == nullptr) != (gumbel_noise == nullptr)) return HPC_ERR_INVALID;
  if (!gumbel_noise && rng_seed == 0) return HPC_ERR_INVALID;
  if (num_draft > 15 || rc != HPC_OK) return HPC_ERR_UNSUPPORTED;
  if (batch_size == 0) return HPC_OK;
  VerifyArgs v{};
  Args& a = v.a;
  fill_common(a, logits, logits_dtype, logits_row_stride, static_cast<int>(rows), vocab_size, 1, temperature, temperature_val,
              gumbel_noise, rng_seed, output_token_ids);
  v.draft = static_cast<const int64_t*>(draft_token_ids);
  v.uniform = static_cast<const float*>(uniform_samples);
  v.K = num_draft;
  v.num_accepted = static_cast<int*>(num_accepted);
  v.stat = static_cast<VerifyStat*>(workspace);
  v.xd = reinterpret_cast<float*>(v.stat + rows * a.S);
  verify_segment_kernel<<<dim3(a.S, static_cast<unsigned>(rows)), kThreads, 0, stream>>>(v);
  HPC_CHECK_LAUNCH();
  verify_final_kernel<<<batch_size, 64, 0, stream>>>(v);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

// workspace: segment statistics [rows][S] of 16 bytes + candidates [rows][S][num_top] u64
extern "C" int64_t hpc_token_logprobs_workspace_bytes(int rows, int num_top, int vocab_size) {
  if (rows < 0 || num_top < 0 || vocab_size <= 0) return 0;
  const int64_t slots = static_cast<int64_t>(rows) * hpc::sampler::segments_of(vocab_size);
  return slots * static_cast<int64_t>(sizeof(hpc::sampler::LogprobStat)) + slots * num_top * 8;
}

// semantics: include/hpc_amd.h.  Every check runs before the rows == 0 return, so none can reach a launch.
extern "C" int hpc_token_logprobs_async(void* token_logprobs, void* token_ranks, void* top_ids, void* top_logprobs, void* workspace,
                                        const void* logits, int logits_dtype, int64_t logits_row_stride, const void* token_ids,
                                        int token_id_bytes, const void* temperature, int temperature_count, float temperature_val,
                                        int rows, int num_top, int vocab_size, hipStream_t stream) {
  using namespace hpc::sampler;
  if (!token_logprobs || !token_ranks || !workspace || !logits || !token_ids) return HPC_ERR_INVALID;
  if (rows < 0 || num_top < 0 || vocab_size <= 0) return HPC_ERR_INVALID;
  if (num_top > 0 && (!top_ids || !top_logprobs)) return HPC_ERR_INVALID;
  if (logits_dtype != 0 && logits_dtype != 1) return HPC_ERR_INVALID;
  if (logits_row_stride < vocab_size) return HPC_ERR_INVALID;
  if (token_id_bytes != 4 && token_id_bytes != 8) return HPC_ERR_INVALID;
  if (temperature ? (temperature_count < 1 || rows % temperature_count != 0) : !(temperature_val >= 0.f)) return HPC_ERR_INVALID;
  if ((vocab_size & 7) || vocab_size >= (1 << kIdxBits)) return HPC_ERR_UNSUPPORTED;
  if (num_top > 32 || num_top > vocab_size) return HPC_ERR_UNSUPPORTED;
  if (rows == 0) return HPC_OK;
  LogprobArgs g{};
  Args& a = g.a;  // fill_common's fields without its noise offset: this op draws nothing
  a.logits = logits;
  a.dtype = logits_dtype;
  a.row_stride = logits_row_stride;
  a.B = rows;
  a.V = vocab_size;
  a.S = segments_of(vocab_size);
  a.seg = (vocab_size + a.S - 1) / a.S;
  a.t_arr = static_cast<const float*>(temperature);
  a.t_val = temperature_val;
  g.tok = token_ids;
  g.tok_bytes = token_id_bytes;
  g.rows_per_temp = temperature ? rows / temperature_count : 1;
  g.K = num_top;
  g.lp = static_cast<float*>(token_logprobs);
  g.rank = static_cast<int*>(token_ranks);
  g.top_ids = static_cast<int*>(top_ids);
  g.top_lp = static_cast<float*>(top_logprobs);
  g.stat = static_cast<LogprobStat*>(workspace);
  g.cand = reinterpret_cast<uint64_t*>(g.stat + static_cast<int64_t>(rows) * a.S);
  // rows sit on the grid's y axis: one launch pair per 65535 rows
  for (int row0 = 0; row0 < rows; row0 += 65535) {
    const int n = rows - row0 < 65535 ? rows - row0 : 65535;
    g.row0 = row0;
    if (num_top > 0) {
      logprobs_segment_kernel<true><<<dim3(a.S, n), kThreads, 0, stream>>>(g);
      HPC_CHECK_LAUNCH();
      logprobs_final_kernel<true><<<n, kThreads, 0, stream>>>(g);
    } else {
      logprobs_segment_kernel<false><<<dim3(a.S, n), kThreads, 0, stream>>>(g);
      HPC_CHECK_LAUNCH();
      logprobs_final_kernel<false><<<n, 64, 0, stream>>>(g);
    }
    HPC_CHECK_LAUNCH();
  }
  return HPC_OK;
}
