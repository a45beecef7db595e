// Fused softmax + top-k router for gfx950: the step between the router GEMM (gemm_bf16xfp32.hip) and
// fuse_moe* - it produces the `topk_ids` / `topk_scale` tensors those ops consume.
//
// The reference has no such kernel (hpc/gemm.py:16-61 stops at the GEMM and callers use torch.topk +
// softmax in eager mode); BASELINE north_star asks for one on wavefront shuffles.  Semantics are pinned
// to the stable PyTorch formulation (oracle/router.py):
//     order   = stable descending sort of the logits  (ties -> smaller expert id first; NaN sorts
//               above +inf like torch.topk)
//     ids     = order[:, :k]                                   (int32, best first)
//     p       = softmax(logits, dim=-1) in fp32
//     weights = p[ids]                  (renormalize = 0)      or p[ids] / sum_j p[ids_j]  (renormalize = 1)
// Selecting on the logits instead of on p is the same choice mathematically (softmax is monotonic)
// and makes the indices independent of the exp implementation: the bar is torch.equal on ids.
//
// MI355X design: one wave per token row, the row held in registers (16 B per lane and 256 experts),
// no LDS.  A round of selection = every lane's best remaining element as a 64-bit composite
// (order-preserving key << 32 | ~expert id) followed by a wave-wide max through 6 shuffle steps; the
// winner is struck out in its owner lane.  k rounds give the top-k in rank order; the row maximum is
// round 0's winner, the softmax denominator one more shuffle reduction.
//
// The second kernel here, grouped_topk_router_kernel, is the group-limited router of DeepSeek-V3 / R1, Kimi-K2 and
// DeepSeek-V2 (tests/grouped_router_ref.py states it in PyTorch): scores s = sigmoid or softmax of the logits, choice
// scores c = s + correction bias, the experts in contiguous groups of which the `topk_group` best stay (group score =
// sum of the group's two best c with a bias, its best c without), top-k on c among the experts that stay, weights
// from the UNBIASED s, renormalised and scaled.  Same row-in-registers layout and the same composite-key rounds over
// the experts; the groups are ranked by their composites (key of the score << 32 | ~group id) without rounds.
#include "ordered_key.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace router {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / 64;
constexpr int kMaxTopk = 64;

// Keys are torch_topk_key, composites and wave_max_u64 as in ordered_key.h.  The row load and the selection rounds are
// written in both kernels below: as shared functions they compile to other listings (a branch the other way round in
// the grouped kernel, other registers in this one), and the softmax kernel decodes its row maximum inside round 0.
// kVec: float4 vectors per lane (experts <= 256 * kVec); element c of vector j of lane l is expert
// 256 j + 4 l + c, so a wave reads whole 1 KB row segments.
template <int kVec>
__global__ __launch_bounds__(kThreads) void topk_router_kernel(const float* __restrict__ logits,
                                                               int* __restrict__ ids,
                                                               float* __restrict__ weights, int num_tokens,
                                                               int num_expert, long ld, int topk,
                                                               int renormalize) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= num_tokens) return;
  const float* src = logits + static_cast<long>(row) * ld;
  float x[kVec][4];
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
    const int e0 = 256 * j + 4 * lane;
    if (e0 < num_expert) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + e0);
#pragma unroll
      for (int c = 0; c < 4; ++c) x[j][c] = v[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) x[j][c] = -__builtin_inff();
    }
  }
  // composites of this lane's elements; 0 = struck out / not an expert
  uint64_t comp[kVec][4];
#pragma unroll
  for (int j = 0; j < kVec; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int e = 256 * j + 4 * lane + c;
      comp[j][c] = e < num_expert ? composite_of(torch_topk_key(x[j][c]), e) : 0ull;
    }

  uint64_t mine = 0;  // lane r keeps the winner of round r (two rounds per lane when topk > 64: not supported)
  float row_max = 0.f;
  for (int r = 0; r < topk; ++r) {
    uint64_t best = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) best = comp[j][c] > best ? comp[j][c] : best;
    const uint64_t win = wave_max_u64(best);
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) comp[j][c] = comp[j][c] == win ? 0ull : comp[j][c];  // composites are unique
    if (lane == r) mine = win;
    if (r == 0) {  // ieee_key_value, spelled out here and below: as a call it moves an instruction in the listing
      const uint32_t k32 = static_cast<uint32_t>(win >> 32);
      const uint32_t bits = (k32 & 0x80000000u) ? (k32 & 0x7fffffffu) : ~k32;
      row_max = __uint_as_float(bits);
    }
  }
  // softmax statistics over the whole row (max = the first winner; -inf rows / NaN follow IEEE like torch)
  float denom = 0.f;
#pragma unroll
  for (int j = 0; j < kVec; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int e = 256 * j + 4 * lane + c;
      if (e < num_expert) denom += expf(x[j][c] - row_max);
    }
  denom = wave_sum(denom);
  float p = 0.f;
  int id = 0;
  if (lane < topk) {
    id = static_cast<int>(index_of(mine));
    const uint32_t k32 = static_cast<uint32_t>(mine >> 32);
    const uint32_t bits = (k32 & 0x80000000u) ? (k32 & 0x7fffffffu) : ~k32;
    p = expf(__uint_as_float(bits) - row_max);
  }
  const float sel = wave_sum(p);
  if (lane < topk) {
    ids[static_cast<long>(row) * topk + lane] = id;
    weights[static_cast<long>(row) * topk + lane] = p / (renormalize ? sel : denom);
  }
}

// ---- group-limited router -------------------------------------------------------------------------------------------
// the two largest of {a1 >= a2} U {b1 >= b2}
__device__ __forceinline__ void top2_merge(float& a1, float& a2, float b1, float b2) {
  const float lo = fminf(a1, b1);
  a1 = fmaxf(a1, b1);
  a2 = fmaxf(lo, fmaxf(a2, b2));
}

// kVec and the element layout as above.  group_lanes: lanes per group when a group is an aligned power-of-two run of
// lanes of one j (group_size = 4 * group_lanes <= 256: every group's score then comes out of the same log2(group_lanes)
// xor-shuffle steps), 0 otherwise (a loop over the groups, each reduced across the whole wave).  select_groups = 0:
// every group stays (one group, or topk_group == num_expert_group) and the group stage is skipped.
template <int kVec>
__global__ __launch_bounds__(kThreads) void grouped_topk_router_kernel(
    const float* __restrict__ logits, const float* __restrict__ bias, int* __restrict__ ids,
    float* __restrict__ weights, int num_tokens, int num_expert, long ld, int topk, int num_group, int topk_group,
    int group_size, int group_lanes, int select_groups, int sigmoid, int renormalize, float scale) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (row >= num_tokens) return;
  const float* src = logits + static_cast<long>(row) * ld;
  const float ninf = -__builtin_inff();
  float s[kVec][4];  // logits, then scores
  float b[kVec][4];
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
    const int e0 = 256 * j + 4 * lane;
#pragma unroll
    for (int c = 0; c < 4; ++c) s[j][c] = ninf, b[j][c] = 0.f;
    if (e0 < num_expert) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + e0);
#pragma unroll
      for (int c = 0; c < 4; ++c) s[j][c] = v[c];
      if (bias) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(bias + e0);
#pragma unroll
        for (int c = 0; c < 4; ++c) b[j][c] = w[c];
      }
    }
  }
  if (sigmoid) {
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) s[j][c] = 1.f / (1.f + expf(-s[j][c]));  // -inf -> 0, +inf -> 1; 0 past num_expert
  } else {
    float row_max = ninf;
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) row_max = fmaxf(row_max, s[j][c]);
    row_max = wave_max(row_max);
    float denom = 0.f;
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s[j][c] = expf(s[j][c] - row_max);  // 0 past num_expert
        denom += s[j][c];
      }
    denom = wave_sum(denom);
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) s[j][c] = s[j][c] / denom;
  }
  // choice scores and their composites; 0 = struck out / not an expert
  float ch[kVec][4];
  uint64_t comp[kVec][4];
#pragma unroll
  for (int j = 0; j < kVec; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int e = 256 * j + 4 * lane + c;
      ch[j][c] = e < num_expert ? s[j][c] + b[j][c] : ninf;
      comp[j][c] = e < num_expert ? composite_of(torch_topk_key(ch[j][c]), e) : 0ull;
    }

  if (select_groups) {
    // this lane's two best of each vector (a float4 never straddles a group) and the group the vector belongs to
    float m1[kVec], m2[kVec];
    int gid[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      m1[j] = fmaxf(ch[j][0], ch[j][1]);
      m2[j] = fminf(ch[j][0], ch[j][1]);
      top2_merge(m1[j], m2[j], fmaxf(ch[j][2], ch[j][3]), fminf(ch[j][2], ch[j][3]));
      const int e0 = 256 * j + 4 * lane;
      gid[j] = e0 < num_expert ? e0 / group_size : -1;
    }
    if (group_lanes) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1)
        if (o < group_lanes) {
#pragma unroll
          for (int j = 0; j < kVec; ++j) top2_merge(m1[j], m2[j], __shfl_xor(m1[j], o, 64), __shfl_xor(m2[j], o, 64));
        }
    } else {
      for (int g = 0; g < num_group; ++g) {
        float g1 = ninf, g2 = ninf;
#pragma unroll
        for (int j = 0; j < kVec; ++j)
          if (gid[j] == g) top2_merge(g1, g2, m1[j], m2[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) top2_merge(g1, g2, __shfl_xor(g1, o, 64), __shfl_xor(g2, o, 64));
#pragma unroll
        for (int j = 0; j < kVec; ++j)
          if (gid[j] == g) m1[j] = g1, m2[j] = g2;
      }
    }
    // group composites (every lane of a group holds the same one): key of the score high, inverted group id low
    uint64_t gcomp[kVec];
    int beaten[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const float score = bias ? m1[j] + m2[j] : m1[j];
      gcomp[j] = gid[j] >= 0 ? composite_of(torch_topk_key(score), gid[j]) : 0ull;
      beaten[j] = 0;
    }
    // a group stays when fewer than topk_group groups beat it (the composites of two groups differ).  Group g's
    // composite is read from the first lane that holds it; the reads do not wait for one another, unlike selection
    // rounds, each of which needs the one before.
    for (int g = 0; g < num_group; ++g) {
      const int e0 = g * group_size;
      uint64_t v = gcomp[0];
#pragma unroll
      for (int j = 1; j < kVec; ++j) v = (e0 >> 8) == j ? gcomp[j] : v;
      const int from = (e0 & 255) >> 2;
      const uint32_t lo = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(v)), from);
      const uint32_t hi = __builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(v >> 32)), from);
      const uint64_t other = (static_cast<uint64_t>(hi) << 32) | lo;
#pragma unroll
      for (int j = 0; j < kVec; ++j) beaten[j] += other > gcomp[j] ? 1 : 0;
    }
    bool keep[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) keep[j] = gid[j] >= 0 && beaten[j] < topk_group;
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) comp[j][c] = keep[j] ? comp[j][c] : 0ull;
  }

  uint64_t mine = 0;  // lane r keeps the winner of round r
  for (int r = 0; r < topk; ++r) {
    uint64_t best = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) best = comp[j][c] > best ? comp[j][c] : best;
    const uint64_t win = wave_max_u64(best);
#pragma unroll
    for (int j = 0; j < kVec; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) comp[j][c] = comp[j][c] == win ? 0ull : comp[j][c];  // composites are unique
    if (lane == r) mine = win;
  }
  // the winner's UNBIASED score, from the lane that holds it (a lane past topk asks lane 63 and drops the answer)
  const uint32_t e = 0xffffffffu - static_cast<uint32_t>(mine);  // index_of, spelled out: as a call the compares below compile differently
  const int owner = (e >> 2) & 63;
  float w = 0.f;
#pragma unroll
  for (int j = 0; j < kVec; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = __shfl(s[j][c], owner, 64);
      if (lane < topk && static_cast<int>(e >> 8) == j && static_cast<int>(e & 3) == c) w = v;
    }
  if (renormalize) w = w / (wave_sum(w) + 1e-20f);
  if (lane < topk) {
    ids[static_cast<long>(row) * topk + lane] = static_cast<int>(e);
    weights[static_cast<long>(row) * topk + lane] = w * scale;
  }
}

// The refusals the two C entries share, wrong arguments (INVALID) before the limits of the row-in-registers layout
// (UNSUPPORTED: 16-byte row segments, one winner per lane).
inline int check_router(const void* topk_ids, const void* topk_scale, const float* logits, int num_tokens, int num_expert,
                        int64_t ld_logits, int topk) {
  if (!topk_ids || !topk_scale || !logits) return HPC_ERR_INVALID;
  if (num_tokens < 0 || num_expert <= 0 || topk <= 0 || topk > num_expert) return HPC_ERR_INVALID;
  if (topk > kMaxTopk || num_expert > 1024 || (num_expert & 3) || (ld_logits & 3) || ld_logits < num_expert)
    return HPC_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(logits) & 15) != 0) return HPC_ERR_UNSUPPORTED;
  return HPC_OK;
}

// LAUNCH(kVec) with the float4 vectors per lane that num_expert needs; `grid` is one wave per token row
#define HPC_ROUTER_LADDER(num_tokens, num_expert, LAUNCH)                  \
  do {                                                                     \
    const int grid = ((num_tokens) + kWavesPerBlock - 1) / kWavesPerBlock; \
    const int vec = ((num_expert) + 255) / 256;                            \
    if (vec == 1) {                                                        \
      LAUNCH(1);                                                           \
    } else if (vec == 2) {                                                 \
      LAUNCH(2);                                                           \
    } else {                                                               \
      LAUNCH(4);                                                           \
    }                                                                      \
  } while (0)

}  // namespace router
}  // namespace hpc

extern "C" int hpc_topk_router_async(int* topk_ids, float* topk_scale, const float* logits, int num_tokens,
                                     int num_expert, int64_t ld_logits, int topk, int renormalize,
                                     hipStream_t stream) {
  using namespace hpc::router;
  const int rc = check_router(topk_ids, topk_scale, logits, num_tokens, num_expert, ld_logits, topk);
  if (rc != HPC_OK || num_tokens == 0) return rc;
#define HPC_ROUTER_LAUNCH(V)                                                                              \
  topk_router_kernel<V><<<grid, kThreads, 0, stream>>>(logits, topk_ids, topk_scale, num_tokens, num_expert, \
                                                       ld_logits, topk, renormalize)
  HPC_ROUTER_LADDER(num_tokens, num_expert, HPC_ROUTER_LAUNCH);
#undef HPC_ROUTER_LAUNCH
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}

extern "C" int hpc_grouped_topk_router_async(int* topk_ids, float* topk_scale, const float* logits,
                                             const float* correction_bias, int num_tokens, int num_expert,
                                             int64_t ld_logits, int topk, int num_expert_group, int topk_group,
                                             int scoring_func, int renormalize, float routed_scaling_factor,
                                             hipStream_t stream) {
  using namespace hpc::router;
  // this entry's own wrong arguments go before the layout limits of either
  const int rc = check_router(topk_ids, topk_scale, logits, num_tokens, num_expert, ld_logits, topk);
  if (rc == HPC_ERR_INVALID) return rc;
  if (num_expert_group < 1 || topk_group < 1 || topk_group > num_expert_group || (scoring_func != 0 && scoring_func != 1))
    return HPC_ERR_INVALID;
  if (num_expert % num_expert_group != 0) return HPC_ERR_INVALID;
  const int group_size = num_expert / num_expert_group;
  if (rc != HPC_OK || (group_size & 3)) return HPC_ERR_UNSUPPORTED;
  if (topk > static_cast<int64_t>(topk_group) * group_size) return HPC_ERR_UNSUPPORTED;  // not enough candidates
  if ((reinterpret_cast<uintptr_t>(correction_bias) & 15) != 0) return HPC_ERR_UNSUPPORTED;
  if (num_tokens == 0) return HPC_OK;
  // a group that is an aligned power-of-two run of lanes of one vector: 4, 8, ... 256 experts
  const int lanes = group_size / 4;
  const int group_lanes = (group_size <= 256 && (lanes & (lanes - 1)) == 0) ? lanes : 0;
  const int select_groups = topk_group < num_expert_group;
#define HPC_ROUTER_LAUNCH(V)                                                                                         \
  grouped_topk_router_kernel<V><<<grid, kThreads, 0, stream>>>(                                                      \
      logits, correction_bias, topk_ids, topk_scale, num_tokens, num_expert, ld_logits, topk, num_expert_group,     \
      topk_group, group_size, group_lanes, select_groups, scoring_func, renormalize, routed_scaling_factor)
  HPC_ROUTER_LADDER(num_tokens, num_expert, HPC_ROUTER_LAUNCH);
#undef HPC_ROUTER_LAUNCH
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
