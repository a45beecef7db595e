// merge_attn_states: two attention results over disjoint key sets, each with its log-sum-exp, merged into the result over the
// union (chunked prefill / prefix caching: a chunk's causal self pass and its non-causal pass over the cached context) - gfx950.
// No reference kernel; the statement is tests/mla_prefill_ref.py::merge_statement.
//
// A small streaming kernel: one group of D / 8 lanes per (row, head), each lane one 16-byte load of a and of b and one 16-byte
// store; fp32 arithmetic with one rounding to bf16:
//   m = max(la, lb)   wa = exp(la - m)   wb = exp(lb - m)   out = (wa a + wb b) / (wa + wb)   lse = m + log(wa + wb)
// A side whose lse is -inf passes the other side through bit for bit; both -inf give zeros and -inf.  out may be out_a and lse
// may be lse_a (in place): every lane has read what it needs before the workgroup's barrier and stores behind it.
// Host side: the grid and the shape refusals are attention_prefill_mla_route.h::merge_route(); the overlap rule is checked here.
#include "attention_prefill_mla_route.h"
#include "byte_span.h"
#include "hpc_common.h"
#include "../../include/hpc_amd.h"

namespace hpc {
namespace merge_states {

struct Args {
  uint16_t* out;
  float* lse;
  const uint16_t* out_a;
  const float* lse_a;
  const uint16_t* out_b;
  const float* lse_b;
  long total;  // num_rows * num_head
  int num_head, lanes_per_row, rows_per_wg;
  long o_row, o_head, a_row, a_head, b_row, b_head;  // strides, elements
};

__global__ __launch_bounds__(kMergeThreads) void merge_attn_states_kernel(const Args p) {
  const int tid = threadIdx.x;
  const int grp = tid / p.lanes_per_row, li = tid - grp * p.lanes_per_row;
  const long rid = static_cast<long>(blockIdx.x) * p.rows_per_wg + grp;
  const bool live = grp < p.rows_per_wg && rid < p.total;
  u32x4 xa = u32x4{0u, 0u, 0u, 0u}, xb = xa;
  float la = 0.f, lb = 0.f;
  long t = 0;
  int h = 0;
  if (live) {
    t = rid / p.num_head;
    h = static_cast<int>(rid - t * p.num_head);
    la = p.lse_a[rid];
    lb = p.lse_b[rid];
    xa = ld16(p.out_a + t * p.a_row + h * p.a_head + li * 8);
    xb = ld16(p.out_b + t * p.b_row + h * p.b_head + li * 8);
  }
  __syncthreads();  // in place: a lane group may straddle two waves, and its first lane overwrites the lse the others read
  if (!live) return;
  constexpr float kNegInf = -__builtin_inff();
  const float m = fmaxf(la, lb);
  u32x4 y;
  float l;
  if (la == kNegInf || lb == kNegInf) {  // a side that saw no key: the other one as it is (zeros and -inf when both)
    y = la == kNegInf ? xb : xa;
    if (m == kNegInf) y = u32x4{0u, 0u, 0u, 0u};
    l = m;
  } else {
    const float wa = expf(la - m), wb = expf(lb - m);
    const float inv = 1.0f / (wa + wb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float lo = (wa * bf16lo_to_f32(xa[i]) + wb * bf16lo_to_f32(xb[i])) * inv;
      const float hi = (wa * bf16hi_to_f32(xa[i]) + wb * bf16hi_to_f32(xb[i])) * inv;
      y[i] = pack_bf16x2(lo, hi);
    }
    l = m + logf(wa + wb);
  }
  st16(p.out + t * p.o_row + h * p.o_head + li * 8, y);
  if (li == 0) p.lse[rid] = l;
}

}  // namespace merge_states
}  // namespace hpc

using namespace hpc;

// no reference kernel; the statement is tests/mla_prefill_ref.py
extern "C" int hpc_merge_attn_states_async(void* out, float* lse, const void* out_a, const float* lse_a, const void* out_b,
                                           const float* lse_b, int64_t num_rows, int num_head, int dim, int64_t out_row_stride,
                                           int64_t out_head_stride, int64_t a_row_stride, int64_t a_head_stride, int64_t b_row_stride,
                                           int64_t b_head_stride, hipStream_t stream) {
  using namespace hpc::merge_states;
  const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  const int64_t strides[6] = {out_row_stride, out_head_stride, a_row_stride, a_head_stride, b_row_stride, b_head_stride};
  const MergeRoute r = merge_route(addr(out), addr(lse), addr(out_a), addr(lse_a), addr(out_b), addr(lse_b), num_rows, num_head, dim,
                                   strides);
  if (r.code != HPC_OK || r.empty) return r.code;
  // outputs may be the a side exactly (same base, same strides: in place); any other overlap of an output with an input is refused
  const ByteSpan so = byte_span(out, num_rows, out_row_stride, num_head, out_head_stride, dim, 2);
  const ByteSpan sa = byte_span(out_a, num_rows, a_row_stride, num_head, a_head_stride, dim, 2);
  const ByteSpan sb = byte_span(out_b, num_rows, b_row_stride, num_head, b_head_stride, dim, 2);
  const ByteSpan sl = byte_span(lse, num_rows, num_head, num_head, 1, 1, 4), sla = byte_span(lse_a, num_rows, num_head, num_head, 1, 1, 4);
  const ByteSpan slb = byte_span(lse_b, num_rows, num_head, num_head, 1, 1, 4);
  const bool o_in_place = out == out_a && out_row_stride == a_row_stride && out_head_stride == a_head_stride;
  if ((!o_in_place && overlap(so, sa)) || overlap(so, sb) || (lse != lse_a && overlap(sl, sla)) || overlap(sl, slb) ||
      overlap(so, sla) || overlap(so, slb) || overlap(so, sl) || overlap(sl, sa) || overlap(sl, sb))
    return HPC_ERR_UNSUPPORTED;
  const Args p{static_cast<uint16_t*>(out), lse, static_cast<const uint16_t*>(out_a), lse_a, static_cast<const uint16_t*>(out_b), lse_b,
               num_rows * num_head, num_head, r.lanes_per_row, r.rows_per_wg,
               out_row_stride, out_head_stride, a_row_stride, a_head_stride, b_row_stride, b_head_stride};
  merge_attn_states_kernel<<<dim3(static_cast<unsigned>(r.grid)), kMergeThreads, 0, stream>>>(p);
  HPC_CHECK_LAUNCH();
  return HPC_OK;
}
