// C++ host side of the dense FP8 linear with 128-block scales (csrc/gemm_blockwise_fp8.hip): gemm_blockwise_fp8, the consumer
// of the (x, x_scale) pair blockwise_fp8_quant / fused_rmsnorm_blockwise_quant write.  Ours only (no reference op; pinned to the
// PyTorch statement tests/linear_fp8_ref.py), so under its own namespace: torch.ops.hpc_linear.* (hpc:: holds the reference's
// surface).  With `output` given nothing is allocated per call beyond the cached scratch and the call captures into a hipGraph.
// No kernels here.
#include "torch_common.h"

using namespace hpc_torch;

namespace {

// Split-K scratch of one call: [kLinearCounterBytes of arrival counters, zero-once | fp32 partial planes].  The counters sit in
// a prefix of ONE size whatever the shape, so that calls of different shapes share the buffer of their stream and no call's
// planes ever land on another call's counters; the counts and sizes are hpc_gemm_blockwise_fp8_plan's.
constexpr int64_t kLinearCounterBytes = 1 << 16;

at::Tensor gemm_blockwise_fp8(const at::Tensor& x, const at::Tensor& x_scale, const at::Tensor& weight,
                              const at::Tensor& weight_scale, const c10::optional<at::Tensor>& output, int64_t splits) {
  cuda_contig(x, "x");
  cuda_contig(x_scale, "x_scale");
  cuda_contig(weight, "weight");
  TORCH_CHECK(weight_scale.is_cuda(), "weight_scale tensor must be cuda");
  TORCH_CHECK(x_scale.device() == x.device() && weight.device() == x.device() && weight_scale.device() == x.device(),
              "x_scale, weight and weight_scale must be on x's device");
  TORCH_CHECK(x.scalar_type() == kF8, "x dtype must be float8_e4m3fn");
  TORCH_CHECK(weight.scalar_type() == kF8, "weight dtype must be float8_e4m3fn");
  TORCH_CHECK(x_scale.scalar_type() == at::kFloat, "x_scale dtype must be float32");
  TORCH_CHECK(weight_scale.scalar_type() == at::kFloat, "weight_scale dtype must be float32");
  TORCH_CHECK(x.dim() == 2, "x must be [num_tokens, k]");
  TORCH_CHECK(weight.dim() == 2, "weight must be [n, k]");
  const int64_t m = x.size(0), k = x.size(1), n = weight.size(0);
  TORCH_CHECK(weight.size(1) == k, "weight must be [n, k] with x's k = ", k, ", got k = ", weight.size(1));
  TORCH_CHECK(k % 128 == 0 && k >= 128, "k must be a multiple of 128, at least 128, got ", k);
  TORCH_CHECK(n % 64 == 0 && n >= 64, "n must be a multiple of 64, at least 64, got ", n);
  TORCH_CHECK(n * k <= 0xfffffff0ll, "weight of ", n, " x ", k, " bytes is beyond 32-bit offsets");
  TORCH_CHECK(m <= 256, "gemm_blockwise_fp8 serves decode batches of at most 256 tokens, got ", m,
              "; use group_gemm_blockwise_fp8 for prefill-sized calls");
  const int64_t kb = k / 128;
  TORCH_CHECK(x_scale.dim() == 2 && x_scale.size(0) == m && x_scale.size(1) == kb, "x_scale must be [num_tokens, k / 128] = [", m,
              ", ", kb, "]");
  TORCH_CHECK(weight_scale.dim() == 2 && weight_scale.size(0) == (n + 127) / 128 && weight_scale.size(1) == kb,
              "weight_scale must be [ceil(n / 128), k / 128] = [", (n + 127) / 128, ", ", kb, "]");
  TORCH_CHECK(weight_scale.stride(1) == 1, "weight_scale must have contiguous inner dim (stride(1)=1), got stride(1)=",
              weight_scale.stride(1));
  TORCH_CHECK(weight_scale.stride(0) >= kb, "weight_scale stride(0)=", weight_scale.stride(0), " must be >= k / 128 = ", kb);
  TORCH_CHECK(splits >= 0, "splits must be 0 (the library chooses) or a count, got ", splits);
  at::Tensor y = out_or_new(output, x, {m, n}, at::kBFloat16, "output", kOnInputDevice);
  if (m == 0) return y;

  int s = 0, max_splits = 0, counters = 0;
  int64_t plane_bytes = 0;
  const int rc_plan = hpc_gemm_blockwise_fp8_plan(i32(m), i32(n), i32(k), i32(std::min<int64_t>(splits, INT32_MAX)),
                                                  hpc_get_cu_count(x.device().index()), &s, &max_splits, &plane_bytes, &counters);
  TORCH_CHECK(splits <= max_splits, "splits = ", splits, " is beyond the ", max_splits, " this shape allows (min(16, k / 128))");
  HPC_LAUNCH_CHECK(rc_plan, "gemm_blockwise_fp8");
  void* planes = nullptr;
  void* cnt = nullptr;
  at::Tensor ws, big_cnt;
  if (s > 1) {
    if (int64_t{counters} * 4 <= kLinearCounterBytes) {
      ws = cached_scratch(kScratchLinear, x, kLinearCounterBytes + plane_bytes, kLinearCounterBytes);
      cnt = ws.data_ptr();
      planes = static_cast<uint8_t*>(ws.data_ptr()) + kLinearCounterBytes;
    } else {  // more tiles than the shared prefix counts (a caller's split of a very tall weight): this call's own buffers
      big_cnt = at::zeros({counters}, x.options().dtype(at::kInt));
      ws = at::empty({plane_bytes}, x.options().dtype(at::kByte));
      cnt = big_cnt.data_ptr();
      planes = ws.data_ptr();
    }
  }
  const int rc = hpc_gemm_blockwise_fp8_async(ptr(y), ptr(x), static_cast<const float*>(x_scale.data_ptr()), ptr(weight),
                                              static_cast<const float*>(weight_scale.data_ptr()), i32(m), i32(n), i32(k),
                                              weight_scale.stride(0), s, planes, plane_bytes, cnt, stream_of(x));
  HPC_LAUNCH_CHECK(rc, "gemm_blockwise_fp8");
  return y;
}

}  // namespace

TORCH_LIBRARY(hpc_linear, m) {
  m.def(
      "gemm_blockwise_fp8(Tensor x, Tensor x_scale, Tensor weight, Tensor weight_scale, Tensor? output, int splits) -> Tensor");
}

TORCH_LIBRARY_IMPL(hpc_linear, CUDA, m) { m.impl("gemm_blockwise_fp8", &gemm_blockwise_fp8); }
