// C++ host side of the 128-block activation quantisers (csrc/blockwise_quant.hip): blockwise_fp8_quant and
// fused_rmsnorm_blockwise_quant, the producers of the (x, x_scale) pair of fuse_moe_blockwise* / group_gemm_blockwise_fp8.
// Ours only (no reference op; pinned to the PyTorch statement tests/blockwise_quant_ref.py), so under their own namespace:
// torch.ops.hpc_quant.* (hpc:: holds the reference's surface).  Every output may be passed in; then nothing is allocated
// and the call captures into a hipGraph.  No kernels here.
#include "torch_common.h"

using namespace hpc_torch;

namespace {

// [T, H] with H % 128 == 0 and 128 <= H <= 16384
void check_rows(const at::Tensor& t, const char* name) {
  cuda_contig(t, name);
  TORCH_CHECK(t.dim() == 2, name, " must be [num_tokens, hidden]");
  const int64_t h = t.size(1);
  TORCH_CHECK(h % 128 == 0 && h >= 128 && h <= 16384, "hidden must be a multiple of 128 in 128..16384, got ", h);
  TORCH_CHECK(t.size(0) <= INT32_MAX, "too many rows");
}

std::tuple<at::Tensor, at::Tensor> blockwise_fp8_quant(const at::Tensor& input, const c10::optional<at::Tensor>& output,
                                                       const c10::optional<at::Tensor>& output_scale) {
  check_rows(input, "input");
  const auto st = input.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16, "input dtype must be float32, float16, or bfloat16");
  const int64_t t = input.size(0), h = input.size(1);
  at::Tensor q = out_or_new(output, input, {t, h}, kF8, "output", kOnInputDevice);
  at::Tensor sc = out_or_new(output_scale, input, {t, h / 128}, at::kFloat, "output_scale", kOnInputDevice);
  if (t == 0) return std::make_tuple(q, sc);
  const int in_dtype = st == at::kBFloat16 ? 0 : (st == at::kHalf ? 1 : 2);
  const int rc = hpc_blockwise_fp8_quant_async(ptr(q), static_cast<float*>(sc.data_ptr()), ptr(input), in_dtype, i32(t), i32(h),
                                               stream_of(input));
  HPC_LAUNCH_CHECK(rc, "blockwise_fp8_quant");
  return std::make_tuple(q, sc);
}

// returns (q, scale, normed); normed is an empty [0] tensor without return_normed
std::tuple<at::Tensor, at::Tensor, at::Tensor> fused_rmsnorm_blockwise_quant(
    const at::Tensor& a, const at::Tensor& weight, double eps, const c10::optional<at::Tensor>& residual, bool return_normed,
    const c10::optional<at::Tensor>& output, const c10::optional<at::Tensor>& output_scale,
    const c10::optional<at::Tensor>& output_normed) {
  check_rows(a, "a");
  TORCH_CHECK(a.scalar_type() == at::kBFloat16, "a dtype must be bfloat16");
  const int64_t t = a.size(0), h = a.size(1);
  cuda_contig(weight, "weight");
  TORCH_CHECK(weight.device() == a.device(), "weight must be on a's device");
  TORCH_CHECK(weight.scalar_type() == at::kBFloat16, "weight dtype must be bfloat16");
  TORCH_CHECK((weight.dim() == 1 && weight.size(0) == h) || (weight.dim() == 2 && weight.size(0) == 1 && weight.size(1) == h),
              "weight must be [hidden] or [1, hidden]");
  if (residual.has_value()) {
    const at::Tensor& r = *residual;
    cuda_contig(r, "residual");
    TORCH_CHECK(r.device() == a.device(), "residual must be on a's device");
    TORCH_CHECK(r.scalar_type() == at::kBFloat16, "residual dtype must be bfloat16");
    TORCH_CHECK(r.sizes() == a.sizes(), "residual shape must match a");
  }
  TORCH_CHECK(return_normed || !output_normed.has_value(), "output_normed needs return_normed");
  at::Tensor q = out_or_new(output, a, {t, h}, kF8, "output", kOnInputDevice);
  at::Tensor sc = out_or_new(output_scale, a, {t, h / 128}, at::kFloat, "output_scale", kOnInputDevice);
  at::Tensor y = return_normed ? out_or_new(output_normed, a, {t, h}, at::kBFloat16, "output_normed", kOnInputDevice)
                               : at::empty({0}, a.options());
  if (t == 0) return std::make_tuple(q, sc, y);
  const int rc = hpc_fused_rmsnorm_blockwise_quant_async(ptr(q), static_cast<float*>(sc.data_ptr()),
                                                         return_normed ? ptr(y) : nullptr, ptr(a), ptr(weight), ptr(residual),
                                                         static_cast<float>(eps), i32(t), i32(h), stream_of(a));
  HPC_LAUNCH_CHECK(rc, "fused_rmsnorm_blockwise_quant");
  return std::make_tuple(q, sc, y);
}

}  // namespace

TORCH_LIBRARY(hpc_quant, m) {
  m.def("blockwise_fp8_quant(Tensor input, Tensor? output, Tensor? output_scale) -> (Tensor, Tensor)");
  m.def(
      "fused_rmsnorm_blockwise_quant(Tensor a, Tensor weight, float eps, Tensor? residual, bool return_normed, Tensor? output, "
      "Tensor? output_scale, Tensor? output_normed) -> (Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(hpc_quant, CUDA, m) {
  m.impl("blockwise_fp8_quant", &blockwise_fp8_quant);
  m.impl("fused_rmsnorm_blockwise_quant", &fused_rmsnorm_blockwise_quant);
}
