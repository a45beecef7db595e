// C++ host side of the MXFP4-weight ops (W4A8: e2m1 weights with e8m0 scales per 32 k, e4m3 activations with f32 scales per 128 k):
// the grouped GEMM and the fused MoE on it, in a namespace of their own - torch.ops.hpc_mxfp4.* (torch.ops.hpc carries the
// reference's surface and nothing else, tests/test_schemas.py).  Compute behind the C-ABI (csrc/group_gemm_mxfp4.hip,
// csrc/fuse_moe.hip).  No kernels here.  The Python side (hpc/mxfp4.py) hands the packed dtypes over as uint8 views.
#include "torch_common.h"

using namespace hpc_torch;

namespace {

void aligned16(const at::Tensor& t, const char* name) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0, name, " must be 16-byte aligned");
}

// The refusals of mxfp4_route() (csrc/group_gemm_mxfp4_route.h) in words, in its order; the plan entry has the last say.
void check_shapes(const char* op, int64_t num_group, int64_t m, int64_t x_rows, int64_t n, int64_t k) {
  TORCH_CHECK(num_group > 0 && n > 0 && k > 0, op, ": num_group, n and k must be positive");
  TORCH_CHECK(k % 128 == 0, op, ": k = ", k, " must be a multiple of 128 (four MX blocks of 32 per scaled MFMA)");
  TORCH_CHECK(n % 64 == 0, op, ": n = ", n, " must be a multiple of 64 (a workgroup owns 64 weight rows)");
  TORCH_CHECK(n * k / 2 <= 0xfffffff0ll, op, ": a group's weights (n * k / 2 bytes) must stay within one 32-bit buffer descriptor");
  TORCH_CHECK(x_rows * k <= 0xfffffff0ll, op, ": x (rows * k bytes) must stay within one 32-bit buffer descriptor");
  TORCH_CHECK(num_group <= 65535, op, ": at most 65535 groups");
  const int rc = hpc_group_gemm_mxfp4_plan(i32(num_group), i32(m), i32(x_rows), i32(n), i32(k), nullptr, nullptr, nullptr);
  TORCH_CHECK(rc == 0, op, ": refused (", err_text(rc), ")");
}

at::Tensor group_gemm(const at::Tensor& x, const at::Tensor& x_scale, const at::Tensor& weight, const at::Tensor& weight_scale,
                      const at::Tensor& seqlens, const at::Tensor& cu_seqlens, const c10::optional<at::Tensor>& row_index,
                      const c10::optional<at::Tensor>& output) {
  const char* op = "group_gemm_mxfp4";
  cuda_contig(x, "x");
  cuda_contig(x_scale, "x_scale");
  cuda_contig(weight, "weight");
  cuda_contig(weight_scale, "weight_scale");
  cuda_contig(seqlens, "seqlens");
  cuda_contig(cu_seqlens, "cu_seqlens");
  TORCH_CHECK(x.scalar_type() == kF8 && x.dim() == 2, "x must be float8_e4m3fn [rows, k]");
  TORCH_CHECK(x_scale.scalar_type() == at::kFloat && x_scale.dim() == 2, "x_scale must be float32 [rows, k / 128]");
  TORCH_CHECK(weight.scalar_type() == at::kByte && weight.dim() == 3, "weight must be uint8 [num_group, n, k / 2] (two e2m1 codes per byte)");
  TORCH_CHECK(weight_scale.scalar_type() == at::kByte && weight_scale.dim() == 3, "weight_scale must be uint8 [num_group, n, k / 32] (e8m0)");
  TORCH_CHECK(seqlens.scalar_type() == at::kInt && cu_seqlens.scalar_type() == at::kInt, "seqlens and cu_seqlens dtype must be int32");
  const int64_t x_rows = x.size(0), k = x.size(1), num_group = weight.size(0), n = weight.size(1);
  TORCH_CHECK(weight.size(2) * 2 == k, "x and weight must share the same k");
  TORCH_CHECK(k % 128 == 0, op, ": k = ", k, " must be a multiple of 128 (four MX blocks of 32 per scaled MFMA)");
  TORCH_CHECK(weight_scale.size(0) == num_group && weight_scale.size(1) == n && weight_scale.size(2) == k / 32,
              "weight_scale must be [num_group, n, k / 32]: one e8m0 byte per 32 values");
  TORCH_CHECK(x_scale.size(0) == x_rows && x_scale.size(1) == k / 128, "x_scale must be [rows, k / 128]");
  TORCH_CHECK(seqlens.dim() == 1 && seqlens.size(0) == num_group && cu_seqlens.dim() == 1 && cu_seqlens.size(0) >= num_group,
              "seqlens must be [num_group] and cu_seqlens hold at least num_group entries");
  int64_t m = x_rows;
  if (row_index.has_value()) {
    cuda_contig(*row_index, "row_index");
    TORCH_CHECK(row_index->scalar_type() == at::kInt && row_index->dim() == 1, "row_index must be int32 [m]");
    m = row_index->size(0);
  }
  check_shapes(op, num_group, m, x_rows, n, k);
  const int64_t shape[2] = {m, n};
  at::Tensor y = out_or_new(output, x, shape, at::kBFloat16, "output", kOnInputDevice);
  if (m == 0) return y;
  aligned16(x, "x");
  aligned16(x_scale, "x_scale");
  aligned16(weight, "weight");
  aligned16(weight_scale, "weight_scale");
  aligned16(y, "output");
  const int rc = hpc_group_gemm_mxfp4_async(ptr(y), ptr(x), static_cast<const float*>(x_scale.data_ptr()), ptr(weight),
                                            ptr(weight_scale), static_cast<const int*>(seqlens.data_ptr()),
                                            static_cast<const int*>(cu_seqlens.data_ptr()),
                                            static_cast<const int*>(ptr(row_index)), i32(num_group), i32(m), i32(x_rows), i32(n),
                                            i32(k), stream_of(x));
  HPC_LAUNCH_CHECK(rc, "group_gemm_mxfp4_async");
  return y;
}

at::Tensor fuse_moe(const at::Tensor& x, const at::Tensor& x_scale, const at::Tensor& gate_up_weight,
                    const at::Tensor& gate_up_weight_scale, const at::Tensor& down_weight, const at::Tensor& down_weight_scale,
                    const at::Tensor& topk_ids, const at::Tensor& topk_scale, const c10::optional<at::Tensor>& shared_output,
                    int64_t rank_ep, int64_t /*num_expert_total*/, const c10::optional<at::Tensor>& output) {
  const char* op = "fuse_moe_mxfp4";
  cuda_contig(x, "x");
  cuda_contig(x_scale, "x_scale");
  cuda_contig(gate_up_weight, "gate_up_weight");
  cuda_contig(gate_up_weight_scale, "gate_up_weight_scale");
  cuda_contig(down_weight, "down_weight");
  cuda_contig(down_weight_scale, "down_weight_scale");
  cuda_contig(topk_ids, "topk_ids");
  cuda_contig(topk_scale, "topk_scale");
  TORCH_CHECK(x.scalar_type() == kF8 && x.dim() == 2, "x must be float8_e4m3fn [num_tokens, hidden]");
  TORCH_CHECK(x_scale.scalar_type() == at::kFloat && topk_scale.scalar_type() == at::kFloat, "x_scale and topk_scale dtype must be float32");
  TORCH_CHECK(gate_up_weight.scalar_type() == at::kByte && down_weight.scalar_type() == at::kByte && gate_up_weight.dim() == 3 &&
                  down_weight.dim() == 3,
              "gate_up_weight and down_weight must be uint8 [num_expert, rows, k / 2] (two e2m1 codes per byte)");
  TORCH_CHECK(gate_up_weight_scale.scalar_type() == at::kByte && down_weight_scale.scalar_type() == at::kByte &&
                  gate_up_weight_scale.dim() == 3 && down_weight_scale.dim() == 3,
              "gate_up_weight_scale and down_weight_scale must be uint8 [num_expert, rows, k / 32] (e8m0)");
  TORCH_CHECK(topk_ids.scalar_type() == at::kInt && topk_ids.dim() == 2, "topk_ids must be int32 [num_tokens, num_topk]");
  const int64_t num_tokens = x.size(0), hidden = x.size(1);
  const int64_t num_experts = gate_up_weight.size(0), inter2 = gate_up_weight.size(1), num_topk = topk_ids.size(1);
  const int64_t inter = inter2 / 2;
  TORCH_CHECK(num_tokens == topk_ids.size(0), "x and topk_ids must share the same num_tokens");
  TORCH_CHECK(topk_ids.sizes() == topk_scale.sizes(), "topk_ids and topk_scale must share the same shape");
  TORCH_CHECK(hidden % 128 == 0, op, ": hidden = ", hidden, " must be a multiple of 128");
  TORCH_CHECK(inter2 % 256 == 0, op, ": gate_up_weight.size(1) = ", inter2, " must be a multiple of 256");
  TORCH_CHECK(num_topk >= 1 && num_topk <= 128, "num_topk must be between 1 and 128");
  TORCH_CHECK(gate_up_weight.size(2) * 2 == hidden, "x and gate_up_weight must share the same k");
  TORCH_CHECK(down_weight.size(0) == num_experts && down_weight.size(1) == hidden && down_weight.size(2) * 2 == inter,
              "down_weight must be [num_expert, hidden, intermediate / 2]");
  TORCH_CHECK(gate_up_weight_scale.size(0) == num_experts && gate_up_weight_scale.size(1) == inter2 &&
                  gate_up_weight_scale.size(2) == hidden / 32,
              "gate_up_weight_scale must be [num_expert, 2 * intermediate, hidden / 32]");
  TORCH_CHECK(down_weight_scale.size(0) == num_experts && down_weight_scale.size(1) == hidden && down_weight_scale.size(2) == inter / 32,
              "down_weight_scale must be [num_expert, hidden, intermediate / 32]");
  TORCH_CHECK(x_scale.dim() == 2 && x_scale.size(0) == num_tokens && x_scale.size(1) == hidden / 128, "x_scale must be per 128 blockwise quant");
  if (shared_output.has_value()) {
    cuda_contig(*shared_output, "shared_output");
    TORCH_CHECK(shared_output->scalar_type() == at::kBFloat16, "shared_output tensor dtype must be bfloat16");
    TORCH_CHECK(shared_output->dim() == 2 && shared_output->size(0) == num_tokens && shared_output->size(1) == hidden,
                "shared_output tensor shape must be same as x tensor");
  }
  const int64_t m = num_tokens * num_topk;
  check_shapes(op, num_experts, m, num_tokens, inter2, hidden);
  check_shapes(op, num_experts, m, m, hidden, inter);
  const int64_t shape[2] = {num_tokens, hidden};
  at::Tensor y = out_or_new(output, x, shape, at::kBFloat16, "output", kOnInputDevice);
  if (num_tokens == 0) return y;
  aligned16(x, "x");
  aligned16(x_scale, "x_scale");
  aligned16(gate_up_weight, "gate_up_weight");
  aligned16(gate_up_weight_scale, "gate_up_weight_scale");
  aligned16(down_weight, "down_weight");
  aligned16(down_weight_scale, "down_weight_scale");
  // scratch as the blockwise op's: from the caching allocator per call (inside a capture: from the graph's pool), never zeroed
  const int64_t nbytes = hpc_fuse_moe_mxfp4_workspace_bytes(i32(num_tokens), i32(num_topk), i32(hidden), i32(inter2), i32(num_experts));
  TORCH_CHECK(nbytes >= 0, op, ": workspace size refused");
  at::Tensor ws = at::empty({std::max<int64_t>(nbytes, 256)}, x.options().dtype(at::kByte));
  const int rc = hpc_fuse_moe_mxfp4_async(ptr(y), ptr(ws), ptr(x), ptr(x_scale), ptr(gate_up_weight), ptr(gate_up_weight_scale),
                                          ptr(down_weight), ptr(down_weight_scale), ptr(topk_ids), ptr(topk_scale), ptr(shared_output),
                                          i32(num_tokens), i32(hidden), i32(inter2), i32(num_topk), i32(num_experts), i32(rank_ep),
                                          stream_of(x));
  HPC_LAUNCH_CHECK(rc, "fuse_moe_mxfp4_async");
  return y;
}

}  // namespace

TORCH_LIBRARY(hpc_mxfp4, m) {
  m.def(
      "group_gemm(Tensor x, Tensor x_scale, Tensor weight, Tensor weight_scale, Tensor seqlens, Tensor cu_seqlens, Tensor? row_index, "
      "Tensor? output) -> Tensor");
  m.def(
      "fuse_moe(Tensor x, Tensor x_scale, Tensor gate_up_weight, Tensor gate_up_weight_scale, Tensor down_weight, Tensor "
      "down_weight_scale, Tensor topk_ids, Tensor topk_scale, Tensor? shared_output, int rank_ep, int num_expert_total, Tensor? "
      "output) -> Tensor");
}

TORCH_LIBRARY_IMPL(hpc_mxfp4, CUDA, m) {
  m.impl("group_gemm", &group_gemm);
  m.impl("fuse_moe", &fuse_moe);
}
