// C++ host side of token_logprobs: the log-probability, rank and top-N of the token a row emitted (kernels: csrc/sampler.hip,
// hpc_token_logprobs_async).  Ours only (no reference op; pinned to the PyTorch statement tests/token_logprobs_ref.py), so
// under its own namespace: torch.ops.hpc_logprobs.* (hpc:: holds the reference's surface).  All four outputs may be passed
// in.  No kernels here.
#include "torch_common.h"

using namespace hpc_torch;

namespace {

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> token_logprobs(
    const at::Tensor& logits, const at::Tensor& token_ids, const c10::optional<at::Tensor>& temperature, double temperature_val,
    int64_t num_top, const c10::optional<at::Tensor>& token_logprobs_out, const c10::optional<at::Tensor>& token_ranks,
    const c10::optional<at::Tensor>& top_ids, const c10::optional<at::Tensor>& top_logprobs) {
  const char* who = "token_logprobs";
  const LogitsDims d = check_logits(logits, who, /*nonempty_vocab=*/true);
  const int64_t rows = d.b, v = d.v;
  TORCH_CHECK(rows <= INT32_MAX, who, ": logits rows must fit an int32, got ", rows);

  TORCH_CHECK(token_ids.is_cuda() && token_ids.device() == logits.device(), "token_ids must be on the logits' device");
  TORCH_CHECK(token_ids.is_contiguous(), "token_ids tensor must be contiguous");
  TORCH_CHECK(token_ids.scalar_type() == at::kInt || token_ids.scalar_type() == at::kLong, "token_ids dtype must be int32 or int64");
  TORCH_CHECK(token_ids.numel() == rows, who, ": token_ids must have one element per logits row = ", rows, ", got ",
              token_ids.numel());

  int64_t count = 0;
  if (temperature.has_value()) {
    const at::Tensor& t = *temperature;
    check_same_device(t, "temperature", &logits);
    TORCH_CHECK(t.is_contiguous(), "temperature tensor must be contiguous");
    TORCH_CHECK(t.scalar_type() == at::kFloat, "temperature dtype must be float32");
    count = t.numel();
    TORCH_CHECK(count >= 1 && rows % count == 0, who, ": temperature must have a number of elements that divides the logits rows = ",
                rows, ", got ", count);
  } else {
    TORCH_CHECK(temperature_val >= 0.0, who, ": scalar temperature must be >= 0, got ", temperature_val);
  }
  TORCH_CHECK(num_top >= 0 && num_top <= 32, who, ": num_top must be in [0, 32], got ", num_top);
  TORCH_CHECK(num_top <= v, who, ": num_top must be <= vocab_size = ", v, ", got ", num_top);

  at::Tensor lp = out_or_new(token_logprobs_out, logits, {rows}, at::kFloat, "token_logprobs", kOnLogitsDevice);
  at::Tensor rank = out_or_new(token_ranks, logits, {rows}, at::kInt, "token_ranks", kOnLogitsDevice);
  at::Tensor ids = out_or_new(top_ids, logits, {rows, num_top}, at::kInt, "top_ids", kOnLogitsDevice);
  at::Tensor tlp = out_or_new(top_logprobs, logits, {rows, num_top}, at::kFloat, "top_logprobs", kOnLogitsDevice);
  if (rows == 0) return std::make_tuple(lp, rank, ids, tlp);
  at::Tensor ws = at::empty({hpc_token_logprobs_workspace_bytes(i32(rows), i32(num_top), i32(v))}, logits.options().dtype(at::kByte));
  const int rc = hpc_token_logprobs_async(
      ptr(lp), ptr(rank), num_top ? ptr(ids) : nullptr, num_top ? ptr(tlp) : nullptr, ptr(ws), ptr(logits),
      logits.scalar_type() == at::kFloat ? 0 : 1, logits.stride(0), ptr(token_ids), token_ids.scalar_type() == at::kLong ? 8 : 4,
      ptr(temperature), i32(count), static_cast<float>(temperature_val), i32(rows), i32(num_top), i32(v), stream_of(logits));
  HPC_LAUNCH_CHECK(rc, "token_logprobs");
  return std::make_tuple(lp, rank, ids, tlp);
}

}  // namespace

TORCH_LIBRARY(hpc_logprobs, m) {
  m.def(
      "token_logprobs(Tensor logits, Tensor token_ids, Tensor? temperature, float temperature_val, int num_top, "
      "Tensor? token_logprobs, Tensor? token_ranks, Tensor? top_ids, Tensor? top_logprobs) -> (Tensor, Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(hpc_logprobs, CUDA, m) {
  m.impl("token_logprobs", &token_logprobs);
}
