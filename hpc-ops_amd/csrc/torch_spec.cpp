// C++ host side of draft-token verification at the end of a speculative decode step (kernels: csrc/sampler.hip,
// hpc_speculative_verify_async).  Ours only (no reference op; pinned to the PyTorch statement tests/spec_verify_ref.py), so
// under its own namespace: torch.ops.hpc_spec.* (hpc:: holds the reference's surface).  Both outputs may be passed in.
// No kernels here.
#include "torch_common.h"

using namespace hpc_torch;

namespace {

std::tuple<at::Tensor, at::Tensor> speculative_verify(const at::Tensor& logits, const at::Tensor& draft_token_ids,
                                                      const c10::optional<at::Tensor>& temperature, double temperature_val,
                                                      const c10::optional<at::Tensor>& uniform_samples,
                                                      const c10::optional<at::Tensor>& gumbel_noise, int64_t seed,
                                                      const c10::optional<at::Tensor>& output_token_ids,
                                                      const c10::optional<at::Tensor>& num_accepted) {
  const char* who = "speculative_verify";
  const LogitsDims d = check_logits(logits, who, /*nonempty_vocab=*/true);
  const int64_t rows = d.b, v = d.v;

  TORCH_CHECK(draft_token_ids.is_cuda() && draft_token_ids.device() == logits.device(), "draft_token_ids must be on the logits' device");
  TORCH_CHECK(draft_token_ids.is_contiguous(), "draft_token_ids tensor must be contiguous");
  TORCH_CHECK(draft_token_ids.scalar_type() == at::kLong, "draft_token_ids dtype must be int64");
  TORCH_CHECK(draft_token_ids.dim() == 2, "draft_token_ids must be 2D [batch_size, num_draft]");
  const int64_t b = draft_token_ids.size(0), k = draft_token_ids.size(1);
  TORCH_CHECK(k <= 15, who, ": num_draft must be <= 15, got ", k);
  TORCH_CHECK(rows == b * (k + 1), who, ": logits rows must be batch_size * (num_draft + 1) = ", b * (k + 1), ", got ", rows);
  TORCH_CHECK(rows <= 65535, who, ": batch_size * (num_draft + 1) must be <= 65535, got ", rows);

  check_1d_float(temperature, "temperature", b, &logits);
  if (!temperature.has_value())
    TORCH_CHECK(temperature_val >= 0.0, who, ": scalar temperature must be >= 0, got ", temperature_val);

  TORCH_CHECK(uniform_samples.has_value() == gumbel_noise.has_value(),
              "uniform_samples and gumbel_noise must both be provided or both be omitted");
  if (gumbel_noise.has_value()) {
    const at::Tensor& u = *uniform_samples;
    TORCH_CHECK(u.is_cuda() && u.device() == logits.device(), "uniform_samples must be on the logits' device");
    TORCH_CHECK(u.is_contiguous(), "uniform_samples tensor must be contiguous");
    TORCH_CHECK(u.scalar_type() == at::kFloat, "uniform_samples dtype must be float32");
    TORCH_CHECK(u.dim() == 2 && u.size(0) == b && u.size(1) == k, "uniform_samples shape must be [", b, ", ", k, "]");
    check_noise(gumbel_noise, rows, v, &logits);
  } else {
    TORCH_CHECK(seed > 0, who, ": seed must be > 0 when uniform_samples and gumbel_noise are not provided, got seed=", seed);
  }

  at::Tensor out = out_or_new(output_token_ids, logits, {b, k + 1}, at::kInt, "output_token_ids", kOnLogitsDevice);
  at::Tensor acc = out_or_new(num_accepted, logits, {b}, at::kInt, "num_accepted", kOnLogitsDevice);
  if (b == 0) return std::make_tuple(out, acc);
  at::Tensor ws = at::empty({hpc_speculative_verify_workspace_bytes(i32(b), i32(k), i32(v))}, logits.options().dtype(at::kByte));
  const int rc = hpc_speculative_verify_async(
      ptr(out), ptr(acc), ptr(ws), ptr(logits), logits.scalar_type() == at::kFloat ? 0 : 1, logits.stride(0),
      k ? ptr(draft_token_ids) : nullptr, ptr(temperature), static_cast<float>(temperature_val), ptr(uniform_samples),
      ptr(gumbel_noise), i32(b), i32(k), i32(v), gumbel_noise.has_value() ? 0ull : static_cast<uint64_t>(seed),
      stream_of(logits));
  HPC_LAUNCH_CHECK(rc, "speculative_verify");
  return std::make_tuple(out, acc);
}

}  // namespace

TORCH_LIBRARY(hpc_spec, m) {
  m.def(
      "speculative_verify(Tensor logits, Tensor draft_token_ids, Tensor? temperature, float temperature_val, "
      "Tensor? uniform_samples, Tensor? gumbel_noise, int seed, Tensor? output_token_ids, Tensor? num_accepted) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(hpc_spec, CUDA, m) {
  m.impl("speculative_verify", &speculative_verify);
}
