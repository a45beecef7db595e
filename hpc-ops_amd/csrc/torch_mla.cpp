// C++ host side of the MLA decode attention over the paged latent KV cache (csrc/attention_decode_mla.hip):
// attention_decode_mla_bf16.  Ours only (no reference op; pinned to the PyTorch statement tests/mla_ref.py), so under its own
// namespace: torch.ops.hpc_mla.* (hpc:: holds the reference's surface).  With `output` (and `output_lse` where an lse is wanted)
// given nothing is allocated per call beyond the cached scratch and the call captures into a hipGraph.  Nothing here reads the
// values of num_seq_kvcache.  No kernels here.
#include "torch_common.h"

using namespace hpc_torch;

namespace {

std::tuple<at::Tensor, at::Tensor> attention_decode_mla_bf16(const at::Tensor& q, const at::Tensor& ckv_cache,
                                                             const at::Tensor& block_ids, const at::Tensor& num_seq_kvcache,
                                                             double softmax_scale, int64_t mtp, bool new_kv_included,
                                                             const c10::optional<at::Tensor>& output,
                                                             const c10::optional<at::Tensor>& output_lse, bool return_lse,
                                                             int64_t splits) {
  cuda_contig(q, "q");
  cuda_contig(block_ids, "block_ids");
  cuda_contig(num_seq_kvcache, "num_seq_kvcache");
  TORCH_CHECK(ckv_cache.is_cuda(), "ckv_cache tensor must be cuda");
  TORCH_CHECK(ckv_cache.device() == q.device() && block_ids.device() == q.device() && num_seq_kvcache.device() == q.device(),
              "ckv_cache, block_ids and num_seq_kvcache must be on q's device");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "q dtype must be bfloat16");
  TORCH_CHECK(ckv_cache.scalar_type() == at::kBFloat16, "ckv_cache dtype must be bfloat16");
  TORCH_CHECK(block_ids.scalar_type() == at::kInt, "block_ids dtype must be int32");
  TORCH_CHECK(num_seq_kvcache.scalar_type() == at::kInt, "num_seq_kvcache dtype must be int32");
  TORCH_CHECK(mtp >= 0 && mtp <= 3, "mtp must be 0 .. 3, got ", mtp);
  const int64_t sq = mtp + 1;
  TORCH_CHECK(q.dim() == 3 && q.size(2) == 576, "q must be [num_batch * num_seq_q, num_head, 576]");
  TORCH_CHECK(ckv_cache.dim() == 3 && ckv_cache.size(2) == 576, "ckv_cache must be [num_blocks, block_size, 576]");
  TORCH_CHECK(block_ids.dim() == 2, "block_ids must be [num_batch, max_blocks]");
  TORCH_CHECK(num_seq_kvcache.dim() == 1, "num_seq_kvcache must be [num_batch]");
  const int64_t b = num_seq_kvcache.size(0), h = q.size(1), page = ckv_cache.size(1);
  TORCH_CHECK(q.size(0) == b * sq, "q must have num_batch * (mtp + 1) = ", b * sq, " rows, got ", q.size(0));
  TORCH_CHECK(block_ids.size(0) == b, "block_ids must have num_batch = ", b, " rows");
  TORCH_CHECK(h % 16 == 0 && h >= 16 && h <= 128, "num_head must be a multiple of 16, 16 .. 128, got ", h);
  TORCH_CHECK(page == 16 || page == 32 || page == 64 || page == 128, "block_size must be 16, 32, 64 or 128, got ", page);
  TORCH_CHECK(ckv_cache.stride(2) == 1, "ckv_cache must have a contiguous last dim");
  TORCH_CHECK(ckv_cache.stride(1) >= 576 && ckv_cache.stride(1) % 8 == 0 && ckv_cache.stride(0) % 8 == 0 &&
                  ckv_cache.stride(0) >= 0,
              "ckv_cache token stride must be >= 576 and, like the block stride, a multiple of 8 elements; got ",
              ckv_cache.stride(1), " and ", ckv_cache.stride(0));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ckv_cache.data_ptr()) % 16 == 0, "ckv_cache must be 16-byte aligned");
  TORCH_CHECK(block_ids.size(1) * page <= (int64_t{1} << 30), "block_ids reaches beyond 2^30 tokens");
  TORCH_CHECK(splits >= 0, "splits must be 0 (the library chooses) or a count, got ", splits);
  at::Tensor out = out_or_new(output, q, {b * sq, h, 512}, at::kBFloat16, "output", kOnInputDevice);
  const bool want_lse = return_lse || output_lse.has_value();
  at::Tensor lse = want_lse ? out_or_new(output_lse, q, {b * sq, h}, at::kFloat, "output_lse", kOnInputDevice)
                            : at::empty({0}, q.options().dtype(at::kFloat));

  int s = 0, max_splits = 0;
  int64_t ws_bytes = 0;
  const int rc_plan = hpc_attention_decode_mla_plan(i32(b), i32(sq), i32(h), i32(std::min<int64_t>(splits, INT32_MAX)),
                                                    b > 0 ? hpc_get_cu_count(q.device().index()) : 256, &s, &max_splits, &ws_bytes);
  TORCH_CHECK(splits <= max_splits, "splits = ", splits, " is beyond the ", max_splits, " pieces a request may be cut into");
  HPC_LAUNCH_CHECK(rc_plan, "attention_decode_mla_bf16");
  if (b == 0) return {out, lse};
  TORCH_CHECK(block_ids.size(1) > 0, "block_ids has no columns");
  at::Tensor ws;
  if (s > 1) ws = cached_scratch(kScratchMla, q, ws_bytes, 0);  // never zeroed: an unwritten piece is never read
  const int rc = hpc_attention_decode_mla_bf16_async(
      ptr(out), want_lse ? static_cast<float*>(lse.data_ptr()) : nullptr, ptr(q), ptr(ckv_cache),
      static_cast<const int*>(block_ids.data_ptr()), static_cast<const int*>(num_seq_kvcache.data_ptr()), i32(b), i32(sq), i32(h),
      i32(page), i32(block_ids.size(1)), ckv_cache.stride(0), ckv_cache.stride(1), static_cast<float>(softmax_scale),
      new_kv_included ? 1 : 0, s, s > 1 ? ws.data_ptr() : nullptr, ws_bytes, stream_of(q));
  HPC_LAUNCH_CHECK(rc, "attention_decode_mla_bf16");
  return {out, lse};
}

}  // namespace

TORCH_LIBRARY(hpc_mla, m) {
  m.def(
      "attention_decode_mla_bf16(Tensor q, Tensor ckv_cache, Tensor block_ids, Tensor num_seq_kvcache, float softmax_scale, "
      "int mtp, bool new_kv_included, Tensor? output, Tensor? output_lse, bool return_lse, int splits) -> (Tensor, Tensor)");
  // the cached split-KV scratch buffers (tests fill them with NaN bytes: no piece that was not written may be read)
  m.def("_workspaces() -> Tensor[]", []() { return list_cached_scratch(kScratchMla); });
}

TORCH_LIBRARY_IMPL(hpc_mla, CUDA, m) { m.impl("attention_decode_mla_bf16", &attention_decode_mla_bf16); }
