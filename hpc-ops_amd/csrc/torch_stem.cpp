// C++ host side of the Stem block-sparse mask ops (prep_paged_kv, prep_varlen_q, oam_gemm, tpd).
//
// Mirrors the reference's entries src/stem/entry.cc:19-266 and registrations :268-295 - schemas verbatim, the same
// refusals with the same messages, the same output shapes (the prep ops size their outputs from kv_seq_lens.max() /
// q_seq_lens.max(), a host read, as the reference does) - with the compute behind the C-ABI (csrc/stem.hip).
// The ops live in their own namespace, torch.ops.hpc_stem.*, not hpc::.  Beyond the reference's
// checks, dtypes, contiguity and the sizes the kernels index with are checked too, so that no kernel reads outside an
// argument.
#include "torch_common.h"

using namespace hpc_torch;

namespace {

void int32_1d(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.scalar_type() == at::kInt && t.is_contiguous(), name, " must be contiguous int32");
}

// reference stem_oam_prep_paged_kv_entry (:19-110)
std::tuple<at::Tensor, at::Tensor> stem_oam_prep_paged_kv(const at::Tensor& kcache, const at::Tensor& vcache,
                                                          const at::Tensor& kscale, const at::Tensor& vscale,
                                                          const at::Tensor& kv_indices, const at::Tensor& kv_seq_lens,
                                                          double lambda_mag, int64_t stem_block_size, int64_t stem_stride,
                                                          int64_t quant_type) {
  TORCH_CHECK(kcache.is_cuda(), "kcache must be CUDA tensor");
  TORCH_CHECK(vcache.is_cuda(), "vcache must be CUDA tensor");
  TORCH_CHECK(kscale.is_cuda(), "kscale must be CUDA tensor");
  TORCH_CHECK(vscale.is_cuda(), "vscale must be CUDA tensor");
  TORCH_CHECK(kv_indices.is_cuda(), "kv_indices must be CUDA tensor");
  TORCH_CHECK(kv_seq_lens.is_cuda(), "kv_seq_lens must be CUDA tensor");
  TORCH_CHECK((quant_type == 0 || quant_type == 1), "quant_type only support 0/1");
  TORCH_CHECK((kscale.element_size() == 4 || kscale.element_size() == 1), "kscale dtype must be float or fp8");
  TORCH_CHECK(stem_block_size == 128 && stem_stride == 16,
              "stem_oam_prep_paged_kv: only stem_block_size=128, stem_stride=16 is supported");
  TORCH_CHECK(kcache.dim() == 4 && vcache.dim() == 4, "kcache / vcache must be [num_blocks, kv_block_size, num_head_kv, dim]");
  const int64_t block_size = kcache.size(1);
  TORCH_CHECK(block_size == 32 || block_size == 64, "stem_oam_prep_paged_kv: kv_block_size must be 32 or 64, got ", block_size);
  const int64_t num_head_kv = kcache.size(2), num_dim_qk = kcache.size(3), num_dim_v = vcache.size(3);
  const int64_t num_batch = kv_seq_lens.size(0), num_seq_max_blocks = kv_indices.size(1);
  TORCH_CHECK(num_dim_qk == 128 && num_dim_v == 128, "stem_oam_prep_paged_kv: unsupported dim_qk=", num_dim_qk, " dim_v=",
              num_dim_v, " (expected dim_qk=128, dim_v=128)");
  TORCH_CHECK(kcache.scalar_type() == at::kFloat8_e4m3fn && vcache.scalar_type() == at::kFloat8_e4m3fn,
              "kcache / vcache dtype must be float8_e4m3fn");
  TORCH_CHECK(kcache.stride(3) == 1 && vcache.stride(3) == 1 && vcache.size(1) == block_size && vcache.size(2) == num_head_kv,
              "kcache / vcache must have contiguous head dims and the same page shape");
  int32_1d(kv_seq_lens, "kv_seq_lens");
  TORCH_CHECK(kv_indices.dim() == 2 && kv_indices.size(0) >= num_batch, "kv_indices must be [num_batch, max_blocks_per_req]");
  int32_1d(kv_indices, "kv_indices");
  TORCH_CHECK(vscale.scalar_type() == at::kFloat && vscale.numel() >= (quant_type == 0 ? num_head_kv : 1),
              "vscale must be float32 [1] (quant_type 1) or [num_head_kv] (quant_type 0)");
  int64_t ks[3] = {0, 0, 0};
  if (quant_type == 0) {
    TORCH_CHECK(kscale.dim() == 4 && kscale.stride(3) == 1, "per-token kscale must be [num_blocks, scale_rows, num_head_kv, dim]");
    const int64_t div = kscale.element_size() == 1 ? static_cast<int64_t>(sizeof(float)) : 1;
    TORCH_CHECK(kscale.element_size() == 4 ? kscale.scalar_type() == at::kFloat
                                           : (kscale.stride(0) % 4 == 0 && kscale.stride(1) % 4 == 0 && kscale.stride(2) % 4 == 0),
                "kscale must be float32 or an fp8 view of float32 storage");
    TORCH_CHECK(kscale.size(1) * 32 >= block_size && kscale.size(2) == num_head_kv && kscale.size(3) * kscale.element_size() >= 128,
                "kscale must hold one scale per token of a page: [num_blocks, kv_block_size / 32, num_head_kv, 32] as float32");
    ks[0] = kscale.stride(0) / div, ks[1] = kscale.stride(1) / div, ks[2] = kscale.stride(2) / div;
  } else {
    TORCH_CHECK(kscale.scalar_type() == at::kFloat && kscale.numel() >= 1, "kscale must be float32 [1]");
  }
  const int64_t max_kv_len = num_batch > 0 ? kv_seq_lens.max().item<int64_t>() : 0;
  TORCH_CHECK(max_kv_len <= num_seq_max_blocks * block_size, "stem_oam_prep_paged_kv: kv_seq_lens exceed the page table");
  const int64_t max_kv_padded = ((max_kv_len + stem_block_size - 1) / stem_block_size) * stem_block_size;
  const int64_t max_num_stem_blocks = max_kv_padded / stem_block_size;
  const int64_t max_k_down_len = max_kv_padded / stem_stride;
  auto kflat = at::empty({num_batch, num_head_kv, max_num_stem_blocks, stem_stride * num_dim_qk}, kcache.options().dtype(at::kBFloat16));
  auto vbias = at::empty({num_batch, num_head_kv, max_num_stem_blocks}, kcache.options().dtype(at::kFloat));
  auto v_norm_down = at::empty({num_batch, num_head_kv, max_k_down_len}, kcache.options().dtype(at::kFloat));
  const int rc = hpc_stem_oam_prep_paged_kv_async(
      ptr(kflat), ptr(vbias), ptr(v_norm_down), ptr(kcache), ptr(vcache), ptr(kscale), ptr(vscale), ptr(kv_indices),
      ptr(kv_seq_lens), i32(quant_type), i32(num_batch), i32(num_dim_qk), i32(num_dim_v), i32(num_head_kv), i32(block_size),
      i32(num_seq_max_blocks), i32(stem_block_size), i32(stem_stride), i32(max_num_stem_blocks), static_cast<float>(lambda_mag),
      kcache.stride(0), kcache.stride(1), kcache.stride(2), vcache.stride(0), vcache.stride(1), vcache.stride(2), ks[0], ks[1],
      ks[2], stream_of(kcache));
  HPC_LAUNCH_CHECK(rc, "stem_oam_prep_paged_kv");
  return std::make_tuple(kflat, vbias);
}

// reference stem_oam_prep_varlen_q_entry (:114-155)
at::Tensor stem_oam_prep_varlen_q(const at::Tensor& q_fp8, const at::Tensor& qscale, const at::Tensor& q_seq_lens,
                                  const at::Tensor& cu_seqlens_q, int64_t stem_block_size, int64_t stem_stride) {
  TORCH_CHECK(q_fp8.is_cuda(), "q_fp8 must be CUDA tensor");
  TORCH_CHECK(q_fp8.is_contiguous(), "q_fp8 must be contiguous");
  TORCH_CHECK(qscale.is_cuda(), "qscale must be CUDA tensor");
  TORCH_CHECK(q_seq_lens.is_cuda(), "q_seq_lens must be CUDA tensor");
  TORCH_CHECK(cu_seqlens_q.is_cuda(), "cu_seqlens_q must be CUDA tensor");
  TORCH_CHECK(stem_block_size == 128 && stem_stride == 16,
              "stem_oam_prep_varlen_q: only stem_block_size=128, stem_stride=16 is supported");
  TORCH_CHECK(q_fp8.dim() == 3, "q_fp8 must be [total_tokens, num_q_heads, dim_qk]");
  const int64_t num_head_q = q_fp8.size(1), num_dim_qk = q_fp8.size(2), num_batch = q_seq_lens.size(0);
  TORCH_CHECK(num_dim_qk == 128, "stem_oam_prep_varlen_q: expected dim_qk=128, got ", num_dim_qk);
  TORCH_CHECK(qscale.dim() == 3, "stem_oam_prep_varlen_q: qscale must be [B, Hq, max_q_pad]");
  TORCH_CHECK(q_fp8.scalar_type() == at::kFloat8_e4m3fn, "q_fp8 dtype must be float8_e4m3fn");
  TORCH_CHECK(qscale.scalar_type() == at::kFloat && qscale.stride(2) == 1 && qscale.size(0) >= num_batch &&
                  qscale.size(1) == num_head_q,
              "qscale must be float32 [num_batch, num_q_heads, max_seq_q_pad] with a contiguous last dim");
  int32_1d(q_seq_lens, "q_seq_lens");
  int32_1d(cu_seqlens_q, "cu_seqlens_q");
  TORCH_CHECK(cu_seqlens_q.numel() >= num_batch + 1, "cu_seqlens_q must be [num_batch + 1]");
  const int64_t max_q_len = num_batch > 0 ? q_seq_lens.max().item<int64_t>() : 0;
  TORCH_CHECK(max_q_len <= qscale.size(2), "stem_oam_prep_varlen_q: qscale holds fewer tokens than q_seq_lens.max()");
  const int64_t max_q_padded = ((max_q_len + stem_block_size - 1) / stem_block_size) * stem_block_size;
  const int64_t max_num_q_blocks = max_q_padded / stem_block_size;
  auto qflat = at::empty({num_batch, num_head_q, max_num_q_blocks, stem_stride * num_dim_qk}, q_fp8.options().dtype(at::kBFloat16));
  const int rc = hpc_stem_oam_prep_varlen_q_async(ptr(qflat), ptr(q_fp8), ptr(qscale), ptr(q_seq_lens), ptr(cu_seqlens_q),
                                                  i32(num_batch), i32(num_head_q), i32(num_dim_qk), i32(stem_block_size),
                                                  i32(stem_stride), i32(max_num_q_blocks), q_fp8.stride(0), qscale.stride(0),
                                                  qscale.stride(1), stream_of(q_fp8));
  HPC_LAUNCH_CHECK(rc, "stem_oam_prep_varlen_q");
  return qflat;
}

// reference stem_oam_gemm_entry (:157-222); every element is written by the kernel, so no -inf fill and no slice copy
at::Tensor stem_oam_gemm(const at::Tensor& qflat, const at::Tensor& kflat, const at::Tensor& vbias, const at::Tensor& q_seq_lens,
                         const at::Tensor& kv_seq_lens, int64_t stem_block_size, int64_t stem_stride, bool causal) {
  TORCH_CHECK(qflat.is_cuda(), "qflat must be CUDA tensor");
  TORCH_CHECK(kflat.is_cuda(), "kflat must be CUDA tensor");
  TORCH_CHECK(vbias.is_cuda(), "vbias must be CUDA tensor");
  TORCH_CHECK(q_seq_lens.is_cuda(), "q_seq_lens must be CUDA tensor");
  TORCH_CHECK(kv_seq_lens.is_cuda(), "kv_seq_lens must be CUDA tensor");
  TORCH_CHECK(stem_block_size == 128 && stem_stride == 16, "stem_oam_gemm: only stem_block_size=128, stem_stride=16 is supported");
  TORCH_CHECK(qflat.dim() == 4 && kflat.dim() == 4 && vbias.dim() == 3, "qflat / kflat must be 4-D and vbias 3-D");
  const int64_t num_batch = qflat.size(0), num_head_q = qflat.size(1), max_num_qb = qflat.size(2), kflat_inner = qflat.size(3);
  const int64_t num_head_kv = kflat.size(1), max_num_kb = kflat.size(2);
  TORCH_CHECK(qflat.size(0) == kflat.size(0), "stem_oam_gemm: batch size mismatch between qflat and kflat");
  TORCH_CHECK(qflat.size(3) == kflat.size(3), "stem_oam_gemm: kFlatDim mismatch between qflat (", qflat.size(3), ") and kflat (",
              kflat.size(3), ")");
  TORCH_CHECK(num_head_kv > 0 && num_head_q % num_head_kv == 0, "stem_oam_gemm: num_head_q (", num_head_q,
              ") must be divisible by num_head_kv (", num_head_kv, ")");
  TORCH_CHECK(vbias.size(0) == num_batch && vbias.size(1) == num_head_kv && vbias.size(2) == max_num_kb,
              "stem_oam_gemm: vbias shape mismatch, expected [", num_batch, ", ", num_head_kv, ", ", max_num_kb, "]");
  const int64_t num_dim_qk = kflat_inner / stem_stride;
  TORCH_CHECK(num_dim_qk == 128, "stem_oam_gemm: expected dim_qk=128, got ", num_dim_qk);
  TORCH_CHECK(qflat.scalar_type() == at::kBFloat16 && kflat.scalar_type() == at::kBFloat16 && vbias.scalar_type() == at::kFloat,
              "qflat / kflat must be bfloat16 and vbias float32");
  TORCH_CHECK(qflat.is_contiguous() && kflat.is_contiguous() && vbias.is_contiguous(), "qflat / kflat / vbias must be contiguous");
  int32_1d(q_seq_lens, "q_seq_lens");
  int32_1d(kv_seq_lens, "kv_seq_lens");
  TORCH_CHECK(q_seq_lens.numel() >= num_batch && kv_seq_lens.numel() >= num_batch, "q_seq_lens / kv_seq_lens must be [num_batch]");
  auto block_logits = at::empty({num_batch, num_head_q, max_num_qb, max_num_kb}, qflat.options().dtype(at::kBFloat16));
  const int rc = hpc_stem_oam_gemm_async(ptr(block_logits), ptr(qflat), ptr(kflat), ptr(vbias), ptr(q_seq_lens), ptr(kv_seq_lens),
                                         i32(num_batch), i32(num_head_q), i32(num_head_kv), i32(max_num_qb), i32(max_num_kb),
                                         i32(stem_block_size), i32(stem_stride), causal ? 1 : 0, stream_of(qflat));
  HPC_LAUNCH_CHECK(rc, "stem_oam_gemm");
  return block_logits;
}

// reference stem_tpd_entry (:224-266); the kernel writes every mask byte, so the mask is not zero-filled first
at::Tensor stem_tpd(const at::Tensor& block_logits, const at::Tensor& q_seq_lens, const at::Tensor& kv_seq_lens,
                    const at::Tensor& num_prompt_tokens, int64_t block_size, double alpha, int64_t initial_blocks,
                    int64_t window_size, double k_block_num_rate_medium, int64_t k_block_num_bias_medium,
                    double k_block_num_rate_large, int64_t k_block_num_bias_large) {
  TORCH_CHECK(block_logits.is_cuda(), "block_logits must be CUDA tensor");
  TORCH_CHECK(q_seq_lens.is_cuda(), "q_seq_lens must be CUDA tensor");
  TORCH_CHECK(kv_seq_lens.is_cuda(), "kv_seq_lens must be CUDA tensor");
  TORCH_CHECK(num_prompt_tokens.is_cuda(), "num_prompt_tokens must be CUDA tensor");
  TORCH_CHECK(block_logits.scalar_type() == at::kBFloat16, "block_logits must be bfloat16");
  TORCH_CHECK(block_logits.is_contiguous(), "block_logits must be contiguous");
  TORCH_CHECK(q_seq_lens.scalar_type() == at::kInt, "q_seq_lens must be int32, got ", q_seq_lens.scalar_type());
  TORCH_CHECK(kv_seq_lens.scalar_type() == at::kInt, "kv_seq_lens must be int32, got ", kv_seq_lens.scalar_type());
  TORCH_CHECK(num_prompt_tokens.scalar_type() == at::kInt, "num_prompt_tokens must be int32, got ", num_prompt_tokens.scalar_type());
  TORCH_CHECK(block_logits.dim() == 4, "block_logits must be [num_batch, num_heads, max_Qb, max_Kb]");
  const int64_t num_batch = block_logits.size(0), num_heads = block_logits.size(1);
  const int64_t max_Qb = block_logits.size(2), max_Kb = block_logits.size(3);
  TORCH_CHECK(num_prompt_tokens.dim() == 1 && num_prompt_tokens.size(0) == num_batch, "num_prompt_tokens must have shape [num_batch=",
              num_batch, "], got ", num_prompt_tokens.sizes());
  TORCH_CHECK(max_Kb <= 32768, "stem_tpd: max_Kb=", max_Kb, " exceeds 32768 limit");
  TORCH_CHECK(q_seq_lens.is_contiguous() && kv_seq_lens.is_contiguous() && num_prompt_tokens.is_contiguous() &&
                  q_seq_lens.numel() >= num_batch && kv_seq_lens.numel() >= num_batch,
              "q_seq_lens / kv_seq_lens must be contiguous [num_batch]");
  TORCH_CHECK(block_size > 0, "stem_tpd: block_size must be positive");
  auto mask = at::empty({num_batch, num_heads, max_Qb, max_Kb}, block_logits.options().dtype(at::kByte));
  const int rc = hpc_stem_tpd_async(ptr(mask), ptr(block_logits), ptr(q_seq_lens), ptr(kv_seq_lens), ptr(num_prompt_tokens),
                                    i32(num_batch), i32(num_heads), i32(max_Qb), i32(max_Kb), i32(block_size),
                                    static_cast<float>(alpha), i32(initial_blocks), i32(window_size),
                                    static_cast<float>(k_block_num_rate_medium), i32(k_block_num_bias_medium),
                                    static_cast<float>(k_block_num_rate_large), i32(k_block_num_bias_large), stream_of(block_logits));
  HPC_LAUNCH_CHECK(rc, "stem_tpd");
  return mask;
}

}  // namespace

// schema strings verbatim from the reference (src/stem/entry.cc:268-295; tests/test_stem.py), namespace hpc_stem
TORCH_LIBRARY(hpc_stem, m) {
  m.def(
      "stem_oam_prep_paged_kv(Tensor kcache, Tensor vcache, "
      "Tensor kscale, Tensor vscale, Tensor kv_indices, Tensor kv_seq_lens, "
      "float lambda_mag, int stem_block_size, int stem_stride, int quant_type) "
      "-> (Tensor, Tensor)");
  m.def(
      "stem_oam_prep_varlen_q(Tensor q_fp8, Tensor qscale, Tensor q_seq_lens, "
      "Tensor cu_seqlens_q, int stem_block_size, int stem_stride) -> Tensor");
  m.def(
      "stem_oam_gemm(Tensor qflat, Tensor kflat, Tensor vbias, "
      "Tensor q_seq_lens, Tensor kv_seq_lens, "
      "int stem_block_size, int stem_stride, bool causal) -> Tensor");
  m.def(
      "stem_tpd(Tensor block_logits, Tensor q_seq_lens, Tensor kv_seq_lens, "
      "Tensor num_prompt_tokens, "
      "int block_size, float alpha, int initial_blocks, int window_size, "
      "float k_block_num_rate_medium, int k_block_num_bias_medium, "
      "float k_block_num_rate_large, int k_block_num_bias_large) -> Tensor");
}

TORCH_LIBRARY_IMPL(hpc_stem, CUDA, m) {
  m.impl("stem_oam_prep_paged_kv", &stem_oam_prep_paged_kv);
  m.impl("stem_oam_prep_varlen_q", &stem_oam_prep_varlen_q);
  m.impl("stem_oam_gemm", &stem_oam_gemm);
  m.impl("stem_tpd", &stem_tpd);
}
