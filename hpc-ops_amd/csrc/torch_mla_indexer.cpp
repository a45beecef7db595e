// C++ host side of the DSA lightning indexer (csrc/mla_indexer.hip): mla_indexer_store_k_fp8, mla_indexer_logits_fp8,
// mla_indexer_topk and the fused mla_indexer_topk_fp8, and of its front end mla_indexer_prep_fp8 (csrc/mla_indexer_prep.hip), under torch.ops.hpc_mla.* beside the MLA ops they serve.  Ours only;
// pinned to the PyTorch statements tests/mla_indexer_ref.py and tests/mla_indexer_prep_ref.py.  dtype, device and shape are
// checked here; the cache's rule, the
// limits, strides and alignment are the launchers' (csrc/mla_indexer_route.h) and come back in their words through
// hpc_mla_indexer_*_refusal.  Nothing here reads the values of a length, a page table or a logit; with `output` given nothing is
// allocated per call beyond the cached scratch of the fused op and the calls capture into a hipGraph.  Behind them the same three
// over a ragged prefill chunk (csrc/mla_indexer_prefill.hip): mla_indexer_logits_prefill_fp8, mla_indexer_topk_prefill and the
// fused mla_indexer_topk_prefill_fp8 over row slabs.  No kernels here.
#include "mla_indexer_route.h"
#include "torch_common.h"

using namespace hpc_torch;

namespace {

void check_on(const at::Tensor& t, const char* name, const at::Tensor& like, at::ScalarType dtype, const char* dtype_name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name, " must be a cuda tensor on the device of the op's first tensor");
  TORCH_CHECK(t.scalar_type() == dtype, name, " dtype must be ", dtype_name);
}
void check_table(const at::Tensor& t, const char* name, const at::Tensor& like, int64_t dims) {
  check_on(t, name, like, at::kInt, "int32");
  TORCH_CHECK(t.dim() == dims && t.is_contiguous(), name, " must be a contiguous ", dims, "-d tensor");
}

// [num_blocks, P * 132] uint8 with a contiguous last dim; returns P.  Whether P, the block stride and the base will do is the
// launchers' rule (mla_indexer_cache_check), in its words.
int64_t check_cache(const at::Tensor& c, const at::Tensor& like) {
  check_on(c, "k_cache", like, at::kByte, "uint8");
  TORCH_CHECK(c.dim() == 2 && c.size(1) > 0 && c.size(1) % hpc::kIdxTokenBytes == 0 && c.stride(1) == 1,
              "k_cache must be [num_blocks, block_size * 132] with a contiguous last dim, got ", c.sizes());
  TORCH_CHECK(c.size(0) <= INT32_MAX && c.size(1) / hpc::kIdxTokenBytes <= INT32_MAX, "sizes beyond int32");
  return c.size(1) / hpc::kIdxTokenBytes;
}
// a [0, N] or [1, N] tensor carries any block stride: the launcher is told the contiguous one
int64_t block_stride(const at::Tensor& c) { return c.size(0) > 1 ? c.stride(0) : c.size(1); }

struct Dims {
  int64_t b, sq, h, page, max_blocks;
};
// q, weights, k_cache, block_ids and num_seq_kvcache of the two ops that read the cache
Dims check_reader(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                  const at::Tensor& num_seq_kvcache, int64_t mtp) {
  TORCH_CHECK(q.is_cuda(), "q tensor must be cuda");
  TORCH_CHECK(q.scalar_type() == kF8, "q dtype must be float8_e4m3fn");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == hpc::kIdxDim && q.is_contiguous(), "q must be a contiguous [num_batch * (mtp + 1), num_head, 128]");
  TORCH_CHECK(mtp >= 0 && mtp <= 3, "mtp must be 0 .. 3, got ", mtp);
  const int64_t sq = mtp + 1, h = q.size(1);
  check_on(weights, "weights", q, at::kFloat, "float32");
  TORCH_CHECK(weights.dim() == 2 && weights.size(0) == q.size(0) && weights.size(1) == h && weights.is_contiguous(),
              "weights must be a contiguous [num_batch * (mtp + 1), num_head] = [", q.size(0), ", ", h, "]");
  check_table(block_ids, "block_ids", q, 2);
  check_table(num_seq_kvcache, "num_seq_kvcache", q, 1);
  const int64_t b = num_seq_kvcache.size(0);
  TORCH_CHECK(q.size(0) == b * sq, "q must have num_batch * (mtp + 1) = ", b * sq, " rows, got ", q.size(0));
  TORCH_CHECK(block_ids.size(0) == b, "block_ids must have num_batch = ", b, " rows");
  const int64_t page = check_cache(k_cache, q);
  TORCH_CHECK(b <= INT32_MAX && h <= INT32_MAX && block_ids.size(1) <= INT32_MAX, "sizes beyond int32");
  return {b, sq, h, page, block_ids.size(1)};
}

// ---- mla_indexer_store_k_fp8 ------------------------------------------------------------------------------------------------------
void store_k_fp8(const at::Tensor& k_cache, const at::Tensor& k, const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index,
                 const at::Tensor& block_ids) {
  TORCH_CHECK(k.is_cuda(), "k tensor must be cuda");
  TORCH_CHECK(k.scalar_type() == at::kBFloat16, "k dtype must be bfloat16");
  TORCH_CHECK(k.dim() == 2 && k.size(1) == hpc::kIdxDim && k.stride(1) == 1, "k must be [rows, 128] with a contiguous last dim");
  const int64_t rows = k.size(0);
  check_table(num_seqlen_per_req, "num_seqlen_per_req", k, 1);
  const int64_t num_req = num_seqlen_per_req.size(0);
  check_table(q_index, "q_index", k, 1);
  TORCH_CHECK(q_index.size(0) == num_req + 1, "q_index must be [num_req + 1] = [", num_req + 1, "]");
  check_table(block_ids, "block_ids", k, 2);
  TORCH_CHECK(block_ids.size(0) == num_req, "block_ids must have num_req = ", num_req, " rows");
  const int64_t page = check_cache(k_cache, k);
  TORCH_CHECK(rows <= INT32_MAX && num_req < INT32_MAX && block_ids.size(1) <= INT32_MAX, "sizes beyond int32");
  const int64_t k_rs = rows > 1 ? k.stride(0) : hpc::kIdxDim;
  const auto ip = [](const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); };
  const char* why = hpc_mla_indexer_store_k_fp8_refusal(ptr(k_cache), ptr(k), ip(num_seqlen_per_req), ip(q_index), ip(block_ids),
                                                        i32(rows), i32(num_req), i32(page), i32(block_ids.size(1)),
                                                        i32(k_cache.size(0)), block_stride(k_cache), k_rs);
  TORCH_CHECK(why == nullptr, "mla_indexer_store_k_fp8: ", why);
  if (rows == 0 || num_req == 0) return;  // nothing to launch
  const int rc = hpc_mla_indexer_store_k_fp8_async(ptr(k_cache), ptr(k), ip(num_seqlen_per_req), ip(q_index), ip(block_ids),
                                                   i32(rows), i32(num_req), i32(page), i32(block_ids.size(1)),
                                                   i32(k_cache.size(0)), block_stride(k_cache), k_rs, stream_of(k));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_store_k_fp8");
}

// ---- mla_indexer_logits_fp8 -------------------------------------------------------------------------------------------------------
at::Tensor logits_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                      const at::Tensor& num_seq_kvcache, int64_t mtp, bool new_kv_included, const c10::optional<at::Tensor>& output) {
  const Dims d = check_reader(q, weights, k_cache, block_ids, num_seq_kvcache, mtp);
  const int64_t cols = d.max_blocks * d.page;
  at::Tensor out = out_or_new(output, q, {d.b * d.sq, cols}, at::kFloat, "output", kOnInputDevice);
  const auto ip = [](const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); };
  const char* why = hpc_mla_indexer_logits_fp8_refusal(static_cast<const float*>(out.data_ptr()), ptr(q),
                                                       static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids),
                                                       ip(num_seq_kvcache), i32(d.b), i32(d.sq), i32(d.h), i32(d.page),
                                                       i32(d.max_blocks), i32(k_cache.size(0)), block_stride(k_cache), cols);
  TORCH_CHECK(why == nullptr, "mla_indexer_logits_fp8: ", why);
  if (d.b == 0) return out;  // nothing to launch
  const int rc = hpc_mla_indexer_logits_fp8_async(static_cast<float*>(out.data_ptr()), ptr(q),
                                                  static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids),
                                                  ip(num_seq_kvcache), i32(d.b), i32(d.sq), i32(d.h), i32(d.page), i32(d.max_blocks),
                                                  i32(k_cache.size(0)), block_stride(k_cache), cols, new_kv_included ? 1 : 0,
                                                  stream_of(q));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_logits_fp8");
  return out;
}

// ---- mla_indexer_topk -------------------------------------------------------------------------------------------------------------
at::Tensor select_topk(const at::Tensor& logits, const at::Tensor& num_seq_kvcache, int64_t topk, int64_t mtp, bool new_kv_included,
                const c10::optional<at::Tensor>& output) {
  TORCH_CHECK(logits.is_cuda(), "logits tensor must be cuda");
  TORCH_CHECK(logits.scalar_type() == at::kFloat, "logits dtype must be float32");
  TORCH_CHECK(logits.dim() == 2 && (logits.size(1) <= 1 || logits.stride(1) == 1), "logits must be [num_batch * (mtp + 1), columns] with a contiguous last dim");
  TORCH_CHECK(mtp >= 0 && mtp <= 3, "mtp must be 0 .. 3, got ", mtp);
  const int64_t sq = mtp + 1;
  check_table(num_seq_kvcache, "num_seq_kvcache", logits, 1);
  const int64_t b = num_seq_kvcache.size(0), cols = logits.size(1);
  TORCH_CHECK(logits.size(0) == b * sq, "logits must have num_batch * (mtp + 1) = ", b * sq, " rows, got ", logits.size(0));
  TORCH_CHECK(topk >= 1 && topk <= hpc::kIdxMaxTopk, "topk must be 1 .. 65536, got ", topk);
  TORCH_CHECK(b <= INT32_MAX, "sizes beyond int32");
  at::Tensor out = out_or_new(output, logits, {b * sq, topk}, at::kInt, "output", kOnInputDevice);
  const int64_t rs = logits.size(0) > 1 ? logits.stride(0) : cols;
  const char* why = hpc_mla_indexer_topk_refusal(static_cast<const int*>(out.data_ptr()), static_cast<const float*>(logits.data_ptr()),
                                                 static_cast<const int*>(num_seq_kvcache.data_ptr()), i32(b), i32(sq), cols,
                                                 i32(topk), rs);
  TORCH_CHECK(why == nullptr, "mla_indexer_topk: ", why);
  if (b == 0) return out;  // nothing to launch
  const int rc = hpc_mla_indexer_topk_async(static_cast<int*>(out.data_ptr()), static_cast<const float*>(logits.data_ptr()),
                                            static_cast<const int*>(num_seq_kvcache.data_ptr()), i32(b), i32(sq), cols, i32(topk),
                                            rs, new_kv_included ? 1 : 0, stream_of(logits));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_topk");
  return out;
}

// ---- mla_indexer_topk_fp8: the two back to back through the cached scratch, whose layout is mla_indexer_scratch()'s ---------------
at::Tensor topk_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                    const at::Tensor& num_seq_kvcache, int64_t topk, int64_t mtp, bool new_kv_included,
                    const c10::optional<at::Tensor>& output) {
  const Dims d = check_reader(q, weights, k_cache, block_ids, num_seq_kvcache, mtp);
  TORCH_CHECK(topk >= 1 && topk <= hpc::kIdxMaxTopk, "topk must be 1 .. 65536, got ", topk);
  at::Tensor out = out_or_new(output, q, {d.b * d.sq, topk}, at::kInt, "output", kOnInputDevice);
  const hpc::MlaIndexerScratch need = hpc::mla_indexer_scratch(d.b * d.sq, d.max_blocks * d.page);
  at::Tensor ws;
  if (d.b > 0) ws = cached_scratch(kScratchMlaIndexer, q, std::max<int64_t>(need.bytes, 16), 0);  // never zeroed
  const auto ip = [](const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); };
  const char* why = hpc_mla_indexer_topk_fp8_refusal(static_cast<const int*>(out.data_ptr()), ptr(q),
                                                     static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids),
                                                     ip(num_seq_kvcache), i32(d.b), i32(d.sq), i32(d.h), i32(d.page),
                                                     i32(d.max_blocks), i32(k_cache.size(0)), block_stride(k_cache), i32(topk),
                                                     d.b > 0 ? ws.data_ptr() : nullptr, d.b > 0 ? ws.numel() : 0);
  TORCH_CHECK(why == nullptr, "mla_indexer_topk_fp8: ", why);
  if (d.b == 0) return out;  // nothing to launch
  const int rc = hpc_mla_indexer_topk_fp8_async(static_cast<int*>(out.data_ptr()), ptr(q),
                                                static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids),
                                                ip(num_seq_kvcache), i32(d.b), i32(d.sq), i32(d.h), i32(d.page), i32(d.max_blocks),
                                                i32(k_cache.size(0)), block_stride(k_cache), i32(topk), new_kv_included ? 1 : 0,
                                                ws.data_ptr(), ws.numel(), stream_of(q));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_topk_fp8");
  return out;
}

// ---- the same three over a ragged prefill chunk (csrc/mla_indexer_prefill.hip), pinned to tests/mla_indexer_prefill_ref.py --------
struct ChunkDims {
  int64_t rows, req, h, page, max_blocks;
};
void check_row_rule(const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, const at::Tensor& like, int64_t row_begin) {
  check_table(num_seqlen_per_req, "num_seqlen_per_req", like, 1);
  check_table(q_index, "q_index", like, 1);
  TORCH_CHECK(q_index.size(0) == num_seqlen_per_req.size(0) + 1, "q_index must be [num_req + 1] = [", num_seqlen_per_req.size(0) + 1, "]");
  TORCH_CHECK(row_begin >= 0 && row_begin <= INT32_MAX, "row_begin must be a row of the chunk, got ", row_begin);
}
ChunkDims check_chunk_reader(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                             const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, int64_t row_begin) {
  TORCH_CHECK(q.is_cuda(), "q tensor must be cuda");
  TORCH_CHECK(q.scalar_type() == kF8, "q dtype must be float8_e4m3fn");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == hpc::kIdxDim && q.is_contiguous(), "q must be a contiguous [rows, num_head, 128]");
  const int64_t rows = q.size(0), h = q.size(1);
  check_on(weights, "weights", q, at::kFloat, "float32");
  TORCH_CHECK(weights.dim() == 2 && weights.size(0) == rows && weights.size(1) == h && weights.is_contiguous(),
              "weights must be a contiguous [rows, num_head] = [", rows, ", ", h, "]");
  check_row_rule(num_seqlen_per_req, q_index, q, row_begin);
  const int64_t req = num_seqlen_per_req.size(0);
  check_table(block_ids, "block_ids", q, 2);
  TORCH_CHECK(block_ids.size(0) == req, "block_ids must have num_req = ", req, " rows");
  const int64_t page = check_cache(k_cache, q);
  TORCH_CHECK(rows <= INT32_MAX && req < INT32_MAX && h <= INT32_MAX && block_ids.size(1) <= INT32_MAX, "sizes beyond int32");
  return {rows, req, h, page, block_ids.size(1)};
}

at::Tensor logits_prefill_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                              const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, int64_t row_begin,
                              const c10::optional<at::Tensor>& output) {
  const ChunkDims d = check_chunk_reader(q, weights, k_cache, block_ids, num_seqlen_per_req, q_index, row_begin);
  const int64_t cols = d.max_blocks * d.page;
  at::Tensor out = out_or_new(output, q, {d.rows, cols}, at::kFloat, "output", kOnInputDevice);
  const auto ip = [](const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); };
  const char* why = hpc_mla_indexer_logits_prefill_fp8_refusal(
      static_cast<const float*>(out.data_ptr()), ptr(q), static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids),
      ip(num_seqlen_per_req), ip(q_index), i32(d.rows), i32(d.req), i32(row_begin), i32(d.h), i32(d.page), i32(d.max_blocks),
      i32(k_cache.size(0)), block_stride(k_cache), cols);
  TORCH_CHECK(why == nullptr, "mla_indexer_logits_prefill_fp8: ", why);
  if (d.rows == 0 || d.req == 0) return out;  // nothing to launch
  const int rc = hpc_mla_indexer_logits_prefill_fp8_async(
      static_cast<float*>(out.data_ptr()), ptr(q), static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids),
      ip(num_seqlen_per_req), ip(q_index), i32(d.rows), i32(d.req), i32(row_begin), i32(d.h), i32(d.page), i32(d.max_blocks),
      i32(k_cache.size(0)), block_stride(k_cache), cols, stream_of(q));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_logits_prefill_fp8");
  return out;
}

at::Tensor topk_prefill(const at::Tensor& logits, const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, int64_t topk,
                        int64_t row_begin, const c10::optional<at::Tensor>& output) {
  TORCH_CHECK(logits.is_cuda(), "logits tensor must be cuda");
  TORCH_CHECK(logits.scalar_type() == at::kFloat, "logits dtype must be float32");
  TORCH_CHECK(logits.dim() == 2 && (logits.size(1) <= 1 || logits.stride(1) == 1), "logits must be [rows, columns] with a contiguous last dim");
  check_row_rule(num_seqlen_per_req, q_index, logits, row_begin);
  const int64_t rows = logits.size(0), cols = logits.size(1), req = num_seqlen_per_req.size(0);
  TORCH_CHECK(topk >= 1 && topk <= hpc::kIdxMaxTopk, "topk must be 1 .. 65536, got ", topk);
  TORCH_CHECK(rows <= INT32_MAX && req < INT32_MAX, "sizes beyond int32");
  at::Tensor out = out_or_new(output, logits, {rows, topk}, at::kInt, "output", kOnInputDevice);
  const int64_t rs = rows > 1 ? logits.stride(0) : cols;
  const auto ip = [](const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); };
  const char* why = hpc_mla_indexer_topk_prefill_refusal(ip(out), static_cast<const float*>(logits.data_ptr()), ip(num_seqlen_per_req),
                                                         ip(q_index), i32(rows), i32(req), i32(row_begin), cols, i32(topk), rs);
  TORCH_CHECK(why == nullptr, "mla_indexer_topk_prefill: ", why);
  if (rows == 0) return out;  // nothing to launch
  if (req == 0) return out.fill_(-1);  // every row is a row of no request
  const int rc = hpc_mla_indexer_topk_prefill_async(static_cast<int*>(out.data_ptr()), static_cast<const float*>(logits.data_ptr()),
                                                    ip(num_seqlen_per_req), ip(q_index), i32(rows), i32(req), i32(row_begin), cols,
                                                    i32(topk), rs, stream_of(logits));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_topk_prefill");
  return out;
}

// the two over row slabs through the cached scratch, whose layout and slab are mla_indexer_prefill_route()'s
at::Tensor topk_prefill_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                            const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, int64_t topk, int64_t scratch_rows,
                            const c10::optional<at::Tensor>& output) {
  const ChunkDims d = check_chunk_reader(q, weights, k_cache, block_ids, num_seqlen_per_req, q_index, 0);
  TORCH_CHECK(topk >= 1 && topk <= hpc::kIdxMaxTopk, "topk must be 1 .. 65536, got ", topk);
  TORCH_CHECK(scratch_rows >= 0 && scratch_rows <= INT32_MAX, "scratch_rows must be 0 (the library chooses) or a row count, got ", scratch_rows);
  at::Tensor out = out_or_new(output, q, {d.rows, topk}, at::kInt, "output", kOnInputDevice);
  const bool work = d.rows > 0 && d.req > 0;
  const hpc::MlaIndexerPrefillRoute r = hpc::mla_indexer_prefill_route(i32(d.rows), i32(d.req), i32(d.h), i32(d.page), i32(d.max_blocks),
                                                                       i32(topk), false, i32(scratch_rows), 256);
  at::Tensor ws;
  if (work && r.code == HPC_OK) ws = cached_scratch(kScratchMlaIndexerPrefill, q, std::max<int64_t>(r.scratch.bytes, 16), 0);  // never zeroed
  const auto ip = [](const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); };
  const char* why = hpc_mla_indexer_topk_prefill_fp8_refusal(
      ip(out), ptr(q), static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids), ip(num_seqlen_per_req), ip(q_index),
      i32(d.rows), i32(d.req), i32(d.h), i32(d.page), i32(d.max_blocks), i32(k_cache.size(0)), block_stride(k_cache), i32(topk),
      i32(scratch_rows), ws.defined() ? ws.data_ptr() : nullptr, ws.defined() ? ws.numel() : 0);
  TORCH_CHECK(why == nullptr, "mla_indexer_topk_prefill_fp8: ", why);
  if (d.rows == 0) return out;  // nothing to launch
  if (d.req == 0) return out.fill_(-1);  // every row is a row of no request
  const int rc = hpc_mla_indexer_topk_prefill_fp8_async(
      static_cast<int*>(out.data_ptr()), ptr(q), static_cast<const float*>(weights.data_ptr()), ptr(k_cache), ip(block_ids),
      ip(num_seqlen_per_req), ip(q_index), i32(d.rows), i32(d.req), i32(d.h), i32(d.page), i32(d.max_blocks), i32(k_cache.size(0)),
      block_stride(k_cache), i32(topk), i32(scratch_rows), ws.data_ptr(), ws.numel(), stream_of(q));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_topk_prefill_fp8");
  return out;
}

// ---- mla_indexer_prep_fp8: the front end (csrc/mla_indexer_prep.hip), pinned to tests/mla_indexer_prep_ref.py -------------------------
// Returns (q8, weights): the caller's out_q / out_weights or fresh contiguous ones; two empty tensors without q.  With the
// outputs given (or no q) nothing is allocated.  The host rule and its words are mla_indexer_prep_route's.
std::tuple<at::Tensor, at::Tensor> prep_fp8(const c10::optional<at::Tensor>& k_cache, const at::Tensor& k, const at::Tensor& k_norm_weight,
                                            const at::Tensor& k_norm_bias, const at::Tensor& cos_sin,
                                            const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, const at::Tensor& block_ids,
                                            const c10::optional<at::Tensor>& q, const c10::optional<at::Tensor>& head_weights,
                                            c10::optional<double> softmax_scale, double eps, bool interleaved, double rotate_scale,
                                            bool pow2_scale, const c10::optional<at::Tensor>& out_k,
                                            const c10::optional<at::Tensor>& out_q, const c10::optional<at::Tensor>& out_weights,
                                            const c10::optional<at::Tensor>& out_q_rot) {
  TORCH_CHECK(k.is_cuda(), "k tensor must be cuda");
  TORCH_CHECK(k.scalar_type() == at::kBFloat16, "k dtype must be bfloat16");
  TORCH_CHECK(k.dim() == 2 && k.size(1) == hpc::kIdxDim && k.stride(1) == 1, "k must be [rows, 128] with a contiguous last dim");
  const int64_t rows = k.size(0);
  for (const auto& [t, name] : {std::pair<const at::Tensor&, const char*>{k_norm_weight, "k_norm_weight"}, {k_norm_bias, "k_norm_bias"}}) {
    check_on(t, name, k, at::kFloat, "float32");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == hpc::kIdxDim && t.is_contiguous(), name, " must be a contiguous [128]");
  }
  check_on(cos_sin, "cos_sin", k, at::kFloat, "float32");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == hpc::kIdxRope && cos_sin.is_contiguous() && cos_sin.size(0) > 0,
              "cos_sin must be a contiguous [max_pos, 64] with max_pos > 0");
  check_table(num_seqlen_per_req, "num_seqlen_per_req", k, 1);
  const int64_t num_req = num_seqlen_per_req.size(0);
  check_table(q_index, "q_index", k, 1);
  TORCH_CHECK(q_index.size(0) == num_req + 1, "q_index must be [num_req + 1] = [", num_req + 1, "]");
  check_table(block_ids, "block_ids", k, 2);
  TORCH_CHECK(block_ids.size(0) == num_req, "block_ids must have num_req = ", num_req, " rows");
  TORCH_CHECK(k_cache.has_value() || out_k.has_value(), "one of k_cache and out_k must be given");
  int64_t page = 0, num_blocks = 0, bs = 0;
  if (k_cache.has_value()) {
    page = check_cache(*k_cache, k);
    num_blocks = k_cache->size(0), bs = block_stride(*k_cache);
  }
  TORCH_CHECK(rows <= INT32_MAX && num_req < INT32_MAX && block_ids.size(1) <= INT32_MAX && cos_sin.size(0) <= INT32_MAX, "sizes beyond int32");
  at::Tensor ok;
  if (out_k.has_value()) ok = out_or_new(out_k, k, {rows, hpc::kIdxDim}, at::kBFloat16, "out_k", kOnInputDevice);

  const bool with_q = q.has_value();
  TORCH_CHECK(with_q || !(head_weights.has_value() || out_q.has_value() || out_weights.has_value() || out_q_rot.has_value()),
              "head_weights, out_q, out_weights and out_q_rot need q");
  int64_t h = 0, q_rs = 0, q_hs = 0;
  at::Tensor q8 = at::empty({0}, k.options().dtype(kF8)), w = at::empty({0}, k.options().dtype(at::kFloat)), qrot;
  bool hw_bf16 = false;
  if (with_q) {
    check_on(*q, "q", k, at::kBFloat16, "bfloat16");
    TORCH_CHECK(q->dim() == 3 && q->size(0) == rows && q->size(2) == hpc::kIdxDim && q->stride(2) == 1,
                "q must be [rows, num_head, 128] with a contiguous last dim");
    h = q->size(1);
    TORCH_CHECK(h == 16 || h == 32 || h == 64, "mla_indexer_prep_fp8: the index head count must be 16, 32 or 64, got ", h);
    TORCH_CHECK(head_weights.has_value() && softmax_scale.has_value(), "q needs head_weights and softmax_scale");
    const at::Tensor& hw = *head_weights;
    TORCH_CHECK(hw.is_cuda() && hw.device() == k.device(), "head_weights must be a cuda tensor on the device of the op's first tensor");
    TORCH_CHECK(hw.scalar_type() == at::kFloat || hw.scalar_type() == at::kBFloat16, "head_weights dtype must be float32 or bfloat16");
    TORCH_CHECK(hw.dim() == 2 && hw.size(0) == rows && hw.size(1) == h && hw.is_contiguous(), "head_weights must be a contiguous [rows, num_head]");
    hw_bf16 = hw.scalar_type() == at::kBFloat16;
    q_rs = rows > 1 ? q->stride(0) : h * q->stride(1), q_hs = q->stride(1);
    q8 = out_or_new(out_q, k, {rows, h, hpc::kIdxDim}, kF8, "out_q", kOnInputDevice);
    w = out_or_new(out_weights, k, {rows, h}, at::kFloat, "out_weights", kOnInputDevice);
    if (out_q_rot.has_value()) qrot = out_or_new(out_q_rot, k, {rows, h, hpc::kIdxDim}, at::kBFloat16, "out_q_rot", kOnInputDevice);
  }
  const int64_t k_rs = rows > 1 ? k.stride(0) : hpc::kIdxDim;
  const auto ip = [](const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); };
  const auto fp = [](const at::Tensor& t) { return static_cast<const float*>(t.data_ptr()); };
  const auto vp = [](const at::Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; };
  // float32(softmax_scale * Hi ** -0.5), formed in double as the caller's Python would
  const float ss = with_q ? static_cast<float>(*softmax_scale * hpc::mla_indexer_prep_head_factor(i32(h))) : 0.f;
  const char* why = hpc_mla_indexer_prep_fp8_refusal(
      ptr(k_cache), vp(ok), with_q ? q8.data_ptr() : nullptr, with_q ? static_cast<float*>(w.data_ptr()) : nullptr, vp(qrot), ptr(k),
      ptr(q), ptr(head_weights), fp(k_norm_weight), fp(k_norm_bias), fp(cos_sin), ip(num_seqlen_per_req), ip(q_index), ip(block_ids),
      i32(rows), i32(num_req), i32(h), i32(page), i32(block_ids.size(1)), i32(num_blocks), i32(cos_sin.size(0)), bs, k_rs, q_rs, q_hs,
      hw_bf16 ? 1 : 0, ss, static_cast<float>(eps), static_cast<float>(rotate_scale));
  TORCH_CHECK(why == nullptr, "mla_indexer_prep_fp8: ", why);
  if (rows == 0 || num_req == 0) return {q8, w};  // nothing to launch
  const int rc = hpc_mla_indexer_prep_fp8_async(
      ptr(k_cache), vp(ok), with_q ? q8.data_ptr() : nullptr, with_q ? static_cast<float*>(w.data_ptr()) : nullptr, vp(qrot), ptr(k),
      ptr(q), ptr(head_weights), fp(k_norm_weight), fp(k_norm_bias), fp(cos_sin), ip(num_seqlen_per_req), ip(q_index), ip(block_ids),
      i32(rows), i32(num_req), i32(h), i32(page), i32(block_ids.size(1)), i32(num_blocks), i32(cos_sin.size(0)), bs, k_rs, q_rs, q_hs,
      hw_bf16 ? 1 : 0, ss, static_cast<float>(eps), static_cast<float>(rotate_scale), interleaved ? 1 : 0, pow2_scale ? 1 : 0,
      stream_of(k));
  HPC_LAUNCH_CHECK(rc, "mla_indexer_prep_fp8");
  return {q8, w};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(hpc_mla, m) {
  m.def("mla_indexer_store_k_fp8(Tensor k_cache, Tensor k, Tensor num_seqlen_per_req, Tensor q_index, Tensor block_ids) -> ()");
  m.def(
      "mla_indexer_logits_fp8(Tensor q, Tensor weights, Tensor k_cache, Tensor block_ids, Tensor num_seq_kvcache, int mtp, "
      "bool new_kv_included, Tensor? output) -> Tensor");
  m.def("mla_indexer_topk(Tensor logits, Tensor num_seq_kvcache, int topk, int mtp, bool new_kv_included, Tensor? output) -> Tensor");
  m.def(
      "mla_indexer_topk_fp8(Tensor q, Tensor weights, Tensor k_cache, Tensor block_ids, Tensor num_seq_kvcache, int topk, int mtp, "
      "bool new_kv_included, Tensor? output) -> Tensor");
  m.def(
      "mla_indexer_prep_fp8(Tensor? k_cache, Tensor k, Tensor k_norm_weight, Tensor k_norm_bias, Tensor cos_sin, "
      "Tensor num_seqlen_per_req, Tensor q_index, Tensor block_ids, Tensor? q, Tensor? head_weights, float? softmax_scale, float eps, "
      "bool interleaved, float rotate_scale, bool pow2_scale, Tensor? out_k, Tensor? out_q, Tensor? out_weights, Tensor? out_q_rot) "
      "-> (Tensor, Tensor)");
  m.def(
      "mla_indexer_logits_prefill_fp8(Tensor q, Tensor weights, Tensor k_cache, Tensor block_ids, Tensor num_seqlen_per_req, "
      "Tensor q_index, int row_begin, Tensor? output) -> Tensor");
  m.def(
      "mla_indexer_topk_prefill(Tensor logits, Tensor num_seqlen_per_req, Tensor q_index, int topk, int row_begin, Tensor? output) "
      "-> Tensor");
  m.def(
      "mla_indexer_topk_prefill_fp8(Tensor q, Tensor weights, Tensor k_cache, Tensor block_ids, Tensor num_seqlen_per_req, "
      "Tensor q_index, int topk, int scratch_rows, Tensor? output) -> Tensor");
  m.def("_mla_indexer_prefill_workspaces() -> Tensor[]", []() { return list_cached_scratch(kScratchMlaIndexerPrefill); });
  // the cached logits scratch of the fused op (tests fill it with NaN bytes: no column that was not written may be read)
  m.def("_mla_indexer_workspaces() -> Tensor[]", []() { return list_cached_scratch(kScratchMlaIndexer); });
}

TORCH_LIBRARY_IMPL(hpc_mla, CUDA, m) {
  m.impl("mla_indexer_store_k_fp8", &store_k_fp8);
  m.impl("mla_indexer_logits_fp8", &logits_fp8);
  m.impl("mla_indexer_topk", &select_topk);
  m.impl("mla_indexer_topk_fp8", &topk_fp8);
  m.impl("mla_indexer_prep_fp8", &prep_fp8);
  m.impl("mla_indexer_logits_prefill_fp8", &logits_prefill_fp8);
  m.impl("mla_indexer_topk_prefill", &topk_prefill);
  m.impl("mla_indexer_topk_prefill_fp8", &topk_prefill_fp8);
}
