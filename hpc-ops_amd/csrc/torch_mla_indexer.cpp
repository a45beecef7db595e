// C++ host side of the DSA lightning indexer, under torch.ops.hpc_mla.* beside the MLA ops it serves.  Ours only; pinned to the
// PyTorch statements tests/mla_indexer_ref.py, tests/mla_indexer_prefill_ref.py and tests/mla_indexer_prep_ref.py.
//   the writer     mla_indexer_store_k_fp8 (csrc/mla_indexer.hip) and the front end mla_indexer_prep_fp8 (csrc/mla_indexer_prep.hip);
//   the readers    logits, top-k and the fused top-k, each ONE body (logits_body, topk_body, fused_body) for a decode step
//                  (mla_indexer_logits_fp8, mla_indexer_topk, mla_indexer_topk_fp8; csrc/mla_indexer.hip) and for a ragged prefill
//                  chunk (mla_indexer_logits_prefill_fp8, mla_indexer_topk_prefill, mla_indexer_topk_prefill_fp8 over row slabs;
//                  csrc/mla_indexer_prefill.hip).  Where the rows of a call come from - its tensor checks, message words and C
//                  arguments - is `Rows`; the eight registered functions only build one from their schema's arguments.
// dtype, device and shape are checked here; the cache's rule, the limits, strides and alignment are the launchers'
// (csrc/mla_indexer_route.h) and come back in their words through hpc_mla_indexer_*_refusal: checked_launch (torch_common.h)
// hands one argument list to the refusal and to the launcher.  Nothing here reads the values of a length, a page table or a
// logit; with `output` given nothing is allocated per call beyond the cached scratch of the fused ops and the calls capture into
// a hipGraph.  No kernels here.
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

const int* ip(const at::Tensor& t) { return static_cast<const int*>(t.data_ptr()); }
const float* fp(const at::Tensor& t) { return static_cast<const float*>(t.data_ptr()); }
const void* cp(const at::Tensor& t) { return t.data_ptr(); }

// The rows of a reader's call as the shim sees them (the launchers' MlaRows, csrc/mla_indexer_route.h): a decode step
// (num_seq_kvcache, mtp, new_kv_included) or a ragged prefill chunk (num_seqlen_per_req, q_index, row_begin), with the tensor
// checks, the message words and the C arguments of its form
struct Rows {
  const at::Tensor& lens;
  const at::Tensor* q_index;  // null: a decode step
  int64_t mtp, row_begin;
  bool new_kv_included;

  bool ragged() const { return q_index != nullptr; }
  int64_t units() const { return lens.size(0); }  // requests: the rows of block_ids
  const char* rows_word() const { return ragged() ? "rows" : "num_batch * (mtp + 1)"; }
  const char* units_word() const { return ragged() ? "num_req" : "num_batch"; }
  bool work(int64_t rows) const { return units() > 0 && (!ragged() || rows > 0); }
  // the tables, on `like`'s device, and the `rows` that `what` (q or logits) has
  void check(const at::Tensor& like, const char* what, int64_t rows) const {
    if (ragged()) {
      check_table(lens, "num_seqlen_per_req", like, 1);
      check_table(*q_index, "q_index", like, 1);
      TORCH_CHECK(q_index->size(0) == units() + 1, "q_index must be [num_req + 1] = [", units() + 1, "]");
      TORCH_CHECK(row_begin >= 0 && row_begin <= INT32_MAX, "row_begin must be a row of the chunk, got ", row_begin);
      TORCH_CHECK(rows <= INT32_MAX && units() < INT32_MAX, "sizes beyond int32");
    } else {
      TORCH_CHECK(mtp >= 0 && mtp <= 3, "mtp must be 0 .. 3, got ", mtp);
      check_table(lens, "num_seq_kvcache", like, 1);
      TORCH_CHECK(rows == units() * (mtp + 1), what, " must have num_batch * (mtp + 1) = ", units() * (mtp + 1), " rows, got ", rows);
      TORCH_CHECK(units() <= INT32_MAX, "sizes beyond int32");
    }
  }
  // where the C entries of the two forms take their rows from (a chunk's row_begin follows where an entry has one)
  auto step_args() const { return std::make_tuple(ip(lens), i32(units()), i32(mtp + 1)); }
  auto chunk_args(int64_t rows) const { return std::make_tuple(ip(lens), ip(*q_index), i32(rows), i32(units())); }
};

struct Dims {
  int64_t rows, h, page, max_blocks;
};
// q, weights, k_cache, block_ids and the rows of the ops that read the cache
Dims check_reader(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                  const Rows& rows) {
  TORCH_CHECK(q.is_cuda(), "q tensor must be cuda");
  TORCH_CHECK(q.scalar_type() == kF8, "q dtype must be float8_e4m3fn");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == hpc::kIdxDim && q.is_contiguous(), "q must be a contiguous [", rows.rows_word(),
              ", num_head, 128]");
  const int64_t n = q.size(0), h = q.size(1);
  check_on(weights, "weights", q, at::kFloat, "float32");
  TORCH_CHECK(weights.dim() == 2 && weights.size(0) == n && weights.size(1) == h && weights.is_contiguous(),
              "weights must be a contiguous [", rows.rows_word(), ", num_head] = [", n, ", ", h, "]");
  rows.check(q, "q", n);
  check_table(block_ids, "block_ids", q, 2);
  TORCH_CHECK(block_ids.size(0) == rows.units(), "block_ids must have ", rows.units_word(), " = ", rows.units(), " rows");
  const int64_t page = check_cache(k_cache, q);
  TORCH_CHECK(h <= INT32_MAX && block_ids.size(1) <= INT32_MAX, "sizes beyond int32");
  return {n, h, page, block_ids.size(1)};
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
  checked_launch("mla_indexer_store_k_fp8", hpc_mla_indexer_store_k_fp8_refusal, hpc_mla_indexer_store_k_fp8_async,
                 rows > 0 && num_req > 0,
                 std::make_tuple(ptr(k_cache), cp(k), ip(num_seqlen_per_req), ip(q_index), ip(block_ids), i32(rows), i32(num_req),
                                 i32(page), i32(block_ids.size(1)), i32(k_cache.size(0)), block_stride(k_cache), k_rs),
                 std::make_tuple(stream_of(k)));
}

// ---- the three readers, one body each for a decode step (mla_indexer_logits_fp8, mla_indexer_topk, mla_indexer_topk_fp8;
// csrc/mla_indexer.hip, pinned to tests/mla_indexer_ref.py) and a ragged prefill chunk (the _prefill ops;
// csrc/mla_indexer_prefill.hip, pinned to tests/mla_indexer_prefill_ref.py) -----------------------------------------------------------
at::Tensor logits_body(const char* op, const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache,
                       const at::Tensor& block_ids, const Rows& rows, const c10::optional<at::Tensor>& output) {
  const Dims d = check_reader(q, weights, k_cache, block_ids, rows);
  const int64_t cols = d.max_blocks * d.page;
  at::Tensor out = out_or_new(output, q, {d.rows, cols}, at::kFloat, "output", kOnInputDevice);
  const auto head = std::make_tuple(static_cast<float*>(out.data_ptr()), cp(q), fp(weights), cp(k_cache), ip(block_ids));
  const auto tail = std::make_tuple(i32(d.h), i32(d.page), i32(d.max_blocks), i32(k_cache.size(0)), block_stride(k_cache), cols);
  if (rows.ragged())
    checked_launch(op, hpc_mla_indexer_logits_prefill_fp8_refusal, hpc_mla_indexer_logits_prefill_fp8_async, rows.work(d.rows),
                   std::tuple_cat(head, rows.chunk_args(d.rows), std::make_tuple(i32(rows.row_begin)), tail),
                   std::make_tuple(stream_of(q)));
  else
    checked_launch(op, hpc_mla_indexer_logits_fp8_refusal, hpc_mla_indexer_logits_fp8_async, rows.work(d.rows),
                   std::tuple_cat(head, rows.step_args(), tail), std::make_tuple(rows.new_kv_included ? 1 : 0, stream_of(q)));
  return out;
}

at::Tensor topk_body(const char* op, const at::Tensor& logits, const Rows& rows, int64_t topk, const c10::optional<at::Tensor>& output) {
  TORCH_CHECK(logits.is_cuda(), "logits tensor must be cuda");
  TORCH_CHECK(logits.scalar_type() == at::kFloat, "logits dtype must be float32");
  TORCH_CHECK(logits.dim() == 2 && (logits.size(1) <= 1 || logits.stride(1) == 1), "logits must be [", rows.rows_word(),
              ", columns] with a contiguous last dim");
  const int64_t n = logits.size(0), cols = logits.size(1);
  rows.check(logits, "logits", n);
  TORCH_CHECK(topk >= 1 && topk <= hpc::kIdxMaxTopk, "topk must be 1 .. 65536, got ", topk);
  at::Tensor out = out_or_new(output, logits, {n, topk}, at::kInt, "output", kOnInputDevice);
  const auto head = std::make_tuple(static_cast<int*>(out.data_ptr()), fp(logits));
  const auto tail = std::make_tuple(cols, i32(topk), n > 1 ? logits.stride(0) : cols);
  if (rows.ragged())
    checked_launch(op, hpc_mla_indexer_topk_prefill_refusal, hpc_mla_indexer_topk_prefill_async, rows.work(n),
                   std::tuple_cat(head, rows.chunk_args(n), std::make_tuple(i32(rows.row_begin)), tail),
                   std::make_tuple(stream_of(logits)));
  else
    checked_launch(op, hpc_mla_indexer_topk_refusal, hpc_mla_indexer_topk_async, rows.work(n),
                   std::tuple_cat(head, rows.step_args(), tail), std::make_tuple(rows.new_kv_included ? 1 : 0, stream_of(logits)));
  if (rows.ragged() && n > 0 && rows.units() == 0) out.fill_(-1);  // every row is a row of no request
  return out;
}

// the two back to back through the cached scratch: a step's in one piece, laid out by mla_indexer_scratch(); a chunk's over row
// slabs, slab and layout being mla_indexer_prefill_route()'s (scratch_rows is a chunk's alone)
at::Tensor fused_body(const char* op, const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache,
                      const at::Tensor& block_ids, const Rows& rows, int64_t topk, int64_t scratch_rows,
                      const c10::optional<at::Tensor>& output) {
  const Dims d = check_reader(q, weights, k_cache, block_ids, rows);
  TORCH_CHECK(topk >= 1 && topk <= hpc::kIdxMaxTopk, "topk must be 1 .. 65536, got ", topk);
  TORCH_CHECK(scratch_rows >= 0 && scratch_rows <= INT32_MAX, "scratch_rows must be 0 (the library chooses) or a row count, got ", scratch_rows);
  at::Tensor out = out_or_new(output, q, {d.rows, topk}, at::kInt, "output", kOnInputDevice);
  const bool work = rows.work(d.rows);
  int64_t need = hpc::mla_indexer_scratch(d.rows, d.max_blocks * d.page).bytes;
  if (rows.ragged()) {
    const hpc::MlaIndexerPrefillRoute r = hpc::mla_indexer_prefill_route(i32(d.rows), i32(rows.units()), i32(d.h), i32(d.page),
                                                                         i32(d.max_blocks), i32(topk), false, i32(scratch_rows), 256);
    need = r.code == HPC_OK ? r.scratch.bytes : -1;  // a refused call gets no scratch; the refusal below says why
  }
  at::Tensor ws;
  if (work && need >= 0)
    ws = cached_scratch(rows.ragged() ? kScratchMlaIndexerPrefill : kScratchMlaIndexer, q, std::max<int64_t>(need, 16), 0);  // never zeroed
  void* ws_ptr = ws.defined() ? ws.data_ptr() : nullptr;
  const int64_t ws_bytes = ws.defined() ? ws.numel() : 0;
  int* op_out = static_cast<int*>(out.data_ptr());
  const auto head = std::make_tuple(op_out, cp(q), fp(weights), cp(k_cache), ip(block_ids));
  const auto shape = std::make_tuple(i32(d.h), i32(d.page), i32(d.max_blocks), i32(k_cache.size(0)), block_stride(k_cache), i32(topk));
  if (rows.ragged()) {
    checked_launch(op, hpc_mla_indexer_topk_prefill_fp8_refusal, hpc_mla_indexer_topk_prefill_fp8_async, work,
                   std::tuple_cat(head, rows.chunk_args(d.rows), shape, std::make_tuple(i32(scratch_rows), ws_ptr, ws_bytes)),
                   std::make_tuple(stream_of(q)));
    if (d.rows > 0 && rows.units() == 0) out.fill_(-1);  // every row is a row of no request
    return out;
  }
  // a step's launcher takes new_kv_included in the middle of its list: written out
  const char* why =
      std::apply(hpc_mla_indexer_topk_fp8_refusal, std::tuple_cat(head, rows.step_args(), shape, std::make_tuple(ws_ptr, ws_bytes)));
  TORCH_CHECK(why == nullptr, op, ": ", why);
  if (!work) return out;  // nothing to launch
  const int rc = hpc_mla_indexer_topk_fp8_async(op_out, cp(q), fp(weights), cp(k_cache), ip(block_ids), ip(rows.lens), i32(rows.units()),
                                                i32(rows.mtp + 1), i32(d.h), i32(d.page), i32(d.max_blocks), i32(k_cache.size(0)),
                                                block_stride(k_cache), i32(topk), rows.new_kv_included ? 1 : 0, ws_ptr, ws_bytes,
                                                stream_of(q));
  HPC_LAUNCH_CHECK(rc, op);
  return out;
}

// the eight registered functions: the schema's arguments as the rows of a step or of a chunk
at::Tensor logits_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                      const at::Tensor& num_seq_kvcache, int64_t mtp, bool new_kv_included, const c10::optional<at::Tensor>& output) {
  return logits_body("mla_indexer_logits_fp8", q, weights, k_cache, block_ids, {num_seq_kvcache, nullptr, mtp, 0, new_kv_included}, output);
}
at::Tensor select_topk(const at::Tensor& logits, const at::Tensor& num_seq_kvcache, int64_t topk, int64_t mtp, bool new_kv_included,
                       const c10::optional<at::Tensor>& output) {
  return topk_body("mla_indexer_topk", logits, {num_seq_kvcache, nullptr, mtp, 0, new_kv_included}, topk, output);
}
at::Tensor topk_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                    const at::Tensor& num_seq_kvcache, int64_t topk, int64_t mtp, bool new_kv_included,
                    const c10::optional<at::Tensor>& output) {
  return fused_body("mla_indexer_topk_fp8", q, weights, k_cache, block_ids, {num_seq_kvcache, nullptr, mtp, 0, new_kv_included}, topk, 0,
                    output);
}
at::Tensor logits_prefill_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                              const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, int64_t row_begin,
                              const c10::optional<at::Tensor>& output) {
  return logits_body("mla_indexer_logits_prefill_fp8", q, weights, k_cache, block_ids, {num_seqlen_per_req, &q_index, 0, row_begin, true},
                     output);
}
at::Tensor topk_prefill(const at::Tensor& logits, const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, int64_t topk,
                        int64_t row_begin, const c10::optional<at::Tensor>& output) {
  return topk_body("mla_indexer_topk_prefill", logits, {num_seqlen_per_req, &q_index, 0, row_begin, true}, topk, output);
}
at::Tensor topk_prefill_fp8(const at::Tensor& q, const at::Tensor& weights, const at::Tensor& k_cache, const at::Tensor& block_ids,
                            const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index, int64_t topk, int64_t scratch_rows,
                            const c10::optional<at::Tensor>& output) {
  return fused_body("mla_indexer_topk_prefill_fp8", q, weights, k_cache, block_ids, {num_seqlen_per_req, &q_index, 0, 0, true}, topk,
                    scratch_rows, output);
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
  const auto vp = [](const at::Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; };
  // float32(softmax_scale * Hi ** -0.5), formed in double as the caller's Python would
  const float ss = with_q ? static_cast<float>(*softmax_scale * hpc::mla_indexer_prep_head_factor(i32(h))) : 0.f;
  checked_launch(
      "mla_indexer_prep_fp8", hpc_mla_indexer_prep_fp8_refusal, hpc_mla_indexer_prep_fp8_async, rows > 0 && num_req > 0,
      std::make_tuple(ptr(k_cache), vp(ok), with_q ? q8.data_ptr() : nullptr, with_q ? static_cast<float*>(w.data_ptr()) : nullptr,
                      vp(qrot), cp(k), ptr(q), ptr(head_weights), fp(k_norm_weight), fp(k_norm_bias), fp(cos_sin), ip(num_seqlen_per_req), ip(q_index), ip(block_ids), i32(rows), i32(num_req), i32(h),
                      i32(page), i32(block_ids.size(1)), i32(num_blocks), i32(cos_sin.size(0)), bs, k_rs, q_rs, q_hs, hw_bf16 ? 1 : 0, ss,
                      static_cast<float>(eps), static_cast<float>(rotate_scale)),
      std::make_tuple(interleaved ? 1 : 0, pow2_scale ? 1 : 0, stream_of(k)));
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
