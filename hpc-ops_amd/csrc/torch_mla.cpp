// C++ host side of the MLA ops over the paged latent KV cache, under their own namespace torch.ops.hpc_mla.* (hpc:: holds the
// reference's surface).  Ours only (no reference op; pinned to PyTorch statements under tests/).  Where each rule lives:
//   the cache      check_cache prints csrc/mla_cache.h's one host rule for a valid cache (row width, stride unit, alignment).  Every
//                  op over a cache is a template on kFp8, registered once per kind (bf16 elements; FP8: csrc/mla_fp8_format.h's
//                  656-byte rows in a uint8 tensor, strides in bytes): the kind and its dtype are the only difference.
//   the attention  decode_mla<kFp8> is the one body of attention_decode_mla_{bf16,fp8} (csrc/attention_decode_mla.hip, pinned to
//                  tests/mla_ref.py), of attention_decode_mla_sparse_{bf16,fp8} (the kernel's kSparse form: a list of token
//                  positions per q row, `indices` null or given) and of attention_prefill_mla_sparse_{bf16,fp8} (that form over
//                  a ragged prefill chunk: MlaRowsOf says whether the rows are a decode step's or a chunk's, the writers' row
//                  rule instead of mtp).  The registered functions only build the rows from their schema's arguments.  Route,
//                  split count and scratch size are the plan entries'; nothing here reads the values of a length or a list.
//   the writer     rope_norm_store_kv{,_fp8} (csrc/mla_store.hip), which writes that cache and the RoPE columns of q.
//   the prompt     attention_prefill_mla_bf16 (csrc/attention_prefill_mla.hip, the non-absorbed 192 / 128 form with an lse
//                  output), merge_attn_states (csrc/merge_attn_states.hip) and, between the cache and the kv_b projection of a
//                  context pass, gather_ckv{,_fp8} (csrc/mla_gather.hip).
//   the absorbs    absorb_q and unabsorb_o (csrc/mla_absorb.hip) either side of the decode attention: their route's refusal in
//                  words and the launch take one argument list (checked_launch, torch_common.h).
// With `output` (and `output_lse` where an lse is wanted) given nothing is allocated per call beyond the cached scratch and the
// calls capture into a hipGraph.  No kernels here.
#include <limits>

#include "byte_span.h"
#include "mla_cache.h"
#include "torch_common.h"

using namespace hpc_torch;

namespace {

// the nope / v head of the prompt side and the absorb matmuls (kMlaPrefillDimNope, kMlaAbsorbNope of their routes); the latent
// row's 512 / 64 / 576 are csrc/mla_cache.h's
constexpr int64_t kNope = 128;

const char* dtype_name(at::ScalarType dtype) {
  switch (dtype) {
    case at::kBFloat16: return "bfloat16";
    case at::kFloat: return "float32";
    case at::kInt: return "int32";
    case at::kByte: return "uint8";
    default: return c10::toString(dtype);
  }
}

// the cache's kind (csrc/mla_cache.h) and the one thing only torch knows of it, the dtype.  The ops over a cache are templates
// on kFp8: one body each, registered once per kind.
struct CacheKind : hpc::MlaCacheKind {
  at::ScalarType dtype;
};
template <bool kFp8>
constexpr CacheKind kCache = kFp8 ? CacheKind{hpc::kMlaCacheFp8, at::kByte} : CacheKind{hpc::kMlaCacheBf16, at::kBFloat16};

// [num_blocks, block_size, row] of the kind's dtype with a contiguous last dim here; the page size, the strides and the
// alignment are mla_cache_check's, the rule of the launchers, in its words
void check_cache(const at::Tensor& c, const CacheKind& kind) {
  TORCH_CHECK(c.scalar_type() == kind.dtype, "ckv_cache dtype must be ", dtype_name(kind.dtype));
  TORCH_CHECK(c.dim() == 3 && c.size(2) == kind.row, "ckv_cache must be [num_blocks, block_size, ", kind.row, "]");
  TORCH_CHECK(c.stride(2) == 1, "ckv_cache must have a contiguous last dim");
  const int64_t page = c.size(1), bs = c.stride(0), ts = c.stride(1);
  const hpc::MlaCacheCheck r = hpc::mla_cache_check(kind, reinterpret_cast<uintptr_t>(c.data_ptr()), page, bs, ts);
  TORCH_CHECK(r.code == HPC_OK, r.why, "; got block_size ", page, ", token stride ", ts, " and block stride ", bs);
}

// A data tensor: on `like`'s device, of `dtype` and `shape` (an entry of -1: any size), its last dim contiguous.  rows16 adds
// what the cache's writer and gather ask of their bf16 rows (kv_a, out_ckv, the gather's output [rows, 576]; q_pe, out_q_pe
// [rows, H, 64]): every other stride a multiple of 8 elements and wide enough that rows (and heads) do not overlap, base 16-byte
// aligned.  The other ops leave strides and alignment to their route (csrc/attention_prefill_mla_route.h,
// csrc/mla_absorb_route.h), whose refusal comes back in its words.
constexpr bool kRows16 = true;
bool fits(const at::Tensor& t, at::IntArrayRef shape) {
  bool ok = t.dim() == static_cast<int64_t>(shape.size());
  for (int64_t d = 0; ok && d < t.dim(); ++d) ok = shape[d] < 0 || t.size(d) == shape[d];
  return ok;
}
void check_data(const at::Tensor& t, const char* name, const at::Tensor& like, at::ScalarType dtype, at::IntArrayRef shape,
                bool rows16 = false) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name, " must be a cuda tensor on the device of the op's first tensor");
  TORCH_CHECK(t.scalar_type() == dtype, name, " dtype must be ", dtype_name(dtype));
  TORCH_CHECK(fits(t, shape), name, " must have shape ", shape, " (-1: any size), got ", t.sizes());
  TORCH_CHECK(t.stride(-1) == 1, name, " must have a contiguous last dim");
  if (!rows16) return;
  const int64_t width = shape.back();
  for (int64_t d = 0; d + 1 < t.dim(); ++d)
    TORCH_CHECK(t.stride(d) % 8 == 0 && (t.stride(d) >= width || t.size(d) <= 1), name, " stride ", d,
                " must be a multiple of 8 elements and at least ", width, ", got ", t.stride(d));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

// An index or table tensor: on `like`'s device, of `dtype` and `shape` (an entry of -1: any size), contiguous
void check_table(const at::Tensor& t, const char* name, const at::Tensor& like, at::ScalarType dtype, at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name, " must be a cuda tensor on the device of the op's first tensor");
  TORCH_CHECK(t.scalar_type() == dtype, name, " dtype must be ", dtype_name(dtype));
  TORCH_CHECK(fits(t, shape) && t.is_contiguous(), name, " must be a contiguous tensor of shape ", shape, " (-1: any size), got ",
              t.sizes());
}

// ---- attention_decode_mla_{bf16,fp8}, attention_decode_mla_sparse_{bf16,fp8} and attention_prefill_mla_sparse_{bf16,fp8}: one
// body.  `indices` null for the dense ops; sparse: each q row attends to the tokens its list names (tests/mla_sparse_ref.py), the
// list's checks stand beside the dense ones.  The rows are a decode step's (num_seq_kvcache, mtp, new_kv_included) or, the
// prefill ops, a ragged chunk's (num_seqlen_per_req, q_index: the writers' row rule as the source of a row's request and of what
// it sees, tests/mla_indexer_prefill_ref.py), routed as num_rows requests of one q row.  Nothing here reads the values of the
// lengths, q_index, block_ids or indices.  With `output` (and `output_lse` where an lse is wanted) given nothing is allocated per
// call beyond the cached scratch.
struct MlaRowsOf {
  const at::Tensor& lens;     // num_seq_kvcache, or a chunk's num_seqlen_per_req
  const at::Tensor* q_index;  // a chunk's; null: a decode step
  int64_t mtp;
  bool new_kv_included;
};
template <bool kFp8>
std::tuple<at::Tensor, at::Tensor> decode_mla(const at::Tensor& q, const at::Tensor& ckv_cache, const at::Tensor& block_ids,
                                              const MlaRowsOf& rows, const at::Tensor* indices, double softmax_scale,
                                              const c10::optional<at::Tensor>& output, const c10::optional<at::Tensor>& output_lse,
                                              bool return_lse, int64_t splits) {
  const bool sparse = indices != nullptr, ragged = rows.q_index != nullptr;
  const char* op = ragged   ? (kFp8 ? "attention_prefill_mla_sparse_fp8" : "attention_prefill_mla_sparse_bf16")
                   : sparse ? (kFp8 ? "attention_decode_mla_sparse_fp8" : "attention_decode_mla_sparse_bf16")
                            : (kFp8 ? "attention_decode_mla_fp8" : "attention_decode_mla_bf16");
  const char* rows_word = ragged ? "rows" : "num_batch * (mtp + 1)";
  cuda_contig(q, "q");
  TORCH_CHECK(q.scalar_type() == at::kBFloat16, "q dtype must be bfloat16");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == hpc::kMlaRow, "q must be [", rows_word, ", num_head, 576]");
  const int64_t t = q.size(0), h = q.size(1);
  TORCH_CHECK(ckv_cache.is_cuda() && ckv_cache.device() == q.device(), "ckv_cache must be a cuda tensor on q's device");
  check_table(rows.lens, ragged ? "num_seqlen_per_req" : "num_seq_kvcache", q, at::kInt, {-1});
  const int64_t units = rows.lens.size(0);  // requests: the rows of block_ids
  if (ragged) {
    check_table(*rows.q_index, "q_index", q, at::kInt, {units + 1});
  } else {
    TORCH_CHECK(rows.mtp >= 0 && rows.mtp <= 3, "mtp must be 0 .. 3, got ", rows.mtp);
    TORCH_CHECK(t == units * (rows.mtp + 1), "q must have num_batch * (mtp + 1) = ", units * (rows.mtp + 1), " rows, got ", t);
  }
  check_table(block_ids, "block_ids", q, at::kInt, {units, -1});
  TORCH_CHECK(h % 16 == 0 && h >= 16 && h <= 128, "num_head must be a multiple of 16, 16 .. 128, got ", h);
  int64_t topk = 0;
  if (sparse) {
    check_table(*indices, "indices", q, at::kInt, {t, -1});
    topk = indices->size(1);
    TORCH_CHECK(topk >= 1 && topk <= 65536, "indices must be [", rows_word, ", topk] with 1 <= topk <= 65536, got topk = ", topk);
  }
  check_cache(ckv_cache, kCache<kFp8>);
  const int64_t page = ckv_cache.size(1);
  TORCH_CHECK(block_ids.size(1) * page <= (int64_t{1} << 30), "block_ids reaches beyond 2^30 tokens");
  TORCH_CHECK((!sparse || ckv_cache.size(0) <= INT32_MAX) && (!ragged || (t <= INT32_MAX && units < INT32_MAX)), "sizes beyond int32");
  TORCH_CHECK(splits >= 0, "splits must be 0 (the library chooses) or a count, got ", splits);
  at::Tensor out = out_or_new(output, q, {t, h, hpc::kMlaLatent}, at::kBFloat16, "output", kOnInputDevice);
  const bool want_lse = return_lse || output_lse.has_value();
  at::Tensor lse = want_lse ? out_or_new(output_lse, q, {t, h}, at::kFloat, "output_lse", kOnInputDevice)
                            : at::empty({0}, q.options().dtype(at::kFloat));

  // the route's units: the requests of a step, the rows of a chunk
  const int64_t b = ragged ? t : units, sq = ragged ? 1 : rows.mtp + 1;
  int s = 0, max_splits = 0;
  int64_t ws_bytes = 0;
  const int wanted = i32(std::min<int64_t>(splits, INT32_MAX)), cus = b > 0 ? hpc_get_cu_count(q.device().index()) : 256;
  const int rc_plan =
      sparse ? hpc_attention_decode_mla_sparse_plan(i32(b), i32(sq), i32(h), i32(topk), wanted, cus, &s, &max_splits, &ws_bytes,
                                                    nullptr, nullptr)
             : hpc_attention_decode_mla_plan(i32(b), i32(sq), i32(h), wanted, cus, &s, &max_splits, &ws_bytes);
  TORCH_CHECK(splits <= max_splits, "splits = ", splits, " is beyond the ", max_splits, " pieces a ", sparse ? "list" : "request",
              " may be cut into");
  HPC_LAUNCH_CHECK(rc_plan, op);
  if (b == 0) return {out, lse};
  if (ragged && units == 0) {  // every row is a row of no request: the empty row
    out.zero_();
    if (want_lse) lse.fill_(-std::numeric_limits<float>::infinity());
    return {out, lse};
  }
  TORCH_CHECK(block_ids.size(1) > 0, "block_ids has no columns");
  at::Tensor ws;
  if (s > 1) ws = cached_scratch(kScratchMla, q, ws_bytes, 0);  // never zeroed: an unwritten piece is never read
  const auto ip = [](const at::Tensor& x) { return static_cast<const int*>(x.data_ptr()); };
  float* lse_ptr = want_lse ? static_cast<float*>(lse.data_ptr()) : nullptr;
  void* ws_ptr = s > 1 ? ws.data_ptr() : nullptr;
  const float scale = static_cast<float>(softmax_scale);
  const int nki = rows.new_kv_included ? 1 : 0, cols = i32(block_ids.size(1)), num_blocks = i32(ckv_cache.size(0));
  const int64_t bs = ckv_cache.stride(0), ts = ckv_cache.stride(1);
  // sparse: the launcher is given the effective count - cutting the list into that many pieces gives the same piece length again
  const int rc =
      ragged   ? (kFp8 ? hpc_attention_prefill_mla_sparse_fp8_async : hpc_attention_prefill_mla_sparse_bf16_async)(
                     ptr(out), lse_ptr, ptr(q), ptr(ckv_cache), ip(block_ids), ip(rows.lens), ip(*rows.q_index), ip(*indices), i32(t),
                     i32(units), i32(h), i32(topk), i32(page), cols, num_blocks, bs, ts, scale, s, ws_ptr, ws_bytes, stream_of(q))
      : sparse ? (kFp8 ? hpc_attention_decode_mla_sparse_fp8_async : hpc_attention_decode_mla_sparse_bf16_async)(
                     ptr(out), lse_ptr, ptr(q), ptr(ckv_cache), ip(block_ids), ip(rows.lens), ip(*indices), i32(b), i32(sq), i32(h),
                     i32(topk), i32(page), cols, num_blocks, bs, ts, scale, nki, s, ws_ptr, ws_bytes, stream_of(q))
               : (kFp8 ? hpc_attention_decode_mla_fp8_async : hpc_attention_decode_mla_bf16_async)(
                     ptr(out), lse_ptr, ptr(q), ptr(ckv_cache), ip(block_ids), ip(rows.lens), i32(b), i32(sq), i32(h), i32(page), cols,
                     bs, ts, scale, nki, s, ws_ptr, ws_bytes, stream_of(q));
  HPC_LAUNCH_CHECK(rc, op);
  return {out, lse};
}

template <bool kFp8>
std::tuple<at::Tensor, at::Tensor> attention_decode_mla(const at::Tensor& q, const at::Tensor& ckv_cache, const at::Tensor& block_ids,
                                                        const at::Tensor& num_seq_kvcache, double softmax_scale, int64_t mtp,
                                                        bool new_kv_included, const c10::optional<at::Tensor>& output,
                                                        const c10::optional<at::Tensor>& output_lse, bool return_lse, int64_t splits) {
  return decode_mla<kFp8>(q, ckv_cache, block_ids, {num_seq_kvcache, nullptr, mtp, new_kv_included}, nullptr, softmax_scale, output,
                          output_lse, return_lse, splits);
}

template <bool kFp8>
std::tuple<at::Tensor, at::Tensor> attention_decode_mla_sparse(const at::Tensor& q, const at::Tensor& ckv_cache,
                                                               const at::Tensor& block_ids, const at::Tensor& num_seq_kvcache,
                                                               const at::Tensor& indices, double softmax_scale, int64_t mtp,
                                                               bool new_kv_included, const c10::optional<at::Tensor>& output,
                                                               const c10::optional<at::Tensor>& output_lse, bool return_lse,
                                                               int64_t splits) {
  return decode_mla<kFp8>(q, ckv_cache, block_ids, {num_seq_kvcache, nullptr, mtp, new_kv_included}, &indices, softmax_scale, output,
                          output_lse, return_lse, splits);
}

// the token-sparse attention over a ragged prefill chunk: the decode op's body, kernel, route and scratch with a chunk's rows
template <bool kFp8>
std::tuple<at::Tensor, at::Tensor> attention_prefill_mla_sparse(const at::Tensor& q, const at::Tensor& ckv_cache,
                                                                const at::Tensor& block_ids, const at::Tensor& num_seqlen_per_req,
                                                                const at::Tensor& q_index, const at::Tensor& indices,
                                                                double softmax_scale, const c10::optional<at::Tensor>& output,
                                                                const c10::optional<at::Tensor>& output_lse, bool return_lse,
                                                                int64_t splits) {
  return decode_mla<kFp8>(q, ckv_cache, block_ids, {num_seqlen_per_req, &q_index, 0, true}, &indices, softmax_scale, output, output_lse,
                          return_lse, splits);
}

// ---- rope_norm_store_kv: the writer of that cache (csrc/mla_store.hip), pinned to tests/mla_store_ref.py --------------------
// Returns out_q_pe (the caller's, or a fresh contiguous one); an empty tensor when q_pe is not given.  With out_q_pe (or no
// q_pe) nothing is allocated and the call captures into a hipGraph.  Nothing here reads the values of num_seqlen_per_req,
// q_index or block_ids.
template <bool kFp8>
at::Tensor rope_norm_store_kv(const c10::optional<at::Tensor>& ckv_cache, const at::Tensor& kv_a, const at::Tensor& cos_sin,
                              const at::Tensor& kv_norm_weight, const at::Tensor& num_seqlen_per_req, const at::Tensor& q_index,
                              const at::Tensor& block_ids, const c10::optional<at::Tensor>& q_pe,
                              const c10::optional<at::Tensor>& out_q_pe, const c10::optional<at::Tensor>& out_ckv, double eps,
                              bool interleaved) {
  constexpr CacheKind kind = kCache<kFp8>;
  TORCH_CHECK(kv_a.is_cuda(), "kv_a tensor must be cuda");
  TORCH_CHECK(kv_a.dim() == 2 && kv_a.size(1) == hpc::kMlaRow, "kv_a must be [rows, 576]");
  const int64_t rows = kv_a.size(0);
  check_data(kv_a, "kv_a", kv_a, at::kBFloat16, {rows, hpc::kMlaRow}, kRows16);
  check_table(cos_sin, "cos_sin", kv_a, at::kFloat, {-1, hpc::kMlaRope});
  TORCH_CHECK(cos_sin.size(0) > 0, "cos_sin must be [max_pos, 64] with max_pos > 0");
  check_table(kv_norm_weight, "kv_norm_weight", kv_a, at::kFloat, {hpc::kMlaLatent});
  check_table(num_seqlen_per_req, "num_seqlen_per_req", kv_a, at::kInt, {-1});
  const int64_t num_req = num_seqlen_per_req.size(0);
  check_table(q_index, "q_index", kv_a, at::kInt, {num_req + 1});
  check_table(block_ids, "block_ids", kv_a, at::kInt, {num_req, -1});
  TORCH_CHECK(ckv_cache.has_value() || out_ckv.has_value(), "one of ckv_cache and out_ckv must be given");
  TORCH_CHECK(q_pe.has_value() || !out_q_pe.has_value(), "out_q_pe needs q_pe");
  TORCH_CHECK(cos_sin.size(0) <= INT32_MAX && rows <= INT32_MAX && num_req < INT32_MAX && block_ids.size(1) <= INT32_MAX,
              "sizes beyond int32");

  int64_t page = 16, block_stride = 0, token_stride = kind.row, num_blocks = 0;
  if (ckv_cache.has_value()) {
    const at::Tensor& c = *ckv_cache;
    TORCH_CHECK(c.is_cuda() && c.device() == kv_a.device(), "ckv_cache must be on kv_a's device");
    check_cache(c, kind);
    page = c.size(1), block_stride = c.stride(0), token_stride = c.stride(1), num_blocks = c.size(0);
    TORCH_CHECK(num_blocks <= INT32_MAX, "sizes beyond int32");
  }
  if (out_ckv.has_value()) check_data(*out_ckv, "out_ckv", kv_a, at::kBFloat16, {rows, hpc::kMlaRow}, kRows16);
  int64_t h = 0;
  at::Tensor oq = at::empty({0}, kv_a.options());
  if (q_pe.has_value()) {
    TORCH_CHECK(q_pe->dim() == 3 && q_pe->size(0) == rows && q_pe->size(2) == hpc::kMlaRope, "q_pe must be [rows, num_head, 64]");
    h = q_pe->size(1);
    TORCH_CHECK(h >= 1 && h <= 128, "num_head must be 1 .. 128, got ", h);
    check_data(*q_pe, "q_pe", kv_a, at::kBFloat16, {rows, h, hpc::kMlaRope}, kRows16);
    if (out_q_pe.has_value()) {
      check_data(*out_q_pe, "out_q_pe", kv_a, at::kBFloat16, {rows, h, hpc::kMlaRope}, kRows16);
      oq = *out_q_pe;
      const int64_t row_extent = (h - 1) * oq.stride(1) + hpc::kMlaRope;
      TORCH_CHECK(rows <= 1 || oq.stride(0) >= row_extent, "out_q_pe stride 0 = ", oq.stride(0),
                  " lets its rows overlap: num_head heads of stride ", oq.stride(1), " need ", row_extent);
      if (rows > 0) {  // q_pe and out_q_pe may share memory only as the same tensor (in place)
        const bool in_place = oq.data_ptr() == q_pe->data_ptr() && oq.strides() == q_pe->strides();
        const auto span = [&](const at::Tensor& t) {
          return hpc::byte_span(t.data_ptr(), rows, t.stride(0), h, t.stride(1), hpc::kMlaRope, 2);
        };
        TORCH_CHECK(in_place || !hpc::overlap(span(oq), span(*q_pe)),
                    "out_q_pe overlaps q_pe without being the same tensor: only the exact in-place form is supported");
      }
    } else {
      oq = at::empty({rows, h, hpc::kMlaRope}, kv_a.options());
    }
  }
  if (rows == 0 || num_req == 0) return oq;  // nothing to launch
  const bool with_q = q_pe.has_value();
  const int rc = (kFp8 ? hpc_mla_rope_norm_store_kv_fp8_async : hpc_mla_rope_norm_store_kv_async)(
      ptr(ckv_cache), ptr(out_ckv), with_q ? oq.data_ptr() : nullptr, ptr(kv_a), ptr(q_pe),
      static_cast<const float*>(cos_sin.data_ptr()), static_cast<const float*>(kv_norm_weight.data_ptr()),
      static_cast<const int*>(num_seqlen_per_req.data_ptr()), static_cast<const int*>(q_index.data_ptr()),
      static_cast<const int*>(block_ids.data_ptr()), i32(rows), i32(num_req), i32(h), i32(page), i32(block_ids.size(1)),
      i32(num_blocks), i32(cos_sin.size(0)), block_stride, token_stride, kv_a.stride(0),
      out_ckv.has_value() ? out_ckv->stride(0) : hpc::kMlaRow, with_q ? q_pe->stride(0) : 0, with_q ? q_pe->stride(1) : 0,
      with_q ? oq.stride(0) : 0, with_q ? oq.stride(1) : 0, static_cast<float>(eps), interleaved ? 1 : 0, stream_of(kv_a));
  HPC_LAUNCH_CHECK(rc, kFp8 ? "mla_rope_norm_store_kv_fp8" : "mla_rope_norm_store_kv");
  return oq;
}

// ---- gather_ckv: the reader of that cache for the prompt side (csrc/mla_gather.hip), pinned to tests/mla_gather_ref.py ------------
// Returns `output` (the caller's) or a fresh contiguous [num_rows, 576]; with `output` nothing is allocated and the call captures
// into a hipGraph.  Nothing here reads the values of block_ids, cu_seqlens or seq_starts: the row count is the host's.
template <bool kFp8>
at::Tensor gather_ckv(const at::Tensor& ckv_cache, const at::Tensor& block_ids, const at::Tensor& cu_seqlens,
                      const c10::optional<at::Tensor>& seq_starts, const c10::optional<at::Tensor>& output,
                      c10::optional<int64_t> num_rows) {
  TORCH_CHECK(ckv_cache.is_cuda(), "ckv_cache tensor must be cuda");
  check_cache(ckv_cache, kCache<kFp8>);
  check_table(cu_seqlens, "cu_seqlens", ckv_cache, at::kInt, {-1});
  TORCH_CHECK(cu_seqlens.size(0) >= 1, "cu_seqlens must be [num_req + 1]");
  const int64_t num_req = cu_seqlens.size(0) - 1;
  check_table(block_ids, "block_ids", ckv_cache, at::kInt, {num_req, -1});
  if (seq_starts.has_value()) check_table(*seq_starts, "seq_starts", ckv_cache, at::kInt, {num_req});
  TORCH_CHECK(output.has_value() || num_rows.has_value(), "one of output and num_rows must be given: the row count is a host value");
  at::Tensor out;
  if (output.has_value()) {
    TORCH_CHECK(output->dim() == 2 && output->size(1) == hpc::kMlaRow, "output must be [num_rows, 576]");
    TORCH_CHECK(!num_rows.has_value() || *num_rows == output->size(0), "num_rows = ", num_rows.value_or(0), " but output has ",
                output->size(0), " rows");
    check_data(*output, "output", ckv_cache, at::kBFloat16, {output->size(0), hpc::kMlaRow}, kRows16);
    out = *output;
  } else {
    TORCH_CHECK(*num_rows >= 0, "num_rows must not be negative, got ", *num_rows);
    out = at::empty({*num_rows, hpc::kMlaRow}, ckv_cache.options().dtype(at::kBFloat16));
  }
  const int64_t rows = out.size(0);
  TORCH_CHECK(rows <= INT32_MAX - 32 && num_req < INT32_MAX && block_ids.size(1) <= INT32_MAX && ckv_cache.size(0) <= INT32_MAX,
              "sizes beyond int32");
  if (rows == 0 || num_req == 0) return out;  // nothing to launch
  const int rc = (kFp8 ? hpc_mla_gather_ckv_fp8_async : hpc_mla_gather_ckv_async)(
      ptr(out), ptr(ckv_cache), static_cast<const int*>(block_ids.data_ptr()), static_cast<const int*>(cu_seqlens.data_ptr()),
      seq_starts.has_value() ? static_cast<const int*>(seq_starts->data_ptr()) : nullptr, i32(rows), i32(num_req),
      i32(ckv_cache.size(1)), i32(block_ids.size(1)), i32(ckv_cache.size(0)), ckv_cache.stride(0), ckv_cache.stride(1),
      out.stride(0), stream_of(ckv_cache));
  HPC_LAUNCH_CHECK(rc, kFp8 ? "mla_gather_ckv_fp8" : "mla_gather_ckv");
  return out;
}

// ---- attention_prefill_mla_bf16 (csrc/attention_prefill_mla.hip), pinned to tests/mla_prefill_ref.py -------------------------
// The stride rules of q, k_nope, k_pe and v (multiples of 8, wide enough, 16-byte base) are the route's
// (csrc/attention_prefill_mla_route.h) and come back as its refusal.  Nothing here reads the values of cu_seqlens_q /
// cu_seqlens_k; with output (and output_lse where an lse is wanted) given nothing is allocated and the call captures into a
// hipGraph.
std::tuple<at::Tensor, at::Tensor> attention_prefill_mla_bf16(const at::Tensor& q, const at::Tensor& k_nope, const at::Tensor& k_pe,
                                                              const at::Tensor& v, const at::Tensor& cu_seqlens_q,
                                                              int64_t max_seqlens_q, double softmax_scale,
                                                              const c10::optional<at::Tensor>& cu_seqlens_k,
                                                              c10::optional<int64_t> max_seqlens_k, bool causal,
                                                              const c10::optional<at::Tensor>& output,
                                                              const c10::optional<at::Tensor>& output_lse, bool return_lse) {
  TORCH_CHECK(q.is_cuda(), "q tensor must be cuda");
  check_data(q, "q", q, at::kBFloat16, {-1, -1, kNope + hpc::kMlaRope});
  const int64_t tq = q.size(0), h = q.size(1), tk = k_nope.dim() > 0 ? k_nope.size(0) : 0;
  check_data(k_nope, "k_nope", q, at::kBFloat16, {-1, -1, kNope});
  check_data(v, "v", q, at::kBFloat16, {-1, -1, kNope});
  check_data(k_pe, "k_pe", q, at::kBFloat16, {-1, hpc::kMlaRope});
  TORCH_CHECK(k_nope.size(1) == h && v.size(1) == h, "k_nope and v must have q's ", h, " heads");
  TORCH_CHECK(v.size(0) == tk && k_pe.size(0) == tk, "k_nope, k_pe and v must have the same number of rows");
  check_table(cu_seqlens_q, "cu_seqlens_q", q, at::kInt, {-1});
  TORCH_CHECK(cu_seqlens_q.size(0) >= 1, "cu_seqlens_q must be [num_batch + 1]");
  if (cu_seqlens_k.has_value()) {
    check_table(*cu_seqlens_k, "cu_seqlens_k", q, at::kInt, {cu_seqlens_q.size(0)});
    TORCH_CHECK(max_seqlens_k.has_value(), "cu_seqlens_k needs max_seqlens_k");
  }
  TORCH_CHECK(max_seqlens_q >= 0 && max_seqlens_q <= INT32_MAX && tq <= INT32_MAX && tk <= INT32_MAX &&
                  (!max_seqlens_k.has_value() || (*max_seqlens_k >= 0 && *max_seqlens_k <= INT32_MAX)),
              "max_seqlens_q / max_seqlens_k must be non-negative int32 counts");
  const int64_t b = cu_seqlens_q.size(0) - 1;
  at::Tensor out = out_or_new(output, q, {tq, h, kNope}, at::kBFloat16, "output", kOnInputDevice);
  const bool want_lse = return_lse || output_lse.has_value();
  at::Tensor lse = want_lse ? out_or_new(output_lse, q, {tq, h}, at::kFloat, "output_lse", kOnInputDevice)
                            : at::empty({0}, q.options().dtype(at::kFloat));
  if (b == 0 || tq == 0) return {out, lse};  // nothing to launch
  // an empty k side (every request without context) has no storage to point at: the kernel reads no row of it, q stands in
  const bool no_keys = tk == 0;
  const int rc = hpc_attention_prefill_mla_bf16_async(
      ptr(out), want_lse ? static_cast<float*>(lse.data_ptr()) : nullptr, ptr(q), no_keys ? ptr(q) : ptr(k_nope),
      no_keys ? ptr(q) : ptr(k_pe), no_keys ? ptr(q) : ptr(v), static_cast<const int*>(cu_seqlens_q.data_ptr()),
      cu_seqlens_k.has_value() ? static_cast<const int*>(cu_seqlens_k->data_ptr()) : nullptr, i32(b), i32(h), i32(max_seqlens_q),
      max_seqlens_k.has_value() ? i32(*max_seqlens_k) : -1, q.stride(0), q.stride(1), no_keys ? kNope * h : k_nope.stride(0),
      no_keys ? kNope : k_nope.stride(1), no_keys ? hpc::kMlaRope : k_pe.stride(0), no_keys ? kNope * h : v.stride(0),
      no_keys ? kNope : v.stride(1),
      static_cast<float>(softmax_scale), causal ? 1 : 0, stream_of(q));
  HPC_LAUNCH_CHECK(rc, "attention_prefill_mla_bf16");
  return {out, lse};
}

// ---- merge_attn_states (csrc/merge_attn_states.hip) ----------------------------------------------------------------------------
std::tuple<at::Tensor, at::Tensor> merge_attn_states(const at::Tensor& out_a, const at::Tensor& lse_a, const at::Tensor& out_b,
                                                     const at::Tensor& lse_b, const c10::optional<at::Tensor>& output,
                                                     const c10::optional<at::Tensor>& output_lse) {
  TORCH_CHECK(out_a.is_cuda(), "out_a tensor must be cuda");
  TORCH_CHECK(out_a.dim() == 3, "out_a must be [T, H, D]");
  const int64_t t = out_a.size(0), h = out_a.size(1), d = out_a.size(2);
  check_data(out_a, "out_a", out_a, at::kBFloat16, {t, h, d});
  check_data(out_b, "out_b", out_a, at::kBFloat16, {t, h, d});
  check_table(lse_a, "lse_a", out_a, at::kFloat, {t, h});
  check_table(lse_b, "lse_b", out_a, at::kFloat, {t, h});
  TORCH_CHECK(d > 0 && d % 8 == 0 && d <= 512, "D must be a multiple of 8, 8 .. 512, got ", d);
  TORCH_CHECK(h <= INT32_MAX, "sizes beyond int32");
  at::Tensor out = output.has_value() ? *output : at::empty({t, h, d}, out_a.options());
  at::Tensor lse = output_lse.has_value() ? *output_lse : at::empty({t, h}, lse_a.options());
  if (output.has_value()) check_data(out, "output", out_a, at::kBFloat16, {t, h, d});
  if (output_lse.has_value()) check_table(lse, "output_lse", out_a, at::kFloat, {t, h});
  if (t == 0 || h == 0) return {out, lse};
  const int rc = hpc_merge_attn_states_async(ptr(out), static_cast<float*>(lse.data_ptr()), ptr(out_a),
                                             static_cast<const float*>(lse_a.data_ptr()), ptr(out_b),
                                             static_cast<const float*>(lse_b.data_ptr()), t, i32(h), i32(d), out.stride(0), out.stride(1),
                                             out_a.stride(0), out_a.stride(1), out_b.stride(0), out_b.stride(1), stream_of(out_a));
  HPC_LAUNCH_CHECK(rc, "merge_attn_states");
  return {out, lse};
}

// ---- absorb_q / unabsorb_o (csrc/mla_absorb.hip), pinned to tests/mla_absorb_ref.py --------------------------------------------
// dtype, device, shape and the contiguous last dim here; strides, alignment, H and overlap are the route's
// (csrc/mla_absorb_route.h) and come back in its words.  With the outputs given nothing is allocated and nothing is read on the host.
at::Tensor absorb_q(const at::Tensor& q_nope, const at::Tensor& w_uk, const c10::optional<at::Tensor>& output) {
  TORCH_CHECK(q_nope.is_cuda(), "q_nope tensor must be cuda");
  TORCH_CHECK(q_nope.dim() == 3 && q_nope.size(2) == kNope, "q_nope must be [T, num_head, 128]");
  const int64_t t = q_nope.size(0), h = q_nope.size(1);
  TORCH_CHECK(h <= INT32_MAX, "sizes beyond int32");
  check_data(q_nope, "q_nope", q_nope, at::kBFloat16, {t, h, kNope});
  check_data(w_uk, "w_uk", q_nope, at::kBFloat16, {h, kNope, hpc::kMlaLatent});
  at::Tensor out;
  if (output.has_value()) {
    check_data(*output, "output", q_nope, at::kBFloat16, {t, h, hpc::kMlaLatent});
    out = *output;
  } else {
    out = at::empty({t, h, hpc::kMlaLatent}, q_nope.options());
  }
  checked_launch("mla_absorb_q", hpc_mla_absorb_q_refusal, hpc_mla_absorb_q_async, t > 0,
                 std::make_tuple(ptr(out), ptr(q_nope), ptr(w_uk), t, i32(h), q_nope.stride(0), q_nope.stride(1), w_uk.stride(0),
                                 w_uk.stride(1), out.stride(0), out.stride(1)),
                 std::make_tuple(stream_of(q_nope)));
  return out;
}

// (o, scale): quant false: o bf16 [T, H * 128] and an empty scale; quant true: the (x, x_scale) pair of gemm_blockwise_fp8
std::tuple<at::Tensor, at::Tensor> unabsorb_o(const at::Tensor& o_lat, const at::Tensor& w_uv, const c10::optional<at::Tensor>& output,
                                              bool quant, const c10::optional<at::Tensor>& output_scale) {
  TORCH_CHECK(o_lat.is_cuda(), "o_lat tensor must be cuda");
  TORCH_CHECK(o_lat.dim() == 3 && o_lat.size(2) == hpc::kMlaLatent, "o_lat must be [T, num_head, 512]");
  const int64_t t = o_lat.size(0), h = o_lat.size(1);
  TORCH_CHECK(h <= INT32_MAX, "sizes beyond int32");
  check_data(o_lat, "o_lat", o_lat, at::kBFloat16, {t, h, hpc::kMlaLatent});
  check_data(w_uv, "w_uv", o_lat, at::kBFloat16, {h, kNope, hpc::kMlaLatent});
  TORCH_CHECK(quant || !output_scale.has_value(), "output_scale needs quant=True");
  const at::ScalarType odt = quant ? kF8 : at::kBFloat16;
  at::Tensor out, scale = at::empty({0}, o_lat.options().dtype(at::kFloat));
  if (output.has_value()) {
    check_data(*output, "output", o_lat, odt, {t, h * kNope});
    out = *output;
  } else {
    out = at::empty({t, h * kNope}, o_lat.options().dtype(odt));
  }
  if (quant) {
    if (output_scale.has_value()) {
      check_table(*output_scale, "output_scale", o_lat, at::kFloat, {t, h});
      scale = *output_scale;
    } else {
      scale = at::empty({t, h}, o_lat.options().dtype(at::kFloat));
    }
  }
  // a [1, N] or [0, N] tensor carries any row stride: the route is told the contiguous one
  const int64_t out_rs = t > 1 ? out.stride(0) : h * kNope;
  float* sp = quant ? static_cast<float*>(scale.data_ptr()) : nullptr;
  checked_launch("mla_unabsorb_o", hpc_mla_unabsorb_o_refusal, hpc_mla_unabsorb_o_async, t > 0,
                 std::make_tuple(ptr(out), sp, ptr(o_lat), ptr(w_uv), t, i32(h), o_lat.stride(0), o_lat.stride(1), w_uv.stride(0),
                                 w_uv.stride(1), out_rs, quant ? 1 : 0),
                 std::make_tuple(stream_of(o_lat)));
  return {out, scale};
}

}  // namespace

TORCH_LIBRARY(hpc_mla, m) {
  m.def("absorb_q(Tensor q_nope, Tensor w_uk, Tensor? output) -> Tensor");
  m.def("unabsorb_o(Tensor o_lat, Tensor w_uv, Tensor? output, bool quant, Tensor? output_scale) -> (Tensor, Tensor)");
  m.def(
      "rope_norm_store_kv(Tensor? ckv_cache, Tensor kv_a, Tensor cos_sin, Tensor kv_norm_weight, Tensor num_seqlen_per_req, "
      "Tensor q_index, Tensor block_ids, Tensor? q_pe, Tensor? out_q_pe, Tensor? out_ckv, float eps, bool interleaved) -> Tensor");
  m.def(
      "attention_decode_mla_bf16(Tensor q, Tensor ckv_cache, Tensor block_ids, Tensor num_seq_kvcache, float softmax_scale, "
      "int mtp, bool new_kv_included, Tensor? output, Tensor? output_lse, bool return_lse, int splits) -> (Tensor, Tensor)");
  m.def(
      "rope_norm_store_kv_fp8(Tensor? ckv_cache, Tensor kv_a, Tensor cos_sin, Tensor kv_norm_weight, Tensor num_seqlen_per_req, "
      "Tensor q_index, Tensor block_ids, Tensor? q_pe, Tensor? out_q_pe, Tensor? out_ckv, float eps, bool interleaved) -> Tensor");
  m.def(
      "attention_decode_mla_fp8(Tensor q, Tensor ckv_cache, Tensor block_ids, Tensor num_seq_kvcache, float softmax_scale, "
      "int mtp, bool new_kv_included, Tensor? output, Tensor? output_lse, bool return_lse, int splits) -> (Tensor, Tensor)");
  m.def(
      "attention_decode_mla_sparse_bf16(Tensor q, Tensor ckv_cache, Tensor block_ids, Tensor num_seq_kvcache, Tensor indices, "
      "float softmax_scale, int mtp, bool new_kv_included, Tensor? output, Tensor? output_lse, bool return_lse, int splits) -> "
      "(Tensor, Tensor)");
  m.def(
      "attention_decode_mla_sparse_fp8(Tensor q, Tensor ckv_cache, Tensor block_ids, Tensor num_seq_kvcache, Tensor indices, "
      "float softmax_scale, int mtp, bool new_kv_included, Tensor? output, Tensor? output_lse, bool return_lse, int splits) -> "
      "(Tensor, Tensor)");
  m.def(
      "attention_prefill_mla_sparse_bf16(Tensor q, Tensor ckv_cache, Tensor block_ids, Tensor num_seqlen_per_req, Tensor q_index, "
      "Tensor indices, float softmax_scale, Tensor? output, Tensor? output_lse, bool return_lse, int splits) -> (Tensor, Tensor)");
  m.def(
      "attention_prefill_mla_sparse_fp8(Tensor q, Tensor ckv_cache, Tensor block_ids, Tensor num_seqlen_per_req, Tensor q_index, "
      "Tensor indices, float softmax_scale, Tensor? output, Tensor? output_lse, bool return_lse, int splits) -> (Tensor, Tensor)");
  m.def(
      "attention_prefill_mla_bf16(Tensor q, Tensor k_nope, Tensor k_pe, Tensor v, Tensor cu_seqlens_q, int max_seqlens_q, "
      "float softmax_scale, Tensor? cu_seqlens_k, int? max_seqlens_k, bool causal, Tensor? output, Tensor? output_lse, "
      "bool return_lse) -> (Tensor, Tensor)");
  m.def(
      "merge_attn_states(Tensor out_a, Tensor lse_a, Tensor out_b, Tensor lse_b, Tensor? output, Tensor? output_lse) -> "
      "(Tensor, Tensor)");
  m.def("gather_ckv(Tensor ckv_cache, Tensor block_ids, Tensor cu_seqlens, Tensor? seq_starts, Tensor? output, int? num_rows) -> Tensor");
  m.def(
      "gather_ckv_fp8(Tensor ckv_cache, Tensor block_ids, Tensor cu_seqlens, Tensor? seq_starts, Tensor? output, int? num_rows) -> "
      "Tensor");
  // the cached split-KV scratch buffers (tests fill them with NaN bytes: no piece that was not written may be read)
  m.def("_workspaces() -> Tensor[]", []() { return list_cached_scratch(kScratchMla); });
}

TORCH_LIBRARY_IMPL(hpc_mla, CUDA, m) {
  m.impl("attention_decode_mla_bf16", &attention_decode_mla<false>);
  m.impl("rope_norm_store_kv", &rope_norm_store_kv<false>);
  m.impl("attention_decode_mla_fp8", &attention_decode_mla<true>);
  m.impl("rope_norm_store_kv_fp8", &rope_norm_store_kv<true>);
  m.impl("attention_decode_mla_sparse_bf16", &attention_decode_mla_sparse<false>);
  m.impl("attention_decode_mla_sparse_fp8", &attention_decode_mla_sparse<true>);
  m.impl("attention_prefill_mla_sparse_bf16", &attention_prefill_mla_sparse<false>);
  m.impl("attention_prefill_mla_sparse_fp8", &attention_prefill_mla_sparse<true>);
  m.impl("attention_prefill_mla_bf16", &attention_prefill_mla_bf16);
  m.impl("merge_attn_states", &merge_attn_states);
  m.impl("gather_ckv", &gather_ckv<false>);
  m.impl("gather_ckv_fp8", &gather_ckv<true>);
  m.impl("absorb_q", &absorb_q);
  m.impl("unabsorb_o", &unabsorb_o);
}
