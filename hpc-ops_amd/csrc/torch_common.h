// Shared by the C++ host translation units (csrc/torch_*.cpp -> hpc/_hpc_torch.so): stream lookup, raw pointers,
// the launch-failed convention of the reference (TORCH_CHECK(running, "<op> launch failed!"), src/attention/entry.cc:722).
#pragma once
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "hpc_amd.h"

namespace hpc_torch {

inline hpc_stream_t stream_of(const at::Tensor& t) {
  // reference: at::cuda::getCurrentCUDAStream(tensor.device) - the current stream of the tensor's device
  return reinterpret_cast<hpc_stream_t>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

inline const char* err_text(int code) {
  switch (code) {
    case -1: return "unsupported configuration";
    case -2: return "invalid argument";
    case -3: return "HIP launch error";
    case -4: return "an earlier fused all-reduce timed out waiting for a peer";
    default: return "error";
  }
}
#define HPC_LAUNCH_CHECK(rc, what) TORCH_CHECK((rc) == 0, what, " launch failed! (", ::hpc_torch::err_text(rc), ")")

// An op whose C entry has a `_refusal` twin: the refusal in words first, then - with work - the launch.  The launcher's
// arguments are the refusal's plus `tail` (a stream, or flags and a stream), so the list is stated once and the call that was
// checked is the call that is launched.
template <class Refusal, class Launch, class... Args, class... Tail>
void checked_launch(const char* op, Refusal refusal, Launch launch, bool work, const std::tuple<Args...>& args,
                    const std::tuple<Tail...>& tail) {
  const char* why = std::apply(refusal, args);
  TORCH_CHECK(why == nullptr, op, ": ", why);
  if (!work) return;  // nothing to launch
  const int rc = std::apply(launch, std::tuple_cat(args, tail));
  HPC_LAUNCH_CHECK(rc, op);
}

inline void* ptr(const at::Tensor& t) { return t.data_ptr(); }
inline void* ptr(const c10::optional<at::Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }

inline void cuda_contig(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " tensor must be cuda");
  TORCH_CHECK(t.is_contiguous(), name, " tensor must be contiguous");
}
inline int i32(int64_t v) { return static_cast<int>(v); }

const auto kF8 = at::kFloat8_e4m3fn;

// An output given by the caller, or a fresh one on `like`'s device: dtype, device, contiguity and shape are checked either
// way.  off_device: the message's words for a tensor elsewhere, which name `like` as its op does.  An int32 output is
// named the way speculative_verify's always were, every other dtype by its ATen name.
constexpr const char* kOnLogitsDevice = " must be on the logits' device";
constexpr const char* kOnInputDevice = " must be on the input's device";
inline at::Tensor out_or_new(const c10::optional<at::Tensor>& given, const at::Tensor& like, at::IntArrayRef shape,
                             at::ScalarType dtype, const char* name, const char* off_device) {
  if (!given.has_value()) return at::empty(shape, like.options().dtype(dtype));
  const at::Tensor& o = *given;
  TORCH_CHECK(o.is_cuda() && o.device() == like.device(), name, off_device);
  if (dtype == at::kInt) {
    TORCH_CHECK(o.scalar_type() == dtype, name, " dtype must be int32");
  } else {
    TORCH_CHECK(o.scalar_type() == dtype, name, " dtype must be ", dtype);
  }
  TORCH_CHECK(o.is_contiguous() && o.sizes() == shape, name, " must be a contiguous tensor of shape ", shape);
  return o;
}

// ---- argument checks of the ops that take [rows, vocab] logits (fused samplers, speculative_verify) ------------------
// Messages as in the reference (src/sampler/entry.cc:13-255).  The stricter forms are speculative_verify's: a vocabulary
// that is not empty, and optional tensors on the logits' device (same_device_as).
struct LogitsDims {
  int64_t b, v;
};
inline LogitsDims check_logits(const at::Tensor& logits, const char* who, bool nonempty_vocab = false) {
  TORCH_CHECK(logits.is_cuda(), "logits must be a device tensor");
  TORCH_CHECK(logits.dim() == 2, "logits tensor must be dim == 2");
  TORCH_CHECK(logits.scalar_type() == at::kFloat || logits.scalar_type() == at::kBFloat16, "logits dtype must be float32 or bfloat16");
  const int64_t b = logits.size(0), v = logits.size(1);
  TORCH_CHECK(logits.stride(1) == 1, who, ": logits must have contiguous inner dim (stride(1)=1), got stride(1)=", logits.stride(1));
  TORCH_CHECK(logits.stride(0) >= v, who, ": logits stride(0)=", logits.stride(0), " must be >= vocab_size=", v);
  TORCH_CHECK((v > 0 || !nonempty_vocab) && v % 8 == 0 && v < (1 << 20), who, ": unsupported vocab_size ", v,
              " (must be a multiple of 8, < 2^20)");
  return {b, v};
}
inline void check_same_device(const at::Tensor& t, const char* name, const at::Tensor* same_device_as) {
  if (same_device_as) {
    TORCH_CHECK(t.is_cuda() && t.device() == same_device_as->device(), name, kOnLogitsDevice);
  }
}
inline void check_1d_float(const c10::optional<at::Tensor>& t, const char* name, int64_t b,
                           const at::Tensor* same_device_as = nullptr) {
  if (!t.has_value()) return;
  check_same_device(*t, name, same_device_as);
  TORCH_CHECK(t->is_contiguous(), name, " tensor must be contiguous");
  TORCH_CHECK(t->scalar_type() == at::kFloat, name, " dtype must be float32");
  TORCH_CHECK(t->dim() == 1, name, " tensor must be 1D");
  TORCH_CHECK(t->size(0) == b, name, " size must be [batch_size=", b, "], got [", t->size(0), "]");
}
inline void check_noise(const c10::optional<at::Tensor>& g, int64_t b, int64_t v, const at::Tensor* same_device_as = nullptr) {
  if (!g.has_value()) return;
  check_same_device(*g, "gumbel_noise", same_device_as);
  TORCH_CHECK(g->is_contiguous(), "gumbel_noise tensor must be contiguous");
  TORCH_CHECK(g->scalar_type() == at::kFloat, "gumbel_noise dtype must be float32");
  TORCH_CHECK(g->dim() == 2, "gumbel_noise must be 2D");
  TORCH_CHECK(g->size(0) == b && g->size(1) == v, "gumbel_noise shape must be [", b, ", ", v, "]");
}

// ---- zero-once scratch --------------------------------------------------------------------------------------------
// Some kernels keep arrival counters in caller scratch that must be ZERO the first time a buffer is used and that
// every call leaves zero again (decode: the counters of split requests; router GEMM: its split-K tickets; dense FP8 linear:
// its split-K tickets in front of its partial planes).  Instead of
// an allocation + a zero-fill launch per call, such scratch is one buffer per (purpose, device, stream, hipGraph
// capture), allocated once with its first `zero_bytes` bytes zeroed.  Calls on one stream are ordered, so sharing the
// buffer between them is safe; different streams get different buffers.  A buffer first used while a hipGraph is being
// captured has its zero-fill only RECORDED (a node of that graph): the key carries the capture id, so such a buffer
// serves the calls of that capture and nothing else, the entries of earlier (ended) captures on the stream are dropped on
// the next call (their memory stays with their graph's pool), and a buffer cached by eager calls is not used inside a capture - every graph
// owns its buffer and its zero node.
enum ScratchPurpose { kScratchDecode = 0, kScratchGemmFlags = 1, kScratchLinear = 2, kScratchMla = 3, kScratchMlaIndexer = 4,
                      kScratchMlaIndexerPrefill = 5 };
using ScratchKey = std::tuple<int, int, void*, long long>;
inline std::mutex& scratch_mutex() {
  static std::mutex mu;
  return mu;
}
inline std::map<ScratchKey, at::Tensor>& scratch_cache() {
  // never destroyed: tensors must not be released during static destruction, after the allocator is gone
  static auto& cache = *new std::map<ScratchKey, at::Tensor>();
  return cache;
}
inline at::Tensor cached_scratch(int purpose, const at::Tensor& like, int64_t nbytes, int64_t zero_bytes) {
  const auto hip_stream = stream_of(like);
  void* stream = static_cast<void*>(hip_stream);
  const long long cap = hpc_stream_capture_id(hip_stream);
  TORCH_CHECK(cap >= 0, "hipStreamGetCaptureInfo failed");
  const int dev = static_cast<int>(like.device().index());
  const ScratchKey key{purpose, dev, stream, cap};
  std::lock_guard<std::mutex> lock(scratch_mutex());
  auto& cache = scratch_cache();
  // Entries of captures that have ENDED on this stream are dropped on every call, not only on a miss: a
  // stream records one capture at a time, so every entry of this (purpose, device, stream) whose capture id is neither
  // 0 (eager) nor the current one belongs to a finished capture - its tensor lives in that graph's private pool and the
  // cache must not keep the pool alive after the graph is destroyed.
  for (auto o = cache.begin(); o != cache.end();)
    o = (std::get<0>(o->first) == purpose && std::get<1>(o->first) == dev && std::get<2>(o->first) == stream &&
         std::get<3>(o->first) != 0 && std::get<3>(o->first) != cap)
            ? cache.erase(o)
            : std::next(o);
  auto it = cache.find(key);
  if (it == cache.end() || it->second.numel() < nbytes) {
    at::Tensor ws = at::empty({nbytes}, like.options().dtype(at::kByte));
    if (zero_bytes > 0) ws.narrow(0, 0, std::min(zero_bytes, nbytes)).zero_();
    it = cache.insert_or_assign(key, ws).first;
  }
  return it->second;
}
// Drops EVERY cached scratch buffer of every purpose: the decode workspaces, the router GEMM's split-K ticket buffers AND
// the dense FP8 linear's tickets + planes, the MLA decode's split-KV partials and the MLA indexer's logits (a decode step's and
// a prefill slab's)
// (hpc.release_decode_workspaces documents them).
inline void release_cached_scratch() {
  std::lock_guard<std::mutex> lock(scratch_mutex());
  scratch_cache().clear();
}
inline std::vector<at::Tensor> list_cached_scratch(int purpose) {
  std::lock_guard<std::mutex> lock(scratch_mutex());
  std::vector<at::Tensor> out;
  for (auto& kv : scratch_cache())
    if (std::get<0>(kv.first) == purpose) out.push_back(kv.second);
  return out;
}

}  // namespace hpc_torch
