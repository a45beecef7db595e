// The bytes a strided [rows, heads, width] view covers, and whether two such ranges share a byte: what the host checks of the
// MLA ops refuse overlapping operands with; behind them the alignment test and the span limit of every host check.  Internal
// header, plain C++, host only; addresses are compared, never dereferenced.
#pragma once
#include <stdint.h>

namespace hpc {

struct ByteSpan {
  uintptr_t lo, hi;  // [lo, hi)
};

// rows >= 1 and heads >= 1; strides in elements of `elem` bytes.  A [rows, width] view is heads = 1 with any head stride.
static inline ByteSpan byte_span(uintptr_t base, int64_t rows, int64_t row_stride, int64_t heads, int64_t head_stride, int64_t width,
                                 int64_t elem) {
  return {base, base + static_cast<uintptr_t>(elem * ((rows - 1) * row_stride + (heads - 1) * head_stride + width))};
}
static inline ByteSpan byte_span(const void* base, int64_t rows, int64_t row_stride, int64_t heads, int64_t head_stride,
                                 int64_t width, int64_t elem) {
  return byte_span(reinterpret_cast<uintptr_t>(base), rows, row_stride, heads, head_stride, width, elem);
}
static inline bool overlap(ByteSpan a, ByteSpan b) { return a.lo < b.hi && b.lo < a.hi; }

// What the host checks ask of a base address and of a stride: a multiple of `a` bytes, and offsets (page id x block stride,
// row x row stride) that stay inside 2^60 bytes, so that sums of two of them stay below 2^61
static inline bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }
constexpr int64_t kMaxSpan = int64_t{1} << 60;

}  // namespace hpc
