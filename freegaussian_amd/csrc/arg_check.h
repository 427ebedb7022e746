// The fused ops' aliasing rule (include/fgraster.h: no output may overlap an input or another output), stated once for the
// entry points of se3_apply.hip, control.hip, bilagrid.hip, color_correct.hip, target_loss.hip, flow_disp.hip, flow_loss.hip and optflow.hip.  Host only: addresses are compared, nothing
// is read through them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace fg_args {

// `bytes` bytes at p (null: absent, overlaps nothing)
struct span { const void* p; size_t bytes; };
// rows of `width` floats, `stride` floats apart, at p (null: absent, its stride is not looked at)
struct rows { const void* p; int64_t stride; int width; };

// bytes of n rows of `width` floats, `stride` floats apart, from the first to the last float read or written (n >= 1)
inline size_t span_bytes(int64_t n, int64_t stride, int width) {
  return ((size_t)(n - 1) * (size_t)stride + (size_t)width) * sizeof(float);
}
inline span rows_span(const rows& r, int64_t n) { return {r.p, r.p ? span_bytes(n, r.stride, r.width) : 0}; }

// (a span of no bytes still counts where it lies strictly inside the other: "absent" is a null pointer, not a length of 0)
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}
inline bool overlap(const span& a, const span& b) { return overlap(a.p, a.bytes, b.p, b.bytes); }

inline bool aligned(const void* p, size_t bytes) { return (uintptr_t)p % bytes == 0; }

// of one row set, and of a table of them: is any of them?
inline bool stride_invalid(const rows& r) { return r.p && r.stride < r.width; }
inline bool stride_far(const rows& r, int64_t max_stride) { return r.p && r.stride > max_stride; }
template <size_t K>
bool stride_invalid(const rows (&table)[K]) {
  return std::any_of(table, table + K, [](const rows& r) { return stride_invalid(r); });
}
template <size_t K>
bool stride_far(const rows (&table)[K], int64_t max_stride) {
  return std::any_of(table, table + K, [=](const rows& r) { return stride_far(r, max_stride); });
}

// two row sets that may be columns of one block (interleaved rows, as the heads of mlp_train's [N,13] and [n,10] blocks are):
// their spans overlap, their floats do not, where both have the same stride, lie whole floats apart and their column ranges
// do not meet
inline bool columns_apart(const rows& a, const rows& b) {
  if (a.stride != b.stride) return false;
  const rows& lo = (uintptr_t)a.p <= (uintptr_t)b.p ? a : b;
  const rows& hi = (uintptr_t)a.p <= (uintptr_t)b.p ? b : a;
  const uintptr_t apart = (uintptr_t)hi.p - (uintptr_t)lo.p;
  return apart % sizeof(float) == 0 && apart >= (size_t)lo.width * sizeof(float) &&
         apart + (size_t)hi.width * sizeof(float) <= (size_t)lo.stride * sizeof(float);
}

// does any output meet an input, or another output?  Tables may be written in place: clash({{out, bytes}}, {{a, na}, {b, nb}})
template <size_t NO, size_t NI>
bool clash(const span (&outs)[NO], const span (&ins)[NI]) {
  for (size_t i = 0; i < NO; ++i) {
    for (const span& in : ins)
      if (overlap(outs[i], in)) return true;
    for (size_t j = i + 1; j < NO; ++j)
      if (overlap(outs[i], outs[j])) return true;
  }
  return false;
}

// the same for outputs of n rows each (n >= 1), which may meet each other as columns of one block
template <size_t NO, size_t NI>
bool clash(const rows (&outs)[NO], int64_t n, const span (&ins)[NI]) {
  for (size_t i = 0; i < NO; ++i) {
    const span out = rows_span(outs[i], n);
    for (const span& in : ins)
      if (overlap(out, in)) return true;
    for (size_t j = i + 1; j < NO; ++j)
      if (overlap(out, rows_span(outs[j], n)) && !columns_apart(outs[i], outs[j])) return true;
  }
  return false;
}

}  // namespace fg_args
