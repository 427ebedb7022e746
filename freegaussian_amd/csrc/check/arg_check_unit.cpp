// Stand-alone host check of arg_check.h -- the spans, the column exception and the outputs-against-inputs rule that
// se3_apply.hip, control.hip, bilagrid.hip and color_correct.hip share -- compiled with AddressSanitizer +
// UndefinedBehaviorSanitizer (make arg-check).  Addresses are compared and never read: the program needs no GPU, links no
// unit and touches nothing.
#include "check_common.h"

#include "../arg_check.h"

using namespace fg_args;

// addresses nobody reads, 16 MiB apart from 1 GiB on
static char* at(int i) { return reinterpret_cast<char*>(((uintptr_t)1 << 30) + ((uintptr_t)i << 24)); }
static const float* fl(int i, ptrdiff_t floats = 0) { return reinterpret_cast<const float*>(at(i)) + floats; }

// a and b, asked in either order
static void expect_overlap(const void* a, size_t na, const void* b, size_t nb, bool want) {
  EXPECT(overlap(a, na, b, nb), want);
  EXPECT(overlap(b, nb, a, na), want);
  EXPECT(overlap(span{a, na}, span{b, nb}), want);
}
static void expect_apart(const rows& a, const rows& b, bool want) {
  EXPECT(columns_apart(a, b), want);
  EXPECT(columns_apart(b, a), want);
}

int main() {
  // ---- overlap: adjacent, one shared byte, nested, null
  expect_overlap(at(0), 100, at(0) + 100, 50, false);
  expect_overlap(at(0), 101, at(0) + 100, 50, true);
  expect_overlap(at(0), 100, at(0) + 99, 1, true);
  expect_overlap(at(0), 100, at(0) + 40, 10, true);
  expect_overlap(at(0), 100, at(0), 100, true);
  expect_overlap(nullptr, 100, at(0), 100, false);
  expect_overlap(nullptr, 100, nullptr, 100, false);
  expect_overlap(nullptr, (size_t)1 << 62, at(0), (size_t)1 << 40, false);
  // the span of no bytes as it behaves today: it counts strictly inside the other, not at its first byte, its end or outside;
  // two of them never meet.  (Absent arguments are null, which is why no caller depends on this.)
  expect_overlap(at(0) + 40, 0, at(0), 100, true);
  expect_overlap(at(0), 0, at(0), 100, false);
  expect_overlap(at(0) + 100, 0, at(0), 100, false);
  expect_overlap(at(1), 0, at(0), 100, false);
  expect_overlap(at(0), 0, at(0), 0, false);
  // ---- span_bytes
  EXPECT(span_bytes(1, 3, 3), 12);
  EXPECT(span_bytes(1, 13, 3), 12);  // (one row: the stride does not count)
  EXPECT(span_bytes(1, 4, 4), 16);
  EXPECT(span_bytes(1, 1 << 16, 4), 16);
  EXPECT(span_bytes(1000, 3, 3), 12000);
  EXPECT(span_bytes(1000, 4, 4), 16000);
  EXPECT(span_bytes(1000, 13, 3), (999 * 13 + 3) * 4);
  EXPECT(span_bytes(1000, 10, 4), (999 * 10 + 4) * 4);
  // the largest rows the SE(3) transform takes: (2^38 - 1) 2^16 + 3 floats, below 2^56 bytes
  const unsigned long long far = (((1ull << 38) - 1) * (1ull << 16) + 3) * 4;
  EXPECT(span_bytes(FG_SE3_MAX_ROWS, FG_SE3_MAX_STRIDE, 3) == far, 1);
  EXPECT(span_bytes(FG_SE3_MAX_ROWS, FG_SE3_MAX_STRIDE, 4) == far + 4, 1);
  EXPECT(far < (1ull << 56), 1);
  EXPECT(rows_span({fl(0), 13, 3}, 1000).bytes, (999 * 13 + 3) * 4);
  EXPECT(rows_span({fl(0), 13, 3}, 1000).p == fl(0), 1);
  EXPECT(rows_span({nullptr, -7, 3}, 1000).p == nullptr, 1);  // (absent: the stride is not looked at)
  EXPECT(rows_span({nullptr, -7, 3}, 1000).bytes, 0);
  // ---- strides and alignment
  EXPECT(stride_invalid(rows{fl(0), 2, 3}), 1);
  EXPECT(stride_invalid(rows{fl(0), 3, 3}), 0);
  EXPECT(stride_invalid(rows{fl(0), 3, 4}), 1);
  EXPECT(stride_invalid(rows{fl(0), INT64_MIN, 3}), 1);
  EXPECT(stride_invalid(rows{nullptr, -7, 3}), 0);
  EXPECT(stride_far(rows{fl(0), (1 << 16) + 1, 3}, 1 << 16), 1);
  EXPECT(stride_far(rows{fl(0), 1 << 16, 3}, 1 << 16), 0);
  EXPECT(stride_far(rows{nullptr, INT64_MAX, 3}, 1 << 16), 0);
  {
    const rows good[3] = {{fl(0), 10, 3}, {nullptr, 0, 4}, {fl(1), 10, 3}}, bad[3] = {{fl(0), 10, 3}, {fl(1), 3, 4}, {nullptr, 0, 3}};
    EXPECT(stride_invalid(good), 0);
    EXPECT(stride_invalid(bad), 1);
    EXPECT(stride_far(good, 10), 0);
    EXPECT(stride_far(good, 9), 1);
  }
  EXPECT(aligned(at(0), 16), 1);
  EXPECT(aligned(at(0) + 8, 16), 0);
  EXPECT(aligned(at(0) + 8, 8), 1);
  EXPECT(aligned(at(0) + 4, 8), 0);
  EXPECT(aligned(at(0) + 15, 16), 0);
  EXPECT(aligned(nullptr, 16), 1);  // (callers test for null first)
  // ---- columns of one block
  expect_apart({fl(0), 13, 3}, {fl(0, 3), 13, 3}, true);   // columns 0..2 and 3..5 of [n,13]
  expect_apart({fl(0), 10, 3}, {fl(0, 3), 10, 4}, true);   // columns 0..2, 3..6 and 7..9 of [n,10]
  expect_apart({fl(0, 3), 10, 4}, {fl(0, 7), 10, 3}, true);
  expect_apart({fl(0), 10, 3}, {fl(0, 7), 10, 3}, true);
  expect_apart({fl(0), 13, 3}, {fl(0, 2), 13, 3}, false);   // 2 floats apart: the last column of one is the first of the other
  expect_apart({fl(0), 13, 3}, {fl(0, 11), 13, 3}, false);  // stride - 2 apart: the upper one runs into the next row
  expect_apart({fl(0), 10, 3}, {fl(0, 7), 10, 4}, false);   // the same by the upper one's width: columns 7..10 of 10
  expect_apart({fl(0), 10, 4}, {fl(0, 3), 10, 3}, false);   // and by the lower one's: columns 0..3 and 3..5
  expect_apart({fl(0), 13, 3}, {fl(0, 3), 14, 3}, false);   // unequal strides
  expect_apart({fl(0), 13, 3}, {at(0) + 14, 13, 3}, false);  // 14 bytes: no whole float
  expect_apart({fl(0), 13, 3}, {fl(0), 13, 3}, false);      // the same rows
  expect_apart({fl(0), 3, 3}, {fl(0, 3), 3, 3}, false);     // contiguous rows have no room for a second set
  // ---- outputs against inputs: three outputs, four inputs, exactly one pair made to clash, each in turn
  const int64_t n = 1000;
  const size_t r3 = span_bytes(n, 3, 3);
  for (int o = -1; o < 3; ++o)
    for (int i = 0; i < 4; ++i) {
      if (o < 0 && i > 0) continue;  // (o = -1: nothing clashes)
      const span ins[4] = {{at(0), r3}, {at(1), span_bytes(n, 13, 3)}, {at(2), (size_t)n * 4}, {at(3), r3}};
      // each output in a place of its own, then output o laid on the last float of input i
      const void* p[3] = {at(4), at(5), at(6)};
      if (o >= 0) p[o] = static_cast<const char*>(ins[i].p) + ins[i].bytes - 4;
      const rows out_rows[3] = {{p[0], 3, 3}, {p[1], 4, 4}, {p[2], 13, 3}};
      const span out_spans[3] = {rows_span(out_rows[0], n), rows_span(out_rows[1], n), rows_span(out_rows[2], n)};
      EXPECT(clash(out_rows, n, ins), o >= 0);
      EXPECT(clash(out_spans, ins), o >= 0);
      // and by the output's last float on the input's first
      if (o >= 0) {
        const void* q[3] = {at(4), at(5), at(6)};
        q[o] = static_cast<const char*>(ins[i].p) - (out_spans[o].bytes - 4);
        const rows back[3] = {{q[0], 3, 3}, {q[1], 4, 4}, {q[2], 13, 3}};
        EXPECT(clash(back, n, ins), 1);
        // the clashing output absent: nothing is left
        const rows gone[3] = {{o == 0 ? nullptr : q[0], 3, 3}, {o == 1 ? nullptr : q[1], 4, 4}, {o == 2 ? nullptr : q[2], 13, 3}};
        EXPECT(clash(gone, n, ins), 0);
      }
    }
  // outputs against each other, each pair in turn: the span form refuses every overlap, the rows form all but columns of a block
  {
    const span ins[4] = {{at(0), r3}, {at(1), r3}, {nullptr, r3}, {at(3), r3}};  // (an absent input meets nothing)
    for (int a = 0; a < 3; ++a)
      for (int b = a + 1; b < 3; ++b) {
        const void* p[3] = {at(4), at(5), at(6)};
        p[b] = static_cast<const char*>(p[a]) + 12;  // 3 floats on: columns 0..2 and 3..5 where the strides allow it
        const rows block[3] = {{p[0], 10, 3}, {p[1], 10, 3}, {p[2], 10, 3}};
        rows tight[3] = {block[0], block[1], block[2]};
        tight[a].stride = tight[b].stride = 5;  // 3 + 3 columns do not fit a row of 5
        rows uneven[3] = {block[0], block[1], block[2]};
        uneven[b].stride = 11;
        EXPECT(clash(block, n, ins), 0);
        EXPECT(clash(tight, n, ins), 1);
        EXPECT(clash(uneven, n, ins), 1);
        const span spans[3] = {rows_span(block[0], n), rows_span(block[1], n), rows_span(block[2], n)};
        EXPECT(clash(spans, ins), 1);
      }
    // the three heads of a [n,10] block at once, and against tables written in place
    const rows heads[3] = {{fl(4), 10, 3}, {fl(4, 3), 10, 4}, {fl(4, 7), 10, 3}};
    EXPECT(clash(heads, n, ins), 0);
    EXPECT(clash(heads, n, {{nullptr, 0}}), 0);
    EXPECT(clash(heads, n, {{nullptr, 0}, {fl(4, 9), 8}}), 1);  // (the last column of the first row and what follows)
    EXPECT(clash({{at(5), 100}}, {{at(5) + 100, 4}, {at(5) - 4, 4}}), 0);
    EXPECT(clash({{at(5), 100}, {at(6), 100}}, {{at(5) + 100, 4}, {at(6) + 99, 4}}), 1);
    const rows wide[3] = {{fl(4), 10, 3}, {fl(4, 3), 10, 4}, {fl(4, 6), 10, 3}};  // the third on the second's last column
    EXPECT(clash(wide, n, ins), 1);
    EXPECT(clash(wide, n, {{nullptr, 0}}), 1);
  }
  return report("arg_check_unit");
}
