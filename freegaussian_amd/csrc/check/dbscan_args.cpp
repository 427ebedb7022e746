// Stand-alone host check of the clustering's entry points -- fg_dbscan_workspace_bytes, fg_dbscan -- for a build of abi.hip
// and dbscan.hip whose HOST code carries AddressSanitizer + UndefinedBehaviorSanitizer (make dbscan-check).  Every call below
// returns before a launch: the program needs no GPU and touches none.
#include <cmath>

#include "check_common.h"

// addresses nobody reads, 64 MiB apart from 1 GiB on: xyz 0, labels 1, core 2, counts 3, workspace 4
static char* at(int i) { return reinterpret_cast<char*>(((uintptr_t)1 << 30) + ((uintptr_t)i << 26)); }

static int run(int64_t n, float eps, int min_samples, size_t bytes, int null_at = -1) {
  return fg_dbscan(n, null_at == 0 ? nullptr : reinterpret_cast<const float*>(at(0)), eps, min_samples,
                   null_at == 1 ? nullptr : reinterpret_cast<int32_t*>(at(1)), null_at == 2 ? nullptr : reinterpret_cast<uint8_t*>(at(2)),
                   null_at == 3 ? nullptr : reinterpret_cast<int32_t*>(at(3)), null_at == 4 ? nullptr : at(4), bytes, nullptr);
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the layout of dbscan.hip, restated: the sample, keys, order, points, cell starts, parent, root, block sums, the sort's scratch
static size_t formula(int64_t n) {
  const size_t m = (size_t)n, cells = m * 4 > 4096 ? m * 4 : 4096;
  // radix_sort.h: alternate keys and values, then 256 counters per workgroup of 256 x (8 below 3 Mi keys, else 16) keys, + 2
  const size_t tile = 256 * (size_t)(n < (3 << 20) ? 8 : 16);
  const size_t sort = 2 * align256(m * 4) + align256(((m + tile - 1) / tile + 2) * 256 * 4);
  return align256(4096 * 3 * 4) + 2 * align256(m * 4) + align256(m * 16) + align256((cells + 2) * 4) + 2 * align256(m * 4) +
         align256(((m + 255) / 256 + 1) * 4) + sort;
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  const float inf = INFINITY, nan = NAN;
  // ---- the query: 0 outside the limits, the layout inside, growing with n
  for (int64_t n : {INT64_MIN, (int64_t)-1, (int64_t)0, (int64_t)FG_DBSCAN_MAX_ROWS + 1, INT64_MAX}) EXPECT(fg_dbscan_workspace_bytes(n), 0);
  size_t before = 0;
  for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1023, (int64_t)1024, (int64_t)1025,
                    (int64_t)33000, (int64_t)240000, (int64_t)1000000, (int64_t)FG_DBSCAN_MAX_ROWS}) {
    const size_t need = fg_dbscan_workspace_bytes(n);
    EXPECT(need, formula(n));
    EXPECT(need % 256, 0);
    EXPECT(need >= before, 1);
    before = need;
  }
  const int64_t n = 1000;
  const size_t need = fg_dbscan_workspace_bytes(n);
  // everything in order but the workspace's size keeps the call on the host
  EXPECT(run(n, 0.5f, 4, 0), FG_ERR_WORKSPACE);
  EXPECT(run(n, 0.5f, 4, need - 1), FG_ERR_WORKSPACE);
  EXPECT(run(1, 0.5f, 1, 0), FG_ERR_WORKSPACE);
  EXPECT(run(FG_DBSCAN_MAX_ROWS, 0.5f, FG_DBSCAN_MAX_MIN_SAMPLES, fg_dbscan_workspace_bytes(FG_DBSCAN_MAX_ROWS) - 1), FG_ERR_WORKSPACE);
  EXPECT(run(n, FG_DBSCAN_MIN_EPS, 4, 0), FG_ERR_WORKSPACE);
  EXPECT(run(n, FG_DBSCAN_MAX_EPS, 4, 0), FG_ERR_WORKSPACE);
  // ---- rows: nothing is clamped
  for (int64_t bad : {INT64_MIN, (int64_t)-1, (int64_t)0, (int64_t)FG_DBSCAN_MAX_ROWS + 1, (int64_t)1 << 31, (int64_t)1 << 32, INT64_MAX})
    EXPECT(run(bad, 0.5f, 4, BIG), FG_ERR_INVALID_ARG);
  // ---- eps
  for (float bad : {0.f, -0.f, -1.f, -inf, inf, nan}) EXPECT(run(n, bad, 4, BIG), FG_ERR_INVALID_ARG);
  for (float bad : {1e-45f, 1e-30f, 0.99e-18f, 1.01e18f, 3e38f}) EXPECT(run(n, bad, 4, BIG), FG_ERR_UNSUPPORTED);
  // ---- min_samples
  for (int bad : {INT32_MIN, -1, 0, FG_DBSCAN_MAX_MIN_SAMPLES + 1, INT32_MAX}) EXPECT(run(n, 0.5f, bad, BIG), FG_ERR_INVALID_ARG);
  // ---- null pointers
  for (int which = 0; which < 5; ++which) EXPECT(run(n, 0.5f, 4, BIG, which), FG_ERR_INVALID_ARG);
  return report("dbscan_args");
}
