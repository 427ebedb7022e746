// Stand-alone host check of the fused colour correction -- fg_color_correct_workspace_bytes, fg_color_correct's argument
// validation and fg_cc_solve (color_correct_solve.h, through fg_debug_color_correct_solve and directly) -- for a build of
// abi.hip and color_correct.hip whose HOST code carries AddressSanitizer + UndefinedBehaviorSanitizer (make
// color-correct-check).  Every fg_color_correct call below returns before a launch: the program needs no GPU and touches none.
#include <cmath>
#include <vector>

#include "../color_correct_solve.h"
#include "check_common.h"

extern "C" int fg_debug_color_correct_solve(const double* G, const double* r, double* w, int32_t* rank);

// addresses nobody reads, 16 MiB apart: img, ref, out, warps, rank, workspace
static float* at(int i) { return reinterpret_cast<float*>((uintptr_t)4096 + ((uintptr_t)i << 24)); }
static int32_t* iat(int i) { return reinterpret_cast<int32_t*>(at(i)); }

static long long want_bytes(long long P) {
  const long long blocks = (P + FG_COLOR_CORRECT_CHUNK_PIXELS - 1) / FG_COLOR_CORRECT_CHUNK_PIXELS;
  return 2048 + (blocks < FG_COLOR_CORRECT_MAX_CHUNKS ? blocks : FG_COLOR_CORRECT_MAX_CHUNKS) * 3 * 128 * 8;
}

// a small generator of its own (the program links no library for one): values in [0.05, 0.95)
static uint64_t state = 0x9E3779B97F4A7C15ull;
static double uniform() {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return 0.05 + 0.9 * (double)(state >> 11) / 9007199254740992.0;
}

// n rows a(x) of random colours (red = 0 with zero_channel) and random targets -> G = A^T A, r = A^T b
static void rows(int n, bool zero_channel, std::vector<double>& A, std::vector<double>& b, double* G, double* r) {
  A.assign((size_t)n * 10, 0.0), b.assign(n, 0.0);
  for (int p = 0; p < n; ++p) {
    const double x0 = zero_channel ? 0.0 : uniform(), x1 = uniform(), x2 = uniform();
    const double a[10] = {x0 * x0, x0 * x1, x0 * x2, x1 * x1, x1 * x2, x2 * x2, x0, x1, x2, 1.0};
    for (int i = 0; i < 10; ++i) A[(size_t)p * 10 + i] = a[i];
    b[p] = uniform();
  }
  for (int i = 0; i < 10; ++i) {
    r[i] = 0.0;
    for (int j = 0; j < 10; ++j) G[i * 10 + j] = 0.0;
    for (int p = 0; p < n; ++p) {
      r[i] += A[(size_t)p * 10 + i] * b[p];
      for (int j = 0; j < 10; ++j) G[i * 10 + j] += A[(size_t)p * 10 + i] * A[(size_t)p * 10 + j];
    }
  }
}

// the four Grams of the hook test, and 1 / 4 / 9 rows: the rank, and the normal equations A^T (A w - b) = 0 that every
// least-squares fit satisfies (relative to |A^T b|)
static void solver_cases() {
  struct { int n; bool zero; int rank; } cases[] = {{50, false, 10}, {50, true, 6}, {0, false, 0}, {1, false, 1}, {4, false, 4}, {9, false, 9}};
  for (const auto& c : cases) {
    std::vector<double> A, b;
    double G[100], r[10], w[10], w2[10];
    rows(c.n, c.zero, A, b, G, r);
    int32_t rank = -7;
    EXPECT(fg_debug_color_correct_solve(G, r, w, &rank), FG_OK);
    EXPECT(rank, c.rank);
    EXPECT(fg_cc_solve_serial(G, r, w2), c.rank);  // the header's function, compiled here: the same answer
    EXPECT(std::memcmp(w, w2, sizeof w), 0);
    double worst = 0.0, scale = 1e-300;
    for (int i = 0; i < 10; ++i) {
      double g = -r[i];
      for (int j = 0; j < 10; ++j) g += G[i * 10 + j] * w[j];
      worst = std::fmax(worst, std::fabs(g)), scale = std::fmax(scale, std::fabs(r[i]));
      EXPECT(std::isfinite(w[i]), 1);
      if (c.n == 0 || (c.zero && (i < 3 || i == 6))) EXPECT(w[i] == 0.0, 1);
    }
    EXPECT(worst <= 1e-9 * scale, 1);
  }
  double G[100] = {0}, r[10] = {0}, w[10];
  int32_t rank;
  EXPECT(fg_debug_color_correct_solve(nullptr, r, w, &rank), FG_ERR_INVALID_ARG);
  EXPECT(fg_debug_color_correct_solve(G, nullptr, w, &rank), FG_ERR_INVALID_ARG);
  EXPECT(fg_debug_color_correct_solve(G, r, nullptr, &rank), FG_ERR_INVALID_ARG);
  EXPECT(fg_debug_color_correct_solve(G, r, w, nullptr), FG_ERR_INVALID_ARG);
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  const long long MAX_P = 16384ll * 16384ll;
  const double eps = 0.5 / 255;
  // the supported range and every value around it; the query is monotone in P
  long long last = 0;
  for (long long P : {(long long)INT64_MIN, -1ll, 0ll, 1ll, 2ll, 3ll, 4ll, 4095ll, 4096ll, 4097ll, 1920ll * 1080, 4096ll * 2048, 4096ll * 2048 + 1,
                      MAX_P - 1, MAX_P, MAX_P + 1, (long long)INT64_MAX})
    for (int iters : {INT32_MIN, -1, 0, 1, 5, 8, 9, INT32_MAX}) {
      const bool ok = P >= 1 && P <= MAX_P && iters >= 1 && iters <= FG_COLOR_CORRECT_MAX_ITERS;
      const long long got = (long long)fg_color_correct_workspace_bytes(P, iters);
      EXPECT(got, ok ? want_bytes(P) : 0);
      if (ok) {
        EXPECT(got >= last, 1);
        if (iters == 8) last = got;
      } else {
        EXPECT(fg_color_correct(P, at(0), at(1), iters, eps, at(2), at(3), iat(4), at(5), BIG, nullptr), FG_ERR_UNSUPPORTED);
      }
    }
  for (double bad : {0.0, -0.25, 0.5, 1.0, (double)NAN, (double)INFINITY, -(double)INFINITY})
    EXPECT(fg_color_correct(100, at(0), at(1), 5, bad, at(2), at(3), iat(4), at(5), BIG, nullptr), FG_ERR_UNSUPPORTED);
  const int64_t P = 37 * 53;
  const size_t image = (size_t)P * 3, need = fg_color_correct_workspace_bytes(P, 5);
  char* ws = reinterpret_cast<char*>(at(5));
  // null buffers (before the range is looked at), aliasing (whole and by the last float), the workspace
  EXPECT(fg_color_correct(P, nullptr, at(1), 5, eps, at(2), at(3), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), nullptr, 5, eps, at(2), at(3), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, nullptr, at(3), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(0, nullptr, at(1), 0, eps, at(2), nullptr, nullptr, nullptr, 0, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(0), at(3), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(1), at(3), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(0) + image - 1, at(3), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(1) - image + 1, at(3), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(4), nullptr, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(4), ws + 8, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(4), at(2), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(4), reinterpret_cast<char*>(at(2)) - need + 16, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(4), at(0), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(4), at(1), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(2), iat(4), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(5), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(3), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(0), ws, BIG, nullptr), FG_ERR_INVALID_ARG);
  for (size_t bytes : {(size_t)0, (size_t)1, need - 1})
    EXPECT(fg_color_correct(P, at(0), at(1), 5, eps, at(2), at(3), iat(4), ws, bytes, nullptr), FG_ERR_WORKSPACE);
  solver_cases();
  return report("color_correct_args");
}
