// The 10 x 10 solve of the fused colour correction (csrc/color_correct.hip), as ONE __host__ __device__ function: the
// solve kernel runs it on the device with a wave's 64 lanes as its lanes, fg_debug_color_correct_solve and
// check/color_correct_args.cpp run it on the CPU with one lane.
//
//   w = D^-1/2 pinv(S) D^-1/2 r,   S = D^-1/2 G D^-1/2 (unit diagonal),   D = diag(G)
//
// with pinv through the eigen-decomposition of S (cyclic Jacobi, float64), eigenvalues at or below FG_COLOR_CORRECT_RCOND
// times the largest dropped.  A zero diagonal entry is a zero column of the feature matrix: its row and column of S are
// zero and w_i = 0.  G = 0 gives w = 0, rank 0.  Where G has full rank this is the least-squares fit; where it has not, it
// is A least-squares fit (the one of least norm in the column-scaled variables D^1/2 w): the fitted values on the rows
// that formed G are those of every least-squares solution.
//
// The sweep visits the 45 pairs in round-robin order: nine rounds of five DISJOINT pairs (round t: (9, t) and
// ((t + i) mod 9, (t - i) mod 9), i = 1 .. 4), so the five rotations of a round commute and their 5 x 10 element updates are
// independent: lane l of a round owns pair l / 10 and index l % 10.  Every phase is a loop `for (l = lane; l < count; l +=
// nlanes)` followed by sync(): with one lane and an empty sync it is plain sequential code, with a wave's lanes and a wave-level
// fence it is the same arithmetic on the same values.  The serial row-by-row sweep this replaced took 0.6 ms per
// solve on one GPU thread (every LDS round trip on the critical path).
#pragma once
#include <math.h>

#include "../../include/fgraster.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FG_CC_HD __host__ __device__
#else
#define FG_CC_HD
#endif

#define FG_CC_N 10           // features of a pixel: the six quadratic terms, the three linear ones, 1
#define FG_CC_MAX_SWEEPS 30  // cyclic Jacobi converges quadratically: a 10 x 10 matrix takes 6 to 10 sweeps
#define FG_CC_WORK 256       // doubles of working storage: S [100], V [100], scale [10], t [10], (c, s) of a round [10]

FG_CC_HD inline void fg_cc_pair(int round, int i, int& p, int& q) {
  const int a = i == 0 ? 9 : (round + i) % 9, b = i == 0 ? round : (round - i + 9) % 9;
  p = a < b ? a : b, q = a < b ? b : a;
}

// G [10,10] row-major (read as symmetric from its upper triangle), r [10] -> w [10]; returns the number of eigenvalues kept
// (to every lane).  work: FG_CC_WORK doubles that every lane sees (the device hands in LDS).  All lanes make the call.
template <class Sync>
FG_CC_HD inline int fg_cc_solve(const double* G, const double* r, double* w, double* work, int lane, int nlanes, Sync sync) {
  const int n = FG_CC_N;
  double *S = work, *V = work + 100, *scale = work + 200, *t = work + 210, *cs = work + 220;
  for (int i = lane; i < n; i += nlanes) scale[i] = G[i * n + i] > 0.0 ? 1.0 / sqrt(G[i * n + i]) : 0.0;
  sync();
  for (int e = lane; e < n * n; e += nlanes) {
    const int i = e / n, j = e - i * n;
    S[e] = i == j ? (scale[i] > 0.0 ? 1.0 : 0.0) : G[(i < j ? i : j) * n + (i < j ? j : i)] * scale[i] * scale[j];
    V[e] = i == j ? 1.0 : 0.0;
  }
  sync();
  for (int sweep = 0; sweep < FG_CC_MAX_SWEEPS; ++sweep) {
    double off = 0.0;  // (every lane adds the same 45 values in the same order: the exit is uniform)
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) off += S[p * n + q] * S[p * n + q];
    if (off <= 1e-300) break;  // (diag(S) is at most 1: an off-diagonal below 1e-150 moves no eigenvalue)
    for (int round = 0; round < 9; ++round) {
      for (int i = lane; i < 5; i += nlanes) {  // the round's five rotations, from the matrix as the round finds it
        int p, q;
        fg_cc_pair(round, i, p, q);
        const double apq = S[p * n + q];
        double c = 1.0, sn = 0.0;
        if (apq != 0.0) {
          const double theta = (S[q * n + q] - S[p * n + p]) / (2.0 * apq);
          const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
        }
        cs[2 * i] = c, cs[2 * i + 1] = sn;
      }
      sync();
      for (int l = lane; l < 50; l += nlanes) {  // S <- S J, V <- V J: columns p, q of row k
        const int i = l / n, k = l - i * n;
        int p, q;
        fg_cc_pair(round, i, p, q);
        const double c = cs[2 * i], sn = cs[2 * i + 1];
        const double akp = S[k * n + p], akq = S[k * n + q], vkp = V[k * n + p], vkq = V[k * n + q];
        S[k * n + p] = c * akp - sn * akq, S[k * n + q] = sn * akp + c * akq;
        V[k * n + p] = c * vkp - sn * vkq, V[k * n + q] = sn * vkp + c * vkq;
      }
      sync();
      for (int l = lane; l < 50; l += nlanes) {  // S <- J^T S: rows p, q of column k; the rotated pair itself becomes 0
        const int i = l / n, k = l - i * n;
        int p, q;
        fg_cc_pair(round, i, p, q);
        const double c = cs[2 * i], sn = cs[2 * i + 1];
        const double apk = S[p * n + k], aqk = S[q * n + k];
        S[p * n + k] = k == q ? 0.0 : c * apk - sn * aqk;
        S[q * n + k] = k == p ? 0.0 : sn * apk + c * aqk;
      }
      sync();
    }
  }
  double top = 0.0;
  for (int i = 0; i < n; ++i) top = S[i * n + i] > top ? S[i * n + i] : top;
  int rank = 0;
  for (int e = 0; e < n; ++e) rank += top > 0.0 && S[e * n + e] > FG_COLOR_CORRECT_RCOND * top ? 1 : 0;
  for (int e = lane; e < n; e += nlanes) {  // t = pinv(Lambda) V^T D^-1/2 r
    double dot = 0.0;
    for (int k = 0; k < n; ++k) dot += V[k * n + e] * (scale[k] * r[k]);
    t[e] = top > 0.0 && S[e * n + e] > FG_COLOR_CORRECT_RCOND * top ? dot / S[e * n + e] : 0.0;
  }
  sync();
  for (int i = lane; i < n; i += nlanes) {
    double sum = 0.0;
    for (int e = 0; e < n; ++e) sum += V[i * n + e] * t[e];
    w[i] = scale[i] * sum;
  }
  sync();
  return rank;
}

struct fg_cc_no_sync {
  FG_CC_HD void operator()() const {}
};

// one lane: the CPU's call
inline int fg_cc_solve_serial(const double* G, const double* r, double* w) {
  double work[FG_CC_WORK];
  return fg_cc_solve(G, r, w, work, 0, 1, fg_cc_no_sync());
}
