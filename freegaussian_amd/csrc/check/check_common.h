// What the stand-alone host check programs of this directory share: the EXPECT count, addresses and sizes that pass every
// check but are never used (each call returns before a launch), the final report, and the fused MLP's two structs filled in.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../../include/fgraster.h"

static int failures = 0;
#define EXPECT(what, want)                                                        \
  do {                                                                            \
    const long long got_ = (long long)(what), want_ = (long long)(want);          \
    if (got_ != want_) {                                                          \
      std::printf("%s:%d: %s = %lld, want %lld\n", __FILE__, __LINE__, #what, got_, want_); \
      ++failures;                                                                 \
    }                                                                             \
  } while (0)

static float* const PTR = reinterpret_cast<float*>(4096);  // an address nobody reads
static const size_t BIG = (size_t)1 << 40;

// the program's last line and its exit status
static int report(const char* name) {
  if (failures) std::printf("%s: %d FAILED\n", name, failures);
  else std::printf("%s: ok\n", name);
  return failures ? 1 : 0;
}

static fg_mlp_desc desc(int aux_width = 21, int32_t precision = FG_MLP_FP32) {
  fg_mlp_desc d;
  std::memset(&d, 0, sizeof d);
  d.size = (int32_t)sizeof d, d.mode = FG_MLP_PLAIN, d.depth = 8, d.width = 256, d.multires = 10, d.aux_width = aux_width;
  d.n_heads = 4, d.precision = precision;
  const int rows[4] = {3, 3, 4, 3};
  for (int h = 0; h < 4; ++h) d.head_rows[h] = rows[h], d.head_weight[h] = PTR, d.head_bias[h] = PTR;
  for (int l = 0; l < 8; ++l) d.weight[l] = PTR, d.bias[l] = PTR;
  return d;
}

static fg_mlp_grads grads(bool all) {
  fg_mlp_grads g;
  std::memset(&g, 0, sizeof g);
  g.size = (int32_t)sizeof g;
  if (all) {
    for (int l = 0; l < 8; ++l) g.weight[l] = PTR, g.bias[l] = PTR;
    for (int h = 0; h < 4; ++h) g.head_weight[h] = PTR, g.head_bias[h] = PTR;
  }
  return g;
}
