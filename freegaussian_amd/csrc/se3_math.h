// The SE(3) exponential of the deformation net's (w, v) heads and the transform of a point, per row: the one statement that
// the fused MLP forward's epilogue (mlp.hip) and the stand-alone op (se3_apply.hip) share.
//
//   theta = |w|,  ws = w / theta + 1e-5,  vs = v / theta + 1e-5      (the offsets are constants of the function)
//   W = hat(ws),  R = I + sin(theta) W + (1 - cos theta) W^2,  G = theta I + (1 - cos theta) W + (theta - sin theta) W^2
//   T = [R | G vs],  out = R x + G vs
//
// FG_SE3_EXP is the forward in the arithmetic of utils.exp_se3 (every product and sum as that function forms it).
// fg_se3_row_bwd is the exact derivative of that function with respect to w, v and x, evaluated in forms that do not cancel
// at small theta: 1 - cos theta as 2 sin^2(theta / 2), theta - sin theta as its series below 1 rad, and the 1 / theta chain
// with the two terms of size |v| / theta that cancel taken out on paper (below).
#pragma once

// FG_SE3_EXP(hd, T): declares `float T[3][4]` in the enclosing scope, rows 0..2 of the [4,4] transform of
// hd = (w0, w1, w2, v0, v1, v2) (a `const float*`).  A macro, not a function: these are the statements mlp_se3_row held, and as
// an inlined function they compile to another register allocation in mlp.hip's inference kernels (a few lines of 3559);
// pasted, every kernel of mlp.hip stays the parent's line for line (profiles/se3_apply_fused.md (f)).
#define FG_SE3_EXP(hd, T)                                                                                        \
  const float theta = sqrtf(hd[0] * hd[0] + hd[1] * hd[1] + hd[2] * hd[2]);                                      \
  const float w0 = hd[0] / theta + 1e-5f, w1 = hd[1] / theta + 1e-5f, w2 = hd[2] / theta + 1e-5f;                \
  const float v[3] = {hd[3] / theta + 1e-5f, hd[4] / theta + 1e-5f, hd[5] / theta + 1e-5f};                      \
  const float Wm[3][3] = {{0.f, -w2, w1}, {w2, 0.f, -w0}, {-w1, w0, 0.f}};                                       \
  float W2[3][3];                                                                                                \
  for (int i = 0; i < 3; ++i)                                                                                    \
    for (int j = 0; j < 3; ++j) W2[i][j] = Wm[i][0] * Wm[0][j] + Wm[i][1] * Wm[1][j] + Wm[i][2] * Wm[2][j];      \
  float s, c;                                                                                                    \
  sincosf(theta, &s, &c);                                                                                        \
  float T[3][4];                                                                                                 \
  for (int i = 0; i < 3; ++i) {                                                                                  \
    float G[3];                                                                                                  \
    for (int j = 0; j < 3; ++j) {                                                                                \
      const float eye = i == j ? 1.f : 0.f;                                                                      \
      T[i][j] = eye + s * Wm[i][j] + (1.f - c) * W2[i][j];                                                       \
      G[j] = theta * eye + (1.f - c) * Wm[i][j] + (theta - s) * W2[i][j];                                        \
    }                                                                                                            \
    T[i][3] = G[0] * v[0] + G[1] * v[1] + G[2] * v[2];                                                           \
  }

// coordinate i of T applied to x (the homogeneous coordinate of a rigid transform is exactly 1: no divide)
#define FG_SE3_POINT(T, x, i) (T[i][0] * x[0] + T[i][1] * x[1] + T[i][2] * x[2] + T[i][3])

struct fg_vec3 {
  float x, y, z;
};
// (every function from here on rounds each product and sum on its own -- no fma contraction -- so that the backward kernel
//  built for one set of gradients gives the bits of the kernel built for another)
__device__ __forceinline__ fg_vec3 operator+(fg_vec3 a, fg_vec3 b) {
#pragma clang fp contract(off)
  return {a.x + b.x, a.y + b.y, a.z + b.z};
}
__device__ __forceinline__ fg_vec3 operator-(fg_vec3 a, fg_vec3 b) {
#pragma clang fp contract(off)
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
__device__ __forceinline__ fg_vec3 operator*(float k, fg_vec3 a) {
#pragma clang fp contract(off)
  return {k * a.x, k * a.y, k * a.z};
}
__device__ __forceinline__ float fg_dot(fg_vec3 a, fg_vec3 b) {
#pragma clang fp contract(off)
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
__device__ __forceinline__ fg_vec3 fg_cross(fg_vec3 a, fg_vec3 b) {
#pragma clang fp contract(off)
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// theta - sin theta: below 1 rad the series theta^3 / 6 (1 - t/20 (1 - t/42 (1 - t/72 (1 - t/110 (1 - t/156))))), t = theta^2
// (the first term left out is below 1e-11 of the sum); from 1 rad on the difference loses less than two bits
__device__ __forceinline__ float fg_theta_minus_sin(float theta, float s) {
#pragma clang fp contract(off)
  if (theta >= 1.f) return theta - s;
  const float t = theta * theta;
  const float poly = 1.f - t * (1.f / 20.f) * (1.f - t * (1.f / 42.f) * (1.f - t * (1.f / 72.f) * (1.f - t * (1.f / 110.f) * (1.f - t * (1.f / 156.f)))));
  return theta * t * (1.f / 6.f) * poly;
}

// The gradients of out = R x + G vs with respect to w, v, x from g = dL/dout; each is formed only where WANT_* is set.
//   A = sin theta, B = 1 - cos theta, C = theta - sin theta, q = |ws|^2, W^2 y = ws (ws . y) - q y
//   g_x  = R^T g          = g - A (ws x g) + B W^2 g
//   g_vs = G^T g          = theta g - B (ws x g) + C W^2 g,          g_v = g_vs / theta
//   g_ws = (A x + B vs) x g + B [g (ws.x) + x (g.ws) - 2 ws (g.x)] + C [g (ws.vs) + vs (g.ws) - 2 ws (g.vs)]
//   d/dtheta at fixed ws, vs:   g . [cos(theta) (ws x x) + A W^2 x + vs + A (ws x vs) + B W^2 vs]
//   g_w  = g_ws / theta + n [d/dtheta - (n . g_ws) / theta - (v . g_vs) / theta^2],   n = w / theta
// In the bracket g . vs and (v . g_vs) / theta^2 are both of size |v| |g| / theta and differ by O(1): with m = v / theta,
// g . vs - m . g = 1e-5 (g0 + g1 + g2) exactly, so the bracket is formed as
//   g . [cos(theta) (ws x x) + A W^2 x + A (ws x vs) + B W^2 vs] + 1e-5 (g0 + g1 + g2) + m . [(B/theta) (ws x g) - (C/theta) W^2 g]
//   - (n . g_ws) / theta
// where every term is of the size of the result.
template <bool WANT_W, bool WANT_V, bool WANT_X>
__device__ __forceinline__ void fg_se3_row_bwd(fg_vec3 w, fg_vec3 v, fg_vec3 x, fg_vec3 g, fg_vec3& g_w, fg_vec3& g_v, fg_vec3& g_x) {
#pragma clang fp contract(off)
  const float theta = sqrtf(fg_dot(w, w));
  const float inv = 1.f / theta;
  const fg_vec3 n = {w.x / theta, w.y / theta, w.z / theta}, m = {v.x / theta, v.y / theta, v.z / theta};
  const fg_vec3 ws = {n.x + 1e-5f, n.y + 1e-5f, n.z + 1e-5f}, vs = {m.x + 1e-5f, m.y + 1e-5f, m.z + 1e-5f};
  float s, c;
  sincosf(theta, &s, &c);
  const float h = sinf(0.5f * theta);
  const float A = s, B = 2.f * h * h, C = fg_theta_minus_sin(theta, s);
  const float q = fg_dot(ws, ws), gw_ = fg_dot(g, ws);
  const fg_vec3 wxg = fg_cross(ws, g);
  const fg_vec3 W2g = gw_ * ws - q * g;
  if (WANT_X) g_x = g - A * wxg + B * W2g;
  if (WANT_V || WANT_W) {
    // g_vs / theta
    const fg_vec3 gv = g - (B * inv) * wxg + (C * inv) * W2g;
    if (WANT_V) g_v = gv;
    if (WANT_W) {
      const float wx = fg_dot(ws, x), wv = fg_dot(ws, vs), gx = fg_dot(g, x), gvs = fg_dot(g, vs);
      const fg_vec3 u = A * x + B * vs;
      const fg_vec3 gws = fg_cross(u, g) + B * (wx * g + gw_ * x - (2.f * gx) * ws) + C * (wv * g + gw_ * vs - (2.f * gvs) * ws);
      const fg_vec3 W2x = wx * ws - q * x, W2v = wv * ws - q * vs;
      const fg_vec3 dth = c * fg_cross(ws, x) + A * (W2x + fg_cross(ws, vs)) + B * W2v;
      const float bracket = fg_dot(g, dth) + 1e-5f * (g.x + g.y + g.z) + fg_dot(m, (B * inv) * wxg - (C * inv) * W2g) - fg_dot(n, gws) * inv;
      g_w = inv * gws + bracket * n;
    }
  }
}
