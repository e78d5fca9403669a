// Trilinear resizing between any two grids, times a scalar (ATen's upsample_trilinear3d with align_corners=True, in either
// direction), and the three-level flow pyramid of a recursive RDN stage: include/modet_hip_resize.h.  Bandwidth- and launch-bound
// gathers: one thread per output voxel (forward) or input voxel (backward) and group of 1 to 4 channels, no LDS, no atomics, one
// launch per call.
// Conventions of warp.hip: 256-thread workgroups, flat grids with a grid-stride loop; here with 64-bit element offsets.
#include <math.h>

#include "common.h"
#include "../../include/modet_hip_resize.h"

namespace {

constexpr int BLK = 256;

// ------------------------------------------------------------------------------------------------ the index rule
// The ONE place that says which input cell an output index lies in, and where in it.  The forward and both backwards call it, so
// the two directions cannot disagree.  c is rounded once: the product must not be contracted into the subtraction.
struct Cell {
  int i0, i1;
  float l;
};
__device__ __forceinline__ Cell axis_cell(int p, int Si, float r) {
#pragma clang fp contract(off)
  const float c = r * (float)p;
  Cell a;
  a.i0 = min((int)c, Si - 1);
  a.i1 = min(a.i0 + 1, Si - 1);
  a.l = c - (float)a.i0;
  return a;
}

struct Grid {                 // one resize: input and output sizes, the three ratios and, for the gather's windows only, their
  int Di, Hi, Wi, Do, Ho, Wo; // inverses (0 where the ratio is 0); all computed on the host, in fp32
  float rz, ry, rx;
  float iz, iy, ix;
};

// V consecutive channels of one voxel: as one 16-byte access (VEC: V == 4, aligned) or float by float
template <int V, bool VEC>
__device__ __forceinline__ void load(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = p[k];
  }
}
template <int V, bool VEC>
__device__ __forceinline__ void store(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) p[k] = v[k];
  }
}

// scale * the 8-corner sum at output voxel (pz, py, px) for the V channels from ch, out of sample base xb
template <int V, bool VEC>
__device__ __forceinline__ void resize_point(const float* __restrict__ xb, const Grid& g, int C, int pz, int py, int px, int ch,
                                             float scale, float (&out)[V]) {
  const Cell cz = axis_cell(pz, g.Di, g.rz), cy = axis_cell(py, g.Hi, g.ry), cx = axis_cell(px, g.Wi, g.rx);
  const int64_t zo[2] = {(int64_t)cz.i0 * g.Hi, (int64_t)cz.i1 * g.Hi};
  const int yo[2] = {cy.i0, cy.i1}, xo[2] = {cx.i0, cx.i1};
  const float wz[2] = {1.f - cz.l, cz.l}, wy[2] = {1.f - cy.l, cy.l}, wx[2] = {1.f - cx.l, cx.l};
  float s[8][V];
#pragma unroll
  for (int q = 0; q < 8; ++q) {                       // issued back to back
    load<V, VEC>(xb + ((zo[q >> 2] + yo[(q >> 1) & 1]) * g.Wi + xo[q & 1]) * C + ch, s[q]);
  }
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float w = (wz[q >> 2] * wy[(q >> 1) & 1]) * wx[q & 1];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = fmaf(w, s[q][k], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) out[k] = scale * acc[k];
}

// the output indices that can name input index q along one axis: a conservative window around q / r (c = r p lies in
// [q - 1, q + 1) for them, up to rounding: one index of margin on either side); r == 0 (So == 1 or Si == 1): every output reads 0
__device__ __forceinline__ void axis_window(int q, int So, float r, float inv, int& lo, int& hi) {
  if (!(r > 0.f)) { lo = 0; hi = So - 1; return; }
  const float flo = ((float)q - 1.f) * inv - 1.f, fhi = ((float)q + 1.f) * inv + 2.f;
  lo = (int)fminf(fmaxf(flo, 0.f), 2.0e9f);
  hi = min((int)fminf(fmaxf(fhi, 0.f), 2.0e9f), So - 1);
}
// the first and the last index of that window whose cell names q (lo > hi: none).  i0 does not decrease with p, so the indices
// between them name q too; the sum below still asks each one, so that nothing rests on that.
__device__ __forceinline__ void axis_matches(int q, int Si, int So, float r, float inv, int& lo, int& hi) {
  int wl, wh;
  axis_window(q, So, r, inv, wl, wh);
  lo = wh + 1; hi = wl - 1;
  for (int p = wl; p <= wh; ++p) {
    const Cell a = axis_cell(p, Si, r);
    if (a.i0 == q || a.i1 == q) { lo = min(lo, p); hi = p; }
  }
}
// the weight input index q has in the stencil of an output whose cell is a (0 when it is neither corner; both when clamped)
__device__ __forceinline__ float axis_weight(const Cell& a, int q) {
  return (a.i0 == q ? 1.f - a.l : 0.f) + (a.i1 == q ? a.l : 0.f);
}

// scale * the transposed sum at input voxel (qz, qy, qx) for the V channels from ch, out of sample base gb of the cotangent
template <int V, bool VEC>
__device__ __forceinline__ void gather_point(const float* __restrict__ gb, const Grid& g, int C, int qz, int qy, int qx, int ch,
                                             float scale, float (&out)[V]) {
  int zl, zh, yl, yh, xl, xh;
  axis_matches(qz, g.Di, g.Do, g.rz, g.iz, zl, zh);
  axis_matches(qy, g.Hi, g.Ho, g.ry, g.iy, yl, yh);
  axis_matches(qx, g.Wi, g.Wo, g.rx, g.ix, xl, xh);
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = 0.f;
  for (int pz = zl; pz <= zh; ++pz) {
    const Cell cz = axis_cell(pz, g.Di, g.rz);
    if (cz.i0 != qz && cz.i1 != qz) continue;
    const float wz = axis_weight(cz, qz);
    for (int py = yl; py <= yh; ++py) {
      const Cell cy = axis_cell(py, g.Hi, g.ry);
      if (cy.i0 != qy && cy.i1 != qy) continue;
      const float wzy = wz * axis_weight(cy, qy);
      const float* row = gb + ((int64_t)pz * g.Ho + py) * g.Wo * C + ch;
      for (int px = xl; px <= xh; ++px) {
        const Cell cx = axis_cell(px, g.Wi, g.rx);
        if (cx.i0 != qx && cx.i1 != qx) continue;
        const float w = wzy * axis_weight(cx, qx);
        float t[V];
        load<V, VEC>(row + (int64_t)px * C, t);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(w, t[k], acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) out[k] = scale * acc[k];
}

// ------------------------------------------------------------------------------------------------ single resize
// element n of the flat (b, z, y, x, channel group) order of `S`-sized volumes -> its coordinates.  One 64-bit division finds the
// sample; inside a sample of fewer than 2^31 elements (wave-uniform: a property of the sizes) the rest is 32-bit arithmetic.
__device__ __forceinline__ void unflatten(int64_t n, int G, int Sz, int Sy, int Sx, int& grp, int& x, int& y, int& z, int64_t& b) {
  const int64_t per = (int64_t)Sz * Sy * Sx * G;
  b = n / per;
  int64_t m = n - b * per;
  if (per < 2147483648LL) {
    unsigned u = (unsigned)m;
    grp = (int)(u % (unsigned)G); u /= (unsigned)G;
    x = (int)(u % (unsigned)Sx); u /= (unsigned)Sx;
    y = (int)(u % (unsigned)Sy);
    z = (int)(u / (unsigned)Sy);
  } else {
    grp = (int)(m % G); m /= G;
    x = (int)(m % Sx); m /= Sx;
    y = (int)(m % Sy);
    z = (int)(m / Sy);
  }
}

template <int V, bool VEC>
__global__ __launch_bounds__(BLK) void resize_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, Grid g, int C,
                                                         float scale, int64_t total) {
  const int G = C / V;
  const int64_t in_sample = (int64_t)g.Di * g.Hi * g.Wi * C;
  for (int64_t n = (int64_t)blockIdx.x * BLK + threadIdx.x; n < total; n += (int64_t)gridDim.x * BLK) {
    int grp, px, py, pz;
    int64_t b;
    unflatten(n, G, g.Do, g.Ho, g.Wo, grp, px, py, pz, b);
    float v[V];
    resize_point<V, VEC>(x + b * in_sample, g, C, pz, py, px, grp * V, scale, v);
    store<V, VEC>(y + n * V, v);
  }
}

template <int V, bool VEC>
__global__ __launch_bounds__(BLK) void resize_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, Grid g, int C,
                                                         float scale, int64_t total) {
  const int G = C / V;
  const int64_t out_sample = (int64_t)g.Do * g.Ho * g.Wo * C;
  for (int64_t n = (int64_t)blockIdx.x * BLK + threadIdx.x; n < total; n += (int64_t)gridDim.x * BLK) {
    int grp, qx, qy, qz;
    int64_t b;
    unflatten(n, G, g.Di, g.Hi, g.Wi, grp, qx, qy, qz, b);
    float v[V];
    gather_point<V, VEC>(dy + b * out_sample, g, C, qz, qy, qx, grp * V, scale, v);
    store<V, VEC>(dx + n * V, v);
  }
}

// ------------------------------------------------------------------------------------------------ the flow pyramid
struct Pyramid {
  Grid g[3];                  // x -> 1/2, 1/4, 1/8
  int64_t n[3];               // voxels of each output over the batch; 0 for an output (cotangent) that is absent
};
__device__ __forceinline__ float pyramid_scale(int k) { return k == 0 ? 0.5f : (k == 1 ? 0.25f : 0.125f); }

// the voxels of the three outputs are one flat range [0, n2 + n4 + n8): a thread finds its output, then runs the single resize's
// arithmetic on the voxel's three channels (12-byte rows: float by float)
__global__ __launch_bounds__(BLK) void pyramid_fwd_kernel(const float* __restrict__ x, float* __restrict__ y2,
                                                          float* __restrict__ y4, float* __restrict__ y8, Pyramid P) {
  const int64_t total = P.n[0] + P.n[1] + P.n[2];
  const int64_t in_sample = (int64_t)P.g[0].Di * P.g[0].Hi * P.g[0].Wi * 3;
  for (int64_t n = (int64_t)blockIdx.x * BLK + threadIdx.x; n < total; n += (int64_t)gridDim.x * BLK) {
    const int k = n < P.n[0] ? 0 : (n < P.n[0] + P.n[1] ? 1 : 2);
    const int64_t m = n - (k == 0 ? 0 : (k == 1 ? P.n[0] : P.n[0] + P.n[1]));
    const Grid g = k == 0 ? P.g[0] : (k == 1 ? P.g[1] : P.g[2]);
    float* y = k == 0 ? y2 : (k == 1 ? y4 : y8);
    int grp, px, py, pz;
    int64_t b;
    unflatten(m, 1, g.Do, g.Ho, g.Wo, grp, px, py, pz, b);
    float v[3];
    resize_point<3, false>(x + b * in_sample, g, 3, pz, py, px, 0, pyramid_scale(k), v);
    store<3, false>(y + m * 3, v);
  }
}

// d_x = [d_x_add +] g2 + g4 + g8, one thread per voxel of the field; d_x_add may be d_x (read before the store, same thread)
__global__ __launch_bounds__(BLK) void pyramid_bwd_kernel(const float* __restrict__ d2, const float* __restrict__ d4,
                                                          const float* __restrict__ d8, const float* add, float* dx, Pyramid P,
                                                          int64_t total) {
  for (int64_t n = (int64_t)blockIdx.x * BLK + threadIdx.x; n < total; n += (int64_t)gridDim.x * BLK) {
#pragma clang fp contract(off)                         // the adds below are adds: never fused with a gradient's scale
    int grp, qx, qy, qz;
    int64_t b;
    unflatten(n, 1, P.g[0].Di, P.g[0].Hi, P.g[0].Wi, grp, qx, qy, qz, b);
    float r[3] = {0.f, 0.f, 0.f};
    bool have = false;
    if (add) {
      r[0] = add[n * 3]; r[1] = add[n * 3 + 1]; r[2] = add[n * 3 + 2];
      have = true;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float* d = k == 0 ? d2 : (k == 1 ? d4 : d8);
      if (!d) continue;
      const Grid& g = P.g[k];
      float v[3];
      gather_point<3, false>(d + b * ((int64_t)g.Do * g.Ho * g.Wo * 3), g, 3, qz, qy, qx, 0, pyramid_scale(k), v);
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] = have ? r[c] + v[c] : v[c];
      have = true;
    }
    dx[n * 3] = r[0]; dx[n * 3 + 1] = r[1]; dx[n * 3 + 2] = r[2];
  }
}

// ------------------------------------------------------------------------------------------------ host
inline float ratio(int Si, int So) { return So > 1 ? (float)(Si - 1) / (float)(So - 1) : 0.f; }
inline float inverse(float r) { return r > 0.f ? 1.f / r : 0.f; }
inline Grid make_grid(int Di, int Hi, int Wi, int Do, int Ho, int Wo) {
  Grid g;
  g.Di = Di; g.Hi = Hi; g.Wi = Wi; g.Do = Do; g.Ho = Ho; g.Wo = Wo;
  g.rz = ratio(Di, Do); g.ry = ratio(Hi, Ho); g.rx = ratio(Wi, Wo);
  g.iz = inverse(g.rz); g.iy = inverse(g.ry); g.ix = inverse(g.rx);
  return g;
}
inline bool resize_args_ok(int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C, float scale) {
  if (B < 1 || B > 65535 || C < 1 || C > MODET_RESIZE_MAX_C) return false;
  if (Di < 1 || Hi < 1 || Wi < 1 || Do < 1 || Ho < 1 || Wo < 1) return false;
  return scale >= -3.0e38f && scale <= 3.0e38f;                      // (NaN fails both)
}
// channels per thread: 4 as one 16-byte access where the rows allow it, else 3, 2 or 1 floats (whichever divides C)
inline int group_width(int C, const void* a, const void* b) {
  if (C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0) return 4;
  return C % 3 == 0 ? 3 : (C % 2 == 0 ? 2 : 1);
}
#define RESIZE_DISPATCH(kernel, V, nvox, ...)                                                                              \
  do {                                                                                                                     \
    const int64_t total = (nvox) * (C / (V));                                                                              \
    const dim3 grid(flat_grid(total, BLK)), block(BLK);                                                                    \
    if ((V) == 4) hipLaunchKernelGGL((kernel<4, true>), grid, block, 0, s, __VA_ARGS__, total);                           \
    else if ((V) == 3) hipLaunchKernelGGL((kernel<3, false>), grid, block, 0, s, __VA_ARGS__, total);                     \
    else if ((V) == 2) hipLaunchKernelGGL((kernel<2, false>), grid, block, 0, s, __VA_ARGS__, total);                     \
    else hipLaunchKernelGGL((kernel<1, false>), grid, block, 0, s, __VA_ARGS__, total);                                   \
  } while (0)
inline bool pyramid_args_ok(int B, int D, int H, int W) {
  return B >= 1 && B <= 65535 && D >= MODET_RESIZE_PYRAMID_MIN && H >= MODET_RESIZE_PYRAMID_MIN && W >= MODET_RESIZE_PYRAMID_MIN;
}
inline Pyramid make_pyramid(int B, int D, int H, int W, const void* p2, const void* p4, const void* p8) {
  Pyramid P;
  const void* ptr[3] = {p2, p4, p8};
  for (int k = 0; k < 3; ++k) {
    const int f = 2 << k;
    P.g[k] = make_grid(D, H, W, D / f, H / f, W / f);
    P.n[k] = ptr[k] ? (int64_t)B * (D / f) * (H / f) * (W / f) : 0;
  }
  return P;
}

}  // namespace

extern "C" {

int modet_resize_fwd(const float* x, float* y, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C, float scale,
                     modet_stream_t stream) {
  MODET_CHECK_PTR(x); MODET_CHECK_PTR(y);
  MODET_CHECK_DIM(resize_args_ok(B, Di, Hi, Wi, Do, Ho, Wo, C, scale));
  const Grid g = make_grid(Di, Hi, Wi, Do, Ho, Wo);
  hipStream_t s = (hipStream_t)stream;
  const int V = group_width(C, x, y);
  RESIZE_DISPATCH(resize_fwd_kernel, V, (int64_t)B * Do * Ho * Wo, x, y, g, C, scale);
  return modet_launch_status();
}

int modet_resize_bwd(const float* d_y, float* d_x, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C, float scale,
                     modet_stream_t stream) {
  MODET_CHECK_PTR(d_y); MODET_CHECK_PTR(d_x);
  MODET_CHECK_DIM(resize_args_ok(B, Di, Hi, Wi, Do, Ho, Wo, C, scale));
  const Grid g = make_grid(Di, Hi, Wi, Do, Ho, Wo);
  hipStream_t s = (hipStream_t)stream;
  const int V = group_width(C, d_y, d_x);
  RESIZE_DISPATCH(resize_bwd_kernel, V, (int64_t)B * Di * Hi * Wi, d_y, d_x, g, C, scale);
  return modet_launch_status();
}

int modet_resize_pyramid_fwd(const float* x, float* y2, float* y4, float* y8, int B, int D, int H, int W, modet_stream_t stream) {
  MODET_CHECK_PTR(x);
  if (!y2 && !y4 && !y8) return MODET_ERR_NULL;
  MODET_CHECK_DIM(pyramid_args_ok(B, D, H, W));
  const Pyramid P = make_pyramid(B, D, H, W, y2, y4, y8);
  const int64_t total = P.n[0] + P.n[1] + P.n[2];
  hipLaunchKernelGGL(pyramid_fwd_kernel, dim3(flat_grid(total, BLK)), dim3(BLK), 0, (hipStream_t)stream, x, y2, y4, y8, P);
  return modet_launch_status();
}

int modet_resize_pyramid_bwd(const float* d_y2, const float* d_y4, const float* d_y8, const float* d_x_add, float* d_x, int B,
                             int D, int H, int W, modet_stream_t stream) {
  MODET_CHECK_PTR(d_x);
  if (!d_y2 && !d_y4 && !d_y8) return MODET_ERR_NULL;
  MODET_CHECK_DIM(pyramid_args_ok(B, D, H, W));
  const Pyramid P = make_pyramid(B, D, H, W, d_y2, d_y4, d_y8);
  const int64_t total = (int64_t)B * D * H * W;
  hipLaunchKernelGGL(pyramid_bwd_kernel, dim3(flat_grid(total, BLK)), dim3(BLK), 0, (hipStream_t)stream, d_y2, d_y4, d_y8, d_x_add,
                     d_x, P, total);
  return modet_launch_status();
}

}  // extern "C"
