// The PCNet family (include/modet_hip_pcnet.h): trilinear upsampling by 2 / 4 / 8 into a slice of a wider row, DFI's gated sum, the
// NFF tail (voxel softmax + concatenation + global pooling + channel gate + rescale) and the residual sum.  All of it is memory
// traffic: fp32, channels-last, no atomics, every reduction in a fixed order.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/modet_hip_pcnet.h"

namespace {

constexpr int BLK = 256;
constexpr int UP_MAX_AXIS = 4096;           // o * (n - 1) and (i + 1) * (f n - 1) stay below 2^28
constexpr int NFF_ROWS_MAX = 1024;          // partial rows per sample

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------ upsampling by f
struct AxisSrc { int i0, i1; float t; };

// output o of an axis of n inputs and f n outputs, den = f n - 1: the cell from the integer quotient, the fraction from the remainder
__device__ __forceinline__ AxisSrc axis_src(int o, int n, int den) {
  const int num = o * (n - 1);
  const int q = num / den;
  AxisSrc a;
  a.i0 = q;
  a.i1 = q + 1 < n ? q + 1 : n - 1;
  a.t = (float)(num - q * den) / (float)den;
  return a;
}

__global__ __launch_bounds__(BLK) void up_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int d, int h, int w, int f,
                                                     int ld, int off, int64_t total) {
  const int fd = f * d, fh = f * h, fw = f * w;
  for (int64_t idx = (int64_t)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * BLK) {
    const int ox = (int)(idx % fw);
    int64_t r = idx / fw;
    const int oy = (int)(r % fh);
    r /= fh;
    const int oz = (int)(r % fd);
    const int64_t b = r / fd;
    const AxisSrc az = axis_src(oz, d, fd - 1), ay = axis_src(oy, h, fh - 1), ax = axis_src(ox, w, fw - 1);
    const float* xb = x + b * d * h * w * 3;
    const float* p00 = xb + ((int64_t)(az.i0 * h + ay.i0) * w) * 3;
    const float* p01 = xb + ((int64_t)(az.i0 * h + ay.i1) * w) * 3;
    const float* p10 = xb + ((int64_t)(az.i1 * h + ay.i0) * w) * 3;
    const float* p11 = xb + ((int64_t)(az.i1 * h + ay.i1) * w) * 3;
    const int x0 = ax.i0 * 3, x1 = ax.i1 * 3;
    const float wx1 = ax.t, wx0 = 1.f - ax.t, wy1 = ay.t, wy0 = 1.f - ay.t, wz1 = az.t, wz0 = 1.f - az.t;
    float* yp = y + idx * ld + off;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v00 = wx0 * p00[x0 + c] + wx1 * p00[x1 + c];
      const float v01 = wx0 * p01[x0 + c] + wx1 * p01[x1 + c];
      const float v10 = wx0 * p10[x0 + c] + wx1 * p10[x1 + c];
      const float v11 = wx0 * p11[x0 + c] + wx1 * p11[x1 + c];
      yp[c] = wz0 * (wy0 * v00 + wy1 * v01) + wz1 * (wy0 * v10 + wy1 * v11);
    }
  }
}

// the outputs of an axis that read input i: those whose first cell is i - 1 or i
__device__ __forceinline__ void axis_support(int i, int n, int fn, int& lo, int& cnt) {
  const int den = fn - 1, m = n - 1;
  lo = i == 0 ? 0 : ((i - 1) * den + m - 1) / m;
  int hi = ((i + 1) * den + m - 1) / m - 1;
  if (hi > fn - 1) hi = fn - 1;
  cnt = hi - lo + 1;
}

__device__ __forceinline__ float axis_weight(int o, int i, int n, int den) {
  const AxisSrc a = axis_src(o, n, den);
  float wt = 0.f;
  if (a.i0 == i) wt += 1.f - a.t;
  if (a.i1 == i) wt += a.t;
  return wt;
}

// one wave per coarse voxel: lane l sums items l, l + 64, ... of the support box (x fastest), then a butterfly over the lanes
__global__ __launch_bounds__(BLK) void up_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int d, int h, int w,
                                                     int f, int ld, int off, int64_t ncoarse) {
  const int fd = f * d, fh = f * h, fw = f * w;
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (BLK / 64);
  for (int64_t cv = (int64_t)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6); cv < ncoarse; cv += nw) {
    const int ix = (int)(cv % w);
    int64_t r = cv / w;
    const int iy = (int)(r % h);
    r /= h;
    const int iz = (int)(r % d);
    const int64_t b = r / d;
    int lz, nz, ly, ny, lx, nx;
    axis_support(iz, d, fd, lz, nz);
    axis_support(iy, h, fh, ly, ny);
    axis_support(ix, w, fw, lx, nx);
    const int n = nz * ny * nx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = lane; k < n; k += 64) {
      const int kx = k % nx, q = k / nx, ky = q % ny, kz = q / ny;
      const int oz = lz + kz, oy = ly + ky, ox = lx + kx;
      const float wt = axis_weight(oz, iz, d, fd - 1) * axis_weight(oy, iy, h, fh - 1) * axis_weight(ox, ix, w, fw - 1);
      const float* p = dy + (((b * fd + oz) * fh + oy) * fw + ox) * ld + off;
      a0 = fmaf(wt, p[0], a0);
      a1 = fmaf(wt, p[1], a1);
      a2 = fmaf(wt, p[2], a2);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) {
      dx[cv * 3 + 0] = a0;
      dx[cv * 3 + 1] = a1;
      dx[cv * 3 + 2] = a2;
    }
  }
}

int up_args(const void* a, const void* b, int B, int d, int h, int w, int f, int ld, int off) {
  MODET_CHECK_PTR(a); MODET_CHECK_PTR(b);
  MODET_CHECK_DIM(B >= 1 && d >= 2 && h >= 2 && w >= 2 && d <= UP_MAX_AXIS && h <= UP_MAX_AXIS && w <= UP_MAX_AXIS);
  if (!(f == 2 || f == 4 || f == 8) || !(ld == 3 || ld == 6 || ld == 9) || off < 0 || off + 3 > ld) return MODET_ERR_UNSUPPORTED;
  MODET_CHECK_DIM((int64_t)B * d * h * w * f * f * f * ld < ((int64_t)1 << 31));
  return MODET_OK;
}

// ------------------------------------------------------------------------------------------------ DFI's gated sum
__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

template <int NH>
__device__ __forceinline__ void dfi_fwd_voxel(const float* xs, const float* ls, float* o) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < NH; ++i) acc = fmaf(xs[3 * i + c], sigmoid_f(ls[3 * i + c]), acc);
    o[c] = acc;
  }
}

template <int NH>
__device__ __forceinline__ void dfi_bwd_voxel(const float* xs, const float* ls, const float* g, float* dxs, float* dls) {
#pragma unroll
  for (int i = 0; i < NH; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float s = sigmoid_f(ls[3 * i + c]);
      dxs[3 * i + c] = g[c] * s;
      dls[3 * i + c] = (g[c] * xs[3 * i + c]) * ((1.f - s) * s);
    }
}

template <int Q>
__device__ __forceinline__ void load4(const float* p, float* r) {
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const float4 v = reinterpret_cast<const float4*>(p)[q];
    r[4 * q] = v.x; r[4 * q + 1] = v.y; r[4 * q + 2] = v.z; r[4 * q + 3] = v.w;
  }
}
template <int Q>
__device__ __forceinline__ void store4(float* p, const float* r) {
#pragma unroll
  for (int q = 0; q < Q; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
}

// four voxels per thread: 12 NH floats of x and of logits as 3 NH 16-byte loads each; the N % 4 last voxels by block 0, scalar
template <int NH>
__global__ __launch_bounds__(BLK) void dfi_fwd_kernel(const float* __restrict__ x, const float* __restrict__ lg,
                                                      float* __restrict__ out, int64_t N) {
  constexpr int R = 3 * NH;
  const int64_t G = N >> 2;
  for (int64_t g = (int64_t)blockIdx.x * BLK + threadIdx.x; g < G; g += (int64_t)gridDim.x * BLK) {
    float xs[4 * R], ls[4 * R], o[12];
    load4<R>(x + g * 4 * R, xs);
    load4<R>(lg + g * 4 * R, ls);
#pragma unroll
    for (int v = 0; v < 4; ++v) dfi_fwd_voxel<NH>(xs + v * R, ls + v * R, o + 3 * v);
    store4<3>(out + g * 12, o);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(N & 3)) {
    const int64_t v = (G << 2) + threadIdx.x;
    float xs[R], ls[R], o[3];
#pragma unroll
    for (int q = 0; q < R; ++q) { xs[q] = x[v * R + q]; ls[q] = lg[v * R + q]; }
    dfi_fwd_voxel<NH>(xs, ls, o);
    out[v * 3] = o[0]; out[v * 3 + 1] = o[1]; out[v * 3 + 2] = o[2];
  }
}

template <int NH>
__global__ __launch_bounds__(BLK) void dfi_bwd_kernel(const float* __restrict__ x, const float* __restrict__ lg,
                                                      const float* __restrict__ dout, float* __restrict__ dx,
                                                      float* __restrict__ dlg, int64_t N) {
  constexpr int R = 3 * NH;
  const int64_t G = N >> 2;
  for (int64_t g = (int64_t)blockIdx.x * BLK + threadIdx.x; g < G; g += (int64_t)gridDim.x * BLK) {
    float xs[4 * R], ls[4 * R], go[12], dxs[4 * R], dls[4 * R];
    load4<R>(x + g * 4 * R, xs);
    load4<R>(lg + g * 4 * R, ls);
    load4<3>(dout + g * 12, go);
#pragma unroll
    for (int v = 0; v < 4; ++v) dfi_bwd_voxel<NH>(xs + v * R, ls + v * R, go + 3 * v, dxs + v * R, dls + v * R);
    store4<R>(dx + g * 4 * R, dxs);
    store4<R>(dlg + g * 4 * R, dls);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(N & 3)) {
    const int64_t v = (G << 2) + threadIdx.x;
    float xs[R], ls[R], go[3], dxs[R], dls[R];
#pragma unroll
    for (int q = 0; q < R; ++q) { xs[q] = x[v * R + q]; ls[q] = lg[v * R + q]; }
    go[0] = dout[v * 3]; go[1] = dout[v * 3 + 1]; go[2] = dout[v * 3 + 2];
    dfi_bwd_voxel<NH>(xs, ls, go, dxs, dls);
#pragma unroll
    for (int q = 0; q < R; ++q) { dx[v * R + q] = dxs[q]; dlg[v * R + q] = dls[q]; }
  }
}

// ------------------------------------------------------------------------------------------------ the NFF tail
// A voxel's row of C channels is spread over `cgp` consecutive lanes, cgp = C / 4 rounded up to a power of two (the lanes from
// C / 4 on idle): lane `sub` of a voxel owns channels 4 sub .. 4 sub + 3 of each of the three maps, one 16-byte load per map.
struct NffGeom { int cgp; int rows; int64_t chunk; };

NffGeom nff_geom(int64_t V, int C) {
  NffGeom g;
  g.cgp = 1;
  while (g.cgp < C / 4) g.cgp <<= 1;
  g.chunk = cdiv64(V, NFF_ROWS_MAX);
  if (g.chunk < 1024) g.chunk = 1024;
  g.rows = (int)cdiv64(V, g.chunk);
  return g;
}

bool nff_ok(int B, int64_t V, int C) {
  return B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31) && C >= 4 && C <= MODET_PCNET_MAX_C && C % 4 == 0;
}

__device__ __forceinline__ void softmax3(const float* __restrict__ lg, float* w) {
  const float l0 = lg[0], l1 = lg[1], l2 = lg[2];
  const float m = fmaxf(fmaxf(l0, l1), l2);
  const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
  const float s = (e0 + e1) + e2;
  w[0] = e0 / s; w[1] = e1 / s; w[2] = e2 / s;
}

// cat[k * 4 + e] = t_k[v, 4 sub + e] * w[k]: the ONE place the concatenation's values are formed
__device__ __forceinline__ void nff_cat(const float* __restrict__ t0, const float* __restrict__ t1, const float* __restrict__ t2,
                                        int64_t row, const float* w, float* t, float* cat) {
  load4<1>(t0 + row, t);
  load4<1>(t1 + row, t + 4);
  load4<1>(t2 + row, t + 8);
#pragma unroll
  for (int q = 0; q < 12; ++q) cat[q] = t[q] * w[q >> 2];
}

// stage 1 of both reductions over the voxels.  MODE 0: sum, maximum and its voxel of cat; MODE 1: sum of d_out * cat.  Workgroup
// (s, b) owns voxels [s chunk, (s + 1) chunk) of sample b and writes row s of the sample's partials.
template <int MODE>
__global__ __launch_bounds__(BLK) void nff_rows_kernel(const float* __restrict__ t0, const float* __restrict__ t1,
                                                       const float* __restrict__ t2, const float* __restrict__ lg,
                                                       const float* __restrict__ dout, double* __restrict__ psum,
                                                       float* __restrict__ pmax, int* __restrict__ parg, int64_t V, int C, int cgp,
                                                       int64_t chunk) {
  __shared__ double ls[4 * 64 * 12];
  __shared__ float lm[MODE == 0 ? 4 * 64 * 12 : 1];
  __shared__ int la[MODE == 0 ? 4 * 64 * 12 : 1];
  const int CG = C >> 2, sub = threadIdx.x & (cgp - 1), vl = threadIdx.x / cgp, vpb = BLK / cgp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.y, v0 = (int64_t)blockIdx.x * chunk, v1 = v0 + chunk < V ? v0 + chunk : V;
  const bool on = sub < CG;
  double s[12];
  float mx[12];
  int ag[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) { s[q] = 0.0; mx[q] = -INFINITY; ag[q] = INT_MAX; }
  for (int64_t vb = v0; vb < v1; vb += vpb) {
    const int64_t v = vb + vl;
    if (on && v < v1) {
      float w[3], t[12], cat[12];
      softmax3(lg + (b * V + v) * 3, w);
      nff_cat(t0, t1, t2, (b * V + v) * C + 4 * sub, w, t, cat);
      if (MODE == 0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) {
          s[q] += (double)cat[q];
          if (cat[q] > mx[q]) { mx[q] = cat[q]; ag[q] = (int)v; }
        }
      } else {
        float go[12];
        const float* gp = dout + (b * V + v) * 3 * C + 4 * sub;
        load4<1>(gp, go);
        load4<1>(gp + C, go + 4);
        load4<1>(gp + 2 * C, go + 8);
#pragma unroll
        for (int q = 0; q < 12; ++q) s[q] += (double)(go[q] * cat[q]);
      }
    }
  }
  // the lanes of a wave that own the same channels, then the four waves through LDS in wave order
  for (int o = 32; o >= cgp; o >>= 1) {
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      s[q] += __shfl_xor(s[q], o, 64);
      if (MODE == 0) {
        const float om = __shfl_xor(mx[q], o, 64);
        const int oa = __shfl_xor(ag[q], o, 64);
        if (om > mx[q] || (om == mx[q] && oa < ag[q])) { mx[q] = om; ag[q] = oa; }
      }
    }
  }
  if (lane < cgp) {
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      ls[(wave * 64 + lane) * 12 + q] = s[q];
      if (MODE == 0) { lm[(wave * 64 + lane) * 12 + q] = mx[q]; la[(wave * 64 + lane) * 12 + q] = ag[q]; }
    }
  }
  __syncthreads();
  if (threadIdx.x < cgp && on) {
    const int64_t rowbase = (b * gridDim.x + blockIdx.x) * 3 * C;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      double a = ls[sub * 12 + q];
      float m = MODE == 0 ? lm[sub * 12 + q] : 0.f;
      int g = MODE == 0 ? la[sub * 12 + q] : 0;
      for (int r = 1; r < 4; ++r) {
        a += ls[(r * 64 + sub) * 12 + q];
        if (MODE == 0) {
          const float om = lm[(r * 64 + sub) * 12 + q];
          const int oa = la[(r * 64 + sub) * 12 + q];
          if (om > m || (om == m && oa < g)) { m = om; g = oa; }
        }
      }
      const int64_t at = rowbase + (q >> 2) * C + 4 * sub + (q & 3);
      psum[at] = a;
      if (MODE == 0) { pmax[at] = m; parg[at] = g; }
    }
  }
}

// stage 2: column j of sample b over its S partial rows; the four waves take a quarter of the rows each, wave 0 adds them in order
template <int MODE>
__global__ __launch_bounds__(BLK) void nff_cols_kernel(const double* __restrict__ psum, const float* __restrict__ pmax,
                                                       const int* __restrict__ parg, float* __restrict__ avg,
                                                       float* __restrict__ mx, int* __restrict__ arg, int S, int C3, double scale) {
  __shared__ double ls[BLK];
  __shared__ float lm[BLK];
  __shared__ int la[BLK];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const int64_t b = blockIdx.y;
  const int r0 = (int)((int64_t)S * rg / 4), r1 = (int)((int64_t)S * (rg + 1) / 4);
  double a = 0.0;
  float m = -INFINITY;
  int g = INT_MAX;
  if (col < C3) {
    for (int r = r0; r < r1; ++r) {
      const int64_t at = (b * S + r) * C3 + col;
      a += psum[at];
      if (MODE == 0) {
        const float om = pmax[at];
        const int oa = parg[at];
        if (om > m || (om == m && oa < g)) { m = om; g = oa; }
      }
    }
  }
  ls[threadIdx.x] = a; lm[threadIdx.x] = m; la[threadIdx.x] = g;
  __syncthreads();
  if (rg == 0 && col < C3) {
    for (int r = 1; r < 4; ++r) {
      a += ls[r * 64 + threadIdx.x];
      const float om = lm[r * 64 + threadIdx.x];
      const int oa = la[r * 64 + threadIdx.x];
      if (MODE == 0 && (om > m || (om == m && oa < g))) { m = om; g = oa; }
    }
    avg[b * C3 + col] = (float)(a * scale);
    if (MODE == 0) { mx[b * C3 + col] = m; arg[b * C3 + col] = g; }
  }
}

// out[v, k C + ch] = cat * g: workgroups (x, b) stride over the voxels of sample b, so a thread's 12 gate values are loaded once
__global__ __launch_bounds__(BLK) void nff_apply_fwd_kernel(const float* __restrict__ t0, const float* __restrict__ t1,
                                                            const float* __restrict__ t2, const float* __restrict__ lg,
                                                            const float* __restrict__ gate, float* __restrict__ out, int64_t V,
                                                            int C, int cgp) {
  const int CG = C >> 2, sub = threadIdx.x & (cgp - 1), vl = threadIdx.x / cgp, vpb = BLK / cgp;
  const int64_t b = blockIdx.y;
  if (sub >= CG) return;                                   // no barrier and no cross-lane traffic below
  float g[12];
#pragma unroll
  for (int k = 0; k < 3; ++k) load4<1>(gate + b * 3 * C + k * C + 4 * sub, g + 4 * k);
  for (int64_t v = (int64_t)blockIdx.x * vpb + vl; v < V; v += (int64_t)gridDim.x * vpb) {
    float w[3], t[12], cat[12];
    softmax3(lg + (b * V + v) * 3, w);
    nff_cat(t0, t1, t2, (b * V + v) * C + 4 * sub, w, t, cat);
#pragma unroll
    for (int q = 0; q < 12; ++q) cat[q] *= g[q];
    float* op = out + (b * V + v) * 3 * C + 4 * sub;
    store4<1>(op, cat);
    store4<1>(op + C, cat + 4);
    store4<1>(op + 2 * C, cat + 8);
  }
}

__global__ __launch_bounds__(BLK) void nff_apply_bwd_kernel(const float* __restrict__ t0, const float* __restrict__ t1,
                                                            const float* __restrict__ t2, const float* __restrict__ lg,
                                                            const float* __restrict__ dout, const float* __restrict__ gate,
                                                            const float* __restrict__ davg, const float* __restrict__ dmx,
                                                            const int* __restrict__ arg, float* __restrict__ dt0,
                                                            float* __restrict__ dt1, float* __restrict__ dt2,
                                                            float* __restrict__ dlg, int64_t V, int C, int cgp) {
  const int CG = C >> 2, sub = threadIdx.x & (cgp - 1), vl = threadIdx.x / cgp, vpb = BLK / cgp;
  const int64_t b = blockIdx.y;
  const bool on = sub < CG;
  float g[12], da[12], dm[12];
  int ag[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) { g[q] = 0.f; da[q] = 0.f; dm[q] = 0.f; ag[q] = -1; }
  if (on) {
    const float fV = (float)V;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      const int64_t at = b * 3 * C + (q >> 2) * C + 4 * sub + (q & 3);
      g[q] = gate[at]; da[q] = davg[at] / fV; dm[q] = dmx[at]; ag[q] = arg[at];
    }
  }
  // every lane of a wave runs the same number of iterations: the butterfly over a voxel's lanes needs all of them
  for (int64_t vb = (int64_t)blockIdx.x * vpb; vb < V; vb += (int64_t)gridDim.x * vpb) {
    const int64_t v = vb + vl;
    const bool act = on && v < V;
    float w[3] = {0.f, 0.f, 0.f}, D[3] = {0.f, 0.f, 0.f};
    if (act) {
      float t[12], cat[12], go[12];
      softmax3(lg + (b * V + v) * 3, w);
      nff_cat(t0, t1, t2, (b * V + v) * C + 4 * sub, w, t, cat);
      const float* gp = dout + (b * V + v) * 3 * C + 4 * sub;
      load4<1>(gp, go);
      load4<1>(gp + C, go + 4);
      load4<1>(gp + 2 * C, go + 8);
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        const float dc = fmaf(go[q], g[q], da[q]) + ((int)v == ag[q] ? dm[q] : 0.f);
        D[q >> 2] = fmaf(dc, t[q], D[q >> 2]);
        go[q] = dc * w[q >> 2];
      }
      const int64_t row = (b * V + v) * C + 4 * sub;
      if (dt0) store4<1>(dt0 + row, go);
      if (dt1) store4<1>(dt1 + row, go + 4);
      if (dt2) store4<1>(dt2 + row, go + 8);
    }
    if (dlg) {
      for (int o = cgp >> 1; o > 0; o >>= 1) {
        D[0] += __shfl_xor(D[0], o, 64);
        D[1] += __shfl_xor(D[1], o, 64);
        D[2] += __shfl_xor(D[2], o, 64);
      }
      if (act && sub == 0) {
        const float dot = (w[0] * D[0] + w[1] * D[1]) + w[2] * D[2];
        float* lp = dlg + (b * V + v) * 3;
        lp[0] = w[0] * (D[0] - dot);
        lp[1] = w[1] * (D[1] - dot);
        lp[2] = w[2] * (D[2] - dot);
      }
    }
  }
}

// ---- the channel gate: one workgroup per sample, fp64 accumulation (3 C <= 768 inputs, R <= 96 hidden units)
constexpr int GATE_MAX_C3 = 3 * MODET_PCNET_MAX_C, GATE_MAX_R = GATE_MAX_C3 / 8;

// hidden units of both pooled vectors: pre-activations by one wave per unit, lanes over the inputs, a butterfly, then ReLU
__device__ __forceinline__ void gate_hidden(const float* __restrict__ W1, const float* a, const float* m, float* ha, float* hm,
                                            int C3, int R) {
  const int lane = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < R; r += BLK / 64) {
    double sa = 0.0, sm = 0.0;
    for (int j = lane; j < C3; j += 64) {
      const double wv = (double)W1[r * C3 + j];
      sa += wv * (double)a[j];
      sm += wv * (double)m[j];
    }
    sa = wave_sum_d(sa);
    sm = wave_sum_d(sm);
    if (lane == 0) { ha[r] = (float)sa; hm[r] = (float)sm; }          // pre-activations; the callers apply the ReLU
  }
}

__global__ __launch_bounds__(BLK) void nff_gate_fwd_kernel(const float* __restrict__ avg, const float* __restrict__ mx,
                                                           const float* __restrict__ W1, const float* __restrict__ W2,
                                                           float* __restrict__ g, int C3, int R) {
  __shared__ float a[GATE_MAX_C3], m[GATE_MAX_C3], ha[GATE_MAX_R], hm[GATE_MAX_R];
  const int64_t b = blockIdx.x;
  for (int j = threadIdx.x; j < C3; j += BLK) { a[j] = avg[b * C3 + j]; m[j] = mx[b * C3 + j]; }
  __syncthreads();
  gate_hidden(W1, a, m, ha, hm, C3, R);
  __syncthreads();
  for (int j = threadIdx.x; j < C3; j += BLK) {
    double z = 0.0;
    for (int r = 0; r < R; ++r) z += (double)W2[j * R + r] * ((double)fmaxf(ha[r], 0.f) + (double)fmaxf(hm[r], 0.f));
    g[b * C3 + j] = (float)(1.0 / (1.0 + exp(-z)));
  }
}

// per sample: d_avg, d_mx and into ws the row [dz (3 C) | relu(pa) (R) | relu(pm) (R) | d_pa (R) | d_pm (R)] for the parameter pass
__global__ __launch_bounds__(BLK) void nff_gate_bwd_kernel(const float* __restrict__ avg, const float* __restrict__ mx,
                                                           const float* __restrict__ W1, const float* __restrict__ W2,
                                                           const float* __restrict__ g, const float* __restrict__ dg,
                                                           float* __restrict__ davg, float* __restrict__ dmx,
                                                           float* __restrict__ ws, int C3, int R) {
  __shared__ float a[GATE_MAX_C3], m[GATE_MAX_C3], dz[GATE_MAX_C3], ha[GATE_MAX_R], hm[GATE_MAX_R], da[GATE_MAX_R], dm[GATE_MAX_R];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  float* row = ws + b * (C3 + 4 * R);
  for (int j = threadIdx.x; j < C3; j += BLK) {
    a[j] = avg[b * C3 + j]; m[j] = mx[b * C3 + j];
    const float gv = g[b * C3 + j];
    dz[j] = dg[b * C3 + j] * ((1.f - gv) * gv);
    row[j] = dz[j];
  }
  __syncthreads();
  gate_hidden(W1, a, m, ha, hm, C3, R);
  __syncthreads();
  for (int r = threadIdx.x >> 6; r < R; r += BLK / 64) {
    double u = 0.0;
    for (int j = lane; j < C3; j += 64) u += (double)W2[j * R + r] * (double)dz[j];
    u = wave_sum_d(u);
    if (lane == 0) {
      da[r] = ha[r] > 0.f ? (float)u : 0.f;
      dm[r] = hm[r] > 0.f ? (float)u : 0.f;
      row[C3 + r] = fmaxf(ha[r], 0.f);
      row[C3 + R + r] = fmaxf(hm[r], 0.f);
      row[C3 + 2 * R + r] = da[r];
      row[C3 + 3 * R + r] = dm[r];
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < C3; j += BLK) {
    double sa = 0.0, sm = 0.0;
    for (int r = 0; r < R; ++r) {
      const double wv = (double)W1[r * C3 + j];
      sa += wv * (double)da[r];
      sm += wv * (double)dm[r];
    }
    davg[b * C3 + j] = (float)sa;
    dmx[b * C3 + j] = (float)sm;
  }
}

// d_W1[r,j] = sum_b d_pa[b,r] avg[b,j] + d_pm[b,r] mx[b,j] and d_W2[j,r] = sum_b dz[b,j] (relu(pa) + relu(pm))[b,r], in sample order
__global__ __launch_bounds__(BLK) void nff_gate_params_kernel(const float* __restrict__ avg, const float* __restrict__ mx,
                                                              const float* __restrict__ ws, float* __restrict__ dW1,
                                                              float* __restrict__ dW2, int B, int C3, int R) {
  const int n = R * C3, stride = C3 + 4 * R;
  for (int e = blockIdx.x * BLK + threadIdx.x; e < 2 * n; e += gridDim.x * BLK) {
    double s = 0.0;
    if (e < n) {
      const int r = e / C3, j = e - r * C3;
      for (int b = 0; b < B; ++b) {
        const float* row = ws + (int64_t)b * stride;
        s += (double)row[C3 + 2 * R + r] * (double)avg[(int64_t)b * C3 + j] + (double)row[C3 + 3 * R + r] * (double)mx[(int64_t)b * C3 + j];
      }
      dW1[e] = (float)s;
    } else {
      const int f = e - n, j = f / R, r = f - j * R;
      for (int b = 0; b < B; ++b) {
        const float* row = ws + (int64_t)b * stride;
        s += (double)row[j] * ((double)row[C3 + r] + (double)row[C3 + R + r]);
      }
      dW2[f] = (float)s;
    }
  }
}

// ------------------------------------------------------------------------------------------------ the residual sum
__global__ __launch_bounds__(BLK) void add_kernel(const float* a, const float* b, float* s, int64_t n) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n4; i += (int64_t)gridDim.x * BLK) {
    const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(b)[i];
    reinterpret_cast<float4*>(s)[i] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    s[i] = a[i] + b[i];
  }
}

size_t nff_ws(int B, int64_t V, int C, int pass) {
  const NffGeom g = nff_geom(V, C);
  const size_t cells = (size_t)B * g.rows * 3 * C;
  if (pass == MODET_PCNET_NFF_PASS_POOL) return cells * 16;
  if (pass == MODET_PCNET_NFF_PASS_BWD_GATE) return cells * 8;
  if (pass == MODET_PCNET_NFF_PASS_GATE_PARAMS) return (size_t)B * (3 * C + 4 * ((3 * C) / 8)) * 4;
  return 0;
}

int nff_grid_x(int64_t V, int vpb) {
  int64_t g = cdiv64(V, vpb);
  if (g > 2048) g = 2048;
  return (int)g;
}

}  // namespace

extern "C" {

int modet_pcnet_upsample_fwd(const float* x, float* y, int B, int d, int h, int w, int f, int ld, int off, modet_stream_t stream) {
  const int rc = up_args(x, y, B, d, h, w, f, ld, off);
  if (rc != MODET_OK) return rc;
  const int64_t total = (int64_t)B * d * h * w * f * f * f;
  hipLaunchKernelGGL(up_fwd_kernel, dim3(flat_grid(total, BLK)), dim3(BLK), 0, (hipStream_t)stream, x, y, d, h, w, f, ld, off, total);
  return modet_launch_status();
}

int modet_pcnet_upsample_bwd(const float* d_y, float* d_x, int B, int d, int h, int w, int f, int ld, int off, modet_stream_t stream) {
  const int rc = up_args(d_y, d_x, B, d, h, w, f, ld, off);
  if (rc != MODET_OK) return rc;
  const int64_t ncoarse = (int64_t)B * d * h * w;
  hipLaunchKernelGGL(up_bwd_kernel, dim3(flat_grid(ncoarse * 64, BLK)), dim3(BLK), 0, (hipStream_t)stream, d_y, d_x, d, h, w, f, ld,
                     off, ncoarse);
  return modet_launch_status();
}

#define DISPATCH_DFI(KERNEL, ...)                                                                                       \
  switch (n) {                                                                                                          \
    case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(flat_grid(N / 4 + 1, BLK)), dim3(BLK), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(flat_grid(N / 4 + 1, BLK)), dim3(BLK), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(KERNEL<3>, dim3(flat_grid(N / 4 + 1, BLK)), dim3(BLK), 0, (hipStream_t)stream, __VA_ARGS__); break; \
  }

int modet_pcnet_dfi_gate_fwd(const float* x, const float* logits, float* out, int64_t N, int n, modet_stream_t stream) {
  MODET_CHECK_PTR(x); MODET_CHECK_PTR(logits); MODET_CHECK_PTR(out);
  MODET_CHECK_DIM(N >= 1 && N < ((int64_t)1 << 40));
  if (n < 1 || n > 3 || !aligned16(x) || !aligned16(logits) || !aligned16(out)) return MODET_ERR_UNSUPPORTED;
  DISPATCH_DFI(dfi_fwd_kernel, x, logits, out, N);
  return modet_launch_status();
}

int modet_pcnet_dfi_gate_bwd(const float* x, const float* logits, const float* d_out, float* d_x, float* d_logits, int64_t N, int n,
                             modet_stream_t stream) {
  MODET_CHECK_PTR(x); MODET_CHECK_PTR(logits); MODET_CHECK_PTR(d_out); MODET_CHECK_PTR(d_x); MODET_CHECK_PTR(d_logits);
  MODET_CHECK_DIM(N >= 1 && N < ((int64_t)1 << 40));
  if (n < 1 || n > 3 || !aligned16(x) || !aligned16(logits) || !aligned16(d_out) || !aligned16(d_x) || !aligned16(d_logits))
    return MODET_ERR_UNSUPPORTED;
  DISPATCH_DFI(dfi_bwd_kernel, x, logits, d_out, d_x, d_logits, N);
  return modet_launch_status();
}

size_t modet_pcnet_nff_ws_bytes(int B, int64_t V, int C, int pass) {
  if (!nff_ok(B, V, C)) return 0;
  return nff_ws(B, V, C, pass);
}

#define NFF_CHECK_WS(pass)                                                                      \
  do {                                                                                          \
    MODET_CHECK_PTR(ws);                                                                        \
    if (ws_bytes < nff_ws(B, V, C, pass) || ((uintptr_t)ws & 7) != 0) return MODET_ERR_WORKSPACE; \
  } while (0)

int modet_pcnet_nff_pool(const float* t0, const float* t1, const float* t2, const float* logits, float* avg, float* mx, int* arg,
                         void* ws, size_t ws_bytes, int B, int64_t V, int C, modet_stream_t stream) {
  MODET_CHECK_PTR(t0); MODET_CHECK_PTR(t1); MODET_CHECK_PTR(t2); MODET_CHECK_PTR(logits);
  MODET_CHECK_PTR(avg); MODET_CHECK_PTR(mx); MODET_CHECK_PTR(arg);
  MODET_CHECK_DIM(B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31));
  if (!nff_ok(B, V, C) || !aligned16(t0) || !aligned16(t1) || !aligned16(t2)) return MODET_ERR_UNSUPPORTED;
  NFF_CHECK_WS(MODET_PCNET_NFF_PASS_POOL);
  const NffGeom g = nff_geom(V, C);
  const size_t cells = (size_t)B * g.rows * 3 * C;
  double* psum = (double*)ws;
  float* pmax = (float*)(psum + cells);
  int* parg = (int*)(pmax + cells);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nff_rows_kernel<0>, dim3(g.rows, B), dim3(BLK), 0, s, t0, t1, t2, logits, (const float*)nullptr, psum, pmax,
                     parg, V, C, g.cgp, g.chunk);
  hipLaunchKernelGGL(nff_cols_kernel<0>, dim3(cdiv(3 * C, 64), B), dim3(BLK), 0, s, (const double*)psum, (const float*)pmax,
                     (const int*)parg, avg, mx, arg, g.rows, 3 * C, 1.0 / (double)V);
  return modet_launch_status();
}

int modet_pcnet_nff_gate_fwd(const float* avg, const float* mx, const float* W1, const float* W2, float* g, int B, int C,
                             modet_stream_t stream) {
  MODET_CHECK_PTR(avg); MODET_CHECK_PTR(mx); MODET_CHECK_PTR(W1); MODET_CHECK_PTR(W2); MODET_CHECK_PTR(g);
  MODET_CHECK_DIM(B >= 1 && B <= 65535);
  if (!nff_ok(B, 1, C)) return MODET_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(nff_gate_fwd_kernel, dim3(B), dim3(BLK), 0, (hipStream_t)stream, avg, mx, W1, W2, g, 3 * C, (3 * C) / 8);
  return modet_launch_status();
}

int modet_pcnet_nff_gate_bwd(const float* avg, const float* mx, const float* W1, const float* W2, const float* g, const float* d_g,
                             float* d_avg, float* d_mx, float* d_W1, float* d_W2, void* ws, size_t ws_bytes, int B, int C,
                             modet_stream_t stream) {
  MODET_CHECK_PTR(avg); MODET_CHECK_PTR(mx); MODET_CHECK_PTR(W1); MODET_CHECK_PTR(W2); MODET_CHECK_PTR(g); MODET_CHECK_PTR(d_g);
  MODET_CHECK_PTR(d_avg); MODET_CHECK_PTR(d_mx);
  if ((d_W1 == nullptr) != (d_W2 == nullptr)) return MODET_ERR_NULL;
  MODET_CHECK_DIM(B >= 1 && B <= 65535);
  if (!nff_ok(B, 1, C)) return MODET_ERR_UNSUPPORTED;
  const int64_t V = 1;
  NFF_CHECK_WS(MODET_PCNET_NFF_PASS_GATE_PARAMS);
  const int C3 = 3 * C, R = C3 / 8;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nff_gate_bwd_kernel, dim3(B), dim3(BLK), 0, s, avg, mx, W1, W2, g, d_g, d_avg, d_mx, (float*)ws, C3, R);
  if (d_W1)
    hipLaunchKernelGGL(nff_gate_params_kernel, dim3(cdiv(2 * R * C3, BLK)), dim3(BLK), 0, s, avg, mx, (const float*)ws, d_W1, d_W2,
                       B, C3, R);
  return modet_launch_status();
}

int modet_pcnet_nff_apply_fwd(const float* t0, const float* t1, const float* t2, const float* logits, const float* g, float* out,
                              int B, int64_t V, int C, modet_stream_t stream) {
  MODET_CHECK_PTR(t0); MODET_CHECK_PTR(t1); MODET_CHECK_PTR(t2); MODET_CHECK_PTR(logits); MODET_CHECK_PTR(g); MODET_CHECK_PTR(out);
  MODET_CHECK_DIM(B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31));
  if (!nff_ok(B, V, C) || !aligned16(t0) || !aligned16(t1) || !aligned16(t2) || !aligned16(g) || !aligned16(out))
    return MODET_ERR_UNSUPPORTED;
  const NffGeom gm = nff_geom(V, C);
  hipLaunchKernelGGL(nff_apply_fwd_kernel, dim3(nff_grid_x(V, BLK / gm.cgp), B), dim3(BLK), 0, (hipStream_t)stream, t0, t1, t2,
                     logits, g, out, V, C, gm.cgp);
  return modet_launch_status();
}

int modet_pcnet_nff_apply_bwd_gate(const float* t0, const float* t1, const float* t2, const float* logits, const float* d_out,
                                   float* d_g, void* ws, size_t ws_bytes, int B, int64_t V, int C, modet_stream_t stream) {
  MODET_CHECK_PTR(t0); MODET_CHECK_PTR(t1); MODET_CHECK_PTR(t2); MODET_CHECK_PTR(logits); MODET_CHECK_PTR(d_out); MODET_CHECK_PTR(d_g);
  MODET_CHECK_DIM(B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31));
  if (!nff_ok(B, V, C) || !aligned16(t0) || !aligned16(t1) || !aligned16(t2) || !aligned16(d_out)) return MODET_ERR_UNSUPPORTED;
  NFF_CHECK_WS(MODET_PCNET_NFF_PASS_BWD_GATE);
  const NffGeom g = nff_geom(V, C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nff_rows_kernel<1>, dim3(g.rows, B), dim3(BLK), 0, s, t0, t1, t2, logits, d_out, (double*)ws, (float*)nullptr,
                     (int*)nullptr, V, C, g.cgp, g.chunk);
  hipLaunchKernelGGL(nff_cols_kernel<1>, dim3(cdiv(3 * C, 64), B), dim3(BLK), 0, s, (const double*)ws, (const float*)nullptr,
                     (const int*)nullptr, d_g, (float*)nullptr, (int*)nullptr, g.rows, 3 * C, 1.0);
  return modet_launch_status();
}

int modet_pcnet_nff_apply_bwd(const float* t0, const float* t1, const float* t2, const float* logits, const float* d_out,
                              const float* g, const float* d_avg, const float* d_mx, const int* arg, float* d_t0, float* d_t1,
                              float* d_t2, float* d_logits, int B, int64_t V, int C, modet_stream_t stream) {
  MODET_CHECK_PTR(t0); MODET_CHECK_PTR(t1); MODET_CHECK_PTR(t2); MODET_CHECK_PTR(logits); MODET_CHECK_PTR(d_out); MODET_CHECK_PTR(g);
  MODET_CHECK_PTR(d_avg); MODET_CHECK_PTR(d_mx); MODET_CHECK_PTR(arg);
  if (!d_t0 && !d_t1 && !d_t2 && !d_logits) return MODET_ERR_NULL;
  MODET_CHECK_DIM(B >= 1 && B <= 65535 && V >= 1 && V < ((int64_t)1 << 31));
  if (!nff_ok(B, V, C) || !aligned16(t0) || !aligned16(t1) || !aligned16(t2) || !aligned16(d_out) || !aligned16(d_t0) ||
      !aligned16(d_t1) || !aligned16(d_t2))
    return MODET_ERR_UNSUPPORTED;
  const NffGeom gm = nff_geom(V, C);
  hipLaunchKernelGGL(nff_apply_bwd_kernel, dim3(nff_grid_x(V, BLK / gm.cgp), B), dim3(BLK), 0, (hipStream_t)stream, t0, t1, t2,
                     logits, d_out, g, d_avg, d_mx, arg, d_t0, d_t1, d_t2, d_logits, V, C, gm.cgp);
  return modet_launch_status();
}

int modet_pcnet_add(const float* a, const float* b, float* s, int64_t n, modet_stream_t stream) {
  MODET_CHECK_PTR(a); MODET_CHECK_PTR(b); MODET_CHECK_PTR(s);
  MODET_CHECK_DIM(n >= 1 && n < ((int64_t)1 << 40));
  if (!aligned16(a) || !aligned16(b) || !aligned16(s)) return MODET_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(add_kernel, dim3(flat_grid(n / 4 + 1, BLK)), dim3(BLK), 0, (hipStream_t)stream, a, b, s, n);
  return modet_launch_status();
}

}  // extern "C"
