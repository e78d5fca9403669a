// What the two stride-2 layer families share: convs2.hip (3x3x3 convolution, 27 taps, w (Cout,Cin,27), Cin 1 or a multiple of 4,
// Cout a multiple of 4) and deconv.hip (4x4x4 transposed convolution, 64 taps, w (Cin,Cout,64), any channel counts, padded to
// multiples of 4 in the workspace).  Internal like common.h, not part of the ABI.  Each family keeps its arithmetic kernels, its
// `covered`, its workspace formula and its voxel split; the float4 helpers, the weight re-layout, stage 2 of the weight gradient
// and the checks before an entry point's first launch are here, once.
//
// A family is three template parameters: T taps; PAD, whether the re-laid weights and the partial rows count channels in padded
// multiples of 4 (CiP, CoP; without PAD they are Cin, Cout and no column is a padding column); CIN_MAJOR, whether w and d_w are
// (Cin,Cout,T) or (Cout,Cin,T).
#pragma once
#include "common.h"

namespace {

constexpr int BLK = 256;

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4fma(float a, float4 b, float4 c) {
  return make_float4(fmaf(a, b.x, c.x), fmaf(a, b.y, c.y), fmaf(a, b.z, c.z), fmaf(a, b.w, c.w));
}
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// d_y split by the sign of y: gp counts with weight 1, gq with weight slope
__device__ __forceinline__ void split_pq(float g, float yv, float& gp, float& gq) {
  const bool pos = yv > 0.f;
  gp = pos ? g : 0.f;
  gq = pos ? 0.f : g;
}
__device__ __forceinline__ void split_pq4(float4 g, float4 yv, float4& gp, float4& gq) {
  split_pq(g.x, yv.x, gp.x, gq.x); split_pq(g.y, yv.y, gp.y, gq.y);
  split_pq(g.z, yv.z, gp.z, gq.z); split_pq(g.w, yv.w, gp.w, gq.w);
}
__host__ __device__ inline int pad4(int c) { return (c + 3) & ~3; }
template <bool PAD>
__host__ __device__ inline int chan(int c) { return PAD ? pad4(c) : c; }
template <int T, bool CIN_MAJOR>
__device__ __forceinline__ int64_t w_index(int tap, int ci, int co, int Cin, int Cout) {
  return (CIN_MAJOR ? (int64_t)ci * Cout + co : (int64_t)co * Cin + ci) * T + tap;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
// rows of C channels: 16-byte loads where C is a multiple of 4, scalar ones otherwise
inline bool aligned_for(const void* p, int C) { return C % 4 == 0 ? aligned16(p) : aligned4(p); }
inline int act_ok(int act, float slope) {
  if (act != 0 && act != 1) return MODET_ERR_UNSUPPORTED;
  if (act == 1 && !(slope >= 0.f)) return MODET_ERR_UNSUPPORTED;      // (a NaN slope fails the comparison too)
  return MODET_OK;
}
inline unsigned blocks_for(int64_t n) { return (unsigned)cdiv64(n, (int64_t)BLK); }

// w -> [tap][ci][co] (to_dgrad == 0) or [tap][co][ci] (to_dgrad == 1), with PAD both counts padded to CiP, CoP with zeros
template <int T, bool PAD, bool CIN_MAJOR>
__global__ __launch_bounds__(BLK) void pack_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout, int to_dgrad) {
  const int CiP = chan<PAD>(Cin), CoP = chan<PAD>(Cout);
  const int n = T * CiP * CoP;
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  int tap, ci, co;
  if (to_dgrad) {
    ci = i % CiP;
    const int r = i / CiP;
    co = r % CoP;
    tap = r / CoP;
  } else {
    co = i % CoP;
    const int r = i / CoP;
    ci = r % CiP;
    tap = r / CiP;
  }
  out[i] = (!PAD || (ci < Cin && co < Cout)) ? w[w_index<T, CIN_MAJOR>(tap, ci, co, Cin, Cout)] : 0.f;
}
template <int T, bool PAD, bool CIN_MAJOR>
inline void launch_pack(const float* w, float* out, int Cin, int Cout, int to_dgrad, hipStream_t st) {
  const int64_t n = (int64_t)T * chan<PAD>(Cin) * chan<PAD>(Cout);
  hipLaunchKernelGGL((pack_kernel<T, PAD, CIN_MAJOR>), dim3(blocks_for(n)), dim3(BLK), 0, st, w, out, Cin, Cout, to_dgrad);
}

// Stage 2 of the weight gradient.  part[(split * NQ + pq)][R], R = T CiP CoP + CoP, column (tap * CiP + ci) * CoP + co, then the
// bias; NQ = ACT ? 2 : 1.  Thread = column; the rows of all voxel splits in split order, four interleaved fp64 chains, P + slope *
// Q, one rounding
template <int T, bool PAD, bool CIN_MAJOR, bool ACT>
__global__ __launch_bounds__(BLK) void colsum_kernel(const float* __restrict__ part, int rows, int Cin, int Cout, double slope,
                                                     float* __restrict__ d_w, float* __restrict__ d_b) {
  const int CiP = chan<PAD>(Cin), CoP = chan<PAD>(Cout);
  const int64_t R = (int64_t)T * CiP * CoP + CoP;
  const int64_t c = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (c >= R) return;
  const int64_t nW = R - CoP;
  const int co = (int)(c % CoP);
  int ci = 0, tap = 0;
  if (c < nW) {
    const int64_t r = c / CoP;
    ci = (int)(r % CiP);
    tap = (int)(r / CiP);
  } else if (d_b == nullptr) {
    return;
  }
  if (PAD && (co >= Cout || ci >= Cin)) return;              // a padding column
  constexpr int NQ = ACT ? 2 : 1;
  double res[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int r = 0;
    for (; r + 3 < rows; r += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] += (double)part[((int64_t)(r + u) * NQ + q) * R + c];
    }
    for (; r < rows; ++r) a[0] += (double)part[((int64_t)r * NQ + q) * R + c];
    res[q] = (a[0] + a[1]) + (a[2] + a[3]);
  }
  const double val = ACT ? fma(slope, res[NQ - 1], res[0]) : res[0];
  if (c < nW) d_w[w_index<T, CIN_MAJOR>(tap, ci, co, Cin, Cout)] = (float)val;
  else d_b[co] = (float)val;
}
// the tail of a weight gradient: the S rows (2 S with an activation) a stage-1 launch left in part -> d_w, d_b
template <int T, bool PAD, bool CIN_MAJOR>
inline void launch_colsum(const float* part, int S, int Cin, int Cout, int act, float slope, float* d_w, float* d_b, hipStream_t st) {
  const int64_t R = (int64_t)T * chan<PAD>(Cin) * chan<PAD>(Cout) + chan<PAD>(Cout);
  if (act)
    hipLaunchKernelGGL((colsum_kernel<T, PAD, CIN_MAJOR, true>), dim3(blocks_for(R)), dim3(BLK), 0, st, part, S, Cin, Cout, (double)slope, d_w, d_b);
  else
    hipLaunchKernelGGL((colsum_kernel<T, PAD, CIN_MAJOR, false>), dim3(blocks_for(R)), dim3(BLK), 0, st, part, S, Cin, Cout, 0.0, d_w, d_b);
}

// What every entry point checks before its first launch, in the order of its error codes.  By role: `xs` has rows of Cin channels
// (x or d_x), `ys` rows of Cout channels (d_y; the forward's y), `y` is the saved output the activation's derivative reads (the
// forward passes its own y again), `w` is w or d_w, `b` the optional bias or d_b; `covered_rc` and `ws_need` are the family's own
// `covered` and `ws_bytes` of this call.
inline int check_call(const void* xs, const void* ys, const void* y, const void* w, const void* b, const void* ws, size_t ws_bytes,
                      size_t ws_need, int covered_rc, int Cin, int Cout, int act, float slope) {
  MODET_CHECK_PTR(xs); MODET_CHECK_PTR(ys); MODET_CHECK_PTR(w); MODET_CHECK_PTR(ws);
  const int rc = covered_rc == MODET_OK ? act_ok(act, slope) : covered_rc;
  if (rc != MODET_OK) return rc;
  if (act == 1) MODET_CHECK_PTR(y);
  if (!aligned_for(xs, Cin) || !aligned_for(ys, Cout) || (act == 1 && !aligned_for(y, Cout)) || !aligned4(w) || !aligned4(b))
    return MODET_ERR_UNSUPPORTED;
  if (ws_bytes < ws_need || !aligned16(ws)) return MODET_ERR_WORKSPACE;
  return MODET_OK;
}

}  // namespace
