// PositionalEncodingLayer of the Im2Grid baseline = Linear(Cin -> 6) + alpha * sinusoidal embedding of the voxel's position, on
// channels-last voxels, fused (one pass over HBM).  reference: "Baseline methods/Im2Grid/models.py":238-274 (permute -> nn.Linear
// -> three aranges, three cos / sin pairs, a zero-filled (D,H,W,6) embedding, three slice assignments, repeat over the batch,
// alpha * emb, add).  Cin per level 1..5: 8, 16, 32, 64, 128; the output always has 6 channels.
//
// G lanes share one voxel (1 up to Cin = 16, then 2 / 4 / 8): lane g owns the 16-byte chunks q = g, g + G, ... of the voxel's row,
// so a wave's loads and stores of x / d_x are contiguous.  Wt and the (cos, sin) table of the shape sit in LDS; the kernels call
// no trigonometric function (the table is an argument, include/modet_hip_posenc.h).
//
// The layer is linear: d_x needs d_y and Wt only, the parameter gradients need x, d_y and the table -- two kernels, the second
// one leaves one fp32 partial row [d_W | d_bias | d_alpha] per workgroup, summed over both uses of a level by one fixed-order fp64
// column sum.
#include "common.h"
#include "../../include/modet_hip_posenc.h"

namespace {

constexpr int BLK = 256;
constexpr int DIM = MODET_POSENC_DIM;
constexpr int MAXC = 128;
constexpr int MAXT = MODET_POSENC_MAX_TABLE;

struct Shape { int D, H, W; };

__device__ __forceinline__ void stage_w(float* Ws /*[DIM][MAXC]*/, const float* __restrict__ Wt, int Cin) {
  for (int i = threadIdx.x; i < DIM * Cin; i += BLK) {
    const int j = i / Cin, c = i - j * Cin;             // Wt is (6, Cin) row-major
    Ws[j * MAXC + c] = Wt[i];
  }
}
__device__ __forceinline__ void stage_tab(float2* ts, const float* __restrict__ tab, Shape s) {
  for (int i = threadIdx.x; i < s.D + s.H + s.W; i += BLK) ts[i] = make_float2(tab[2 * i], tab[2 * i + 1]);
}
// emb[0..5] of voxel n (n < 2^31: 32-bit divisions)
__device__ __forceinline__ void embedding(const float2* ts, Shape s, unsigned n, float (&e)[DIM]) {
  const unsigned t1 = n / (unsigned)s.W, w = n - t1 * (unsigned)s.W;
  const unsigned t2 = t1 / (unsigned)s.H, h = t1 - t2 * (unsigned)s.H;
  const unsigned d = t2 % (unsigned)s.D;
  const float2 ed = ts[d], eh = ts[s.D + h], ew = ts[s.D + s.H + w];
  e[0] = ed.x; e[1] = ed.y; e[2] = eh.x; e[3] = eh.y; e[4] = ew.x; e[5] = ew.y;
}

template <int G, int CH>
__global__ __launch_bounds__(BLK) void posenc_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ Wt, const float* __restrict__ bias,
                                                         const float* __restrict__ alpha_p, const float* __restrict__ tab,
                                                         float* __restrict__ y1, float* __restrict__ y2, int64_t N, Shape s,
                                                         int Cin) {
  const float* __restrict__ x = blockIdx.y ? x2 : x1;     // gridDim.y == 2: both uses of the level in one launch
  float* __restrict__ y = blockIdx.y ? y2 : y1;
  __shared__ __attribute__((aligned(16))) float Ws[DIM * MAXC];
  __shared__ float2 ts[MAXT];
  stage_w(Ws, Wt, Cin);
  stage_tab(ts, tab, s);
  __syncthreads();
  constexpr int VPB = BLK / G;
  const int v = threadIdx.x / G, g = threadIdx.x % G, Q = Cin >> 2;
  const float alpha = alpha_p[0];
  float b[DIM];
#pragma unroll
  for (int j = 0; j < DIM; ++j) b[j] = bias[j];
  const int64_t ntiles = cdiv64(N, (int64_t)VPB);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t n = t * VPB + v;
    const bool ok = n < N;
    float4 xv[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int q = g + i * G;
      xv[i] = (ok && q < Q) ? *reinterpret_cast<const float4*>(x + n * Cin + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float z[DIM];
#pragma unroll
    for (int j = 0; j < DIM; ++j) z[j] = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int q = g + i * G;
      if (q < Q) {
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          const float4 w4 = *reinterpret_cast<const float4*>(Ws + j * MAXC + 4 * q);
          z[j] = fmaf(xv[i].x, w4.x, z[j]);
          z[j] = fmaf(xv[i].y, w4.y, z[j]);
          z[j] = fmaf(xv[i].z, w4.z, z[j]);
          z[j] = fmaf(xv[i].w, w4.w, z[j]);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < G; o <<= 1)
#pragma unroll
      for (int j = 0; j < DIM; ++j) z[j] += __shfl_xor(z[j], o, 64);
    if (ok && g == 0) {
      float e[DIM];
      embedding(ts, s, (unsigned)n, e);
      float* yp = y + n * DIM;
#pragma unroll
      for (int j = 0; j < DIM; j += 2)
        *reinterpret_cast<float2*>(yp + j) = make_float2(fmaf(alpha, e[j], z[j] + b[j]), fmaf(alpha, e[j + 1], z[j + 1] + b[j + 1]));
    }
  }
}

template <int G, int CH>
__global__ __launch_bounds__(BLK) void posenc_bwd_data_kernel(const float* __restrict__ dy1, const float* __restrict__ dy2,
                                                              const float* __restrict__ Wt, float* __restrict__ dx1,
                                                              float* __restrict__ dx2, int64_t N, int Cin, int second_only) {
  const bool u2 = blockIdx.y || second_only;
  const float* __restrict__ dy = u2 ? dy2 : dy1;
  float* __restrict__ dx = u2 ? dx2 : dx1;
  __shared__ __attribute__((aligned(16))) float Ws[DIM * MAXC];
  stage_w(Ws, Wt, Cin);
  __syncthreads();
  constexpr int VPB = BLK / G;
  const int v = threadIdx.x / G, g = threadIdx.x % G, Q = Cin >> 2;
  const int64_t ntiles = cdiv64(N, (int64_t)VPB);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t n = t * VPB + v;
    if (n >= N) continue;
    float gy[DIM];
#pragma unroll
    for (int j = 0; j < DIM; j += 2) {
      const float2 p = *reinterpret_cast<const float2*>(dy + n * DIM + j);
      gy[j] = p.x; gy[j + 1] = p.y;
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int q = g + i * G;
      if (q < Q) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          const float4 w4 = *reinterpret_cast<const float4*>(Ws + j * MAXC + 4 * q);
          a.x = fmaf(gy[j], w4.x, a.x); a.y = fmaf(gy[j], w4.y, a.y); a.z = fmaf(gy[j], w4.z, a.z); a.w = fmaf(gy[j], w4.w, a.w);
        }
        *reinterpret_cast<float4*>(dx + n * Cin + 4 * q) = a;
      }
    }
  }
}

// one partial row per workgroup: part[(blockIdx.y * gridDim.x + blockIdx.x)][6 * Cin + 7] = [d_W (6, Cin) | d_bias (6) | d_alpha]
template <int G, int CH>
__global__ __launch_bounds__(BLK) void posenc_bwd_params_kernel(const float* __restrict__ x1, const float* __restrict__ dy1,
                                                                const float* __restrict__ x2, const float* __restrict__ dy2,
                                                                const float* __restrict__ tab, float* __restrict__ part,
                                                                int64_t N, Shape s, int Cin) {
  const float* __restrict__ x = blockIdx.y ? x2 : x1;
  const float* __restrict__ dy = blockIdx.y ? dy2 : dy1;
  const int R = DIM * Cin + DIM + 1;
  __shared__ float2 ts[MAXT];
  __shared__ float red[(BLK / 64) * (DIM * MAXC + DIM + 1)];
  stage_tab(ts, tab, s);
  __syncthreads();
  constexpr int VPB = BLK / G;
  const int v = threadIdx.x / G, g = threadIdx.x % G, Q = Cin >> 2;
  float4 aw[CH][DIM];
  float ab[DIM], aa = 0.f;
#pragma unroll
  for (int j = 0; j < DIM; ++j) {
    ab[j] = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) aw[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int64_t ntiles = cdiv64(N, (int64_t)VPB);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t n = t * VPB + v;
    if (n >= N) continue;
    float4 xv[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int q = g + i * G;
      xv[i] = q < Q ? *reinterpret_cast<const float4*>(x + n * Cin + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float gy[DIM];
#pragma unroll
    for (int j = 0; j < DIM; j += 2) {
      const float2 p = *reinterpret_cast<const float2*>(dy + n * DIM + j);
      gy[j] = p.x; gy[j + 1] = p.y;
    }
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
      for (int j = 0; j < DIM; ++j) {
        aw[i][j].x = fmaf(gy[j], xv[i].x, aw[i][j].x); aw[i][j].y = fmaf(gy[j], xv[i].y, aw[i][j].y);
        aw[i][j].z = fmaf(gy[j], xv[i].z, aw[i][j].z); aw[i][j].w = fmaf(gy[j], xv[i].w, aw[i][j].w);
      }
    if (g == 0) {               // the voxel's d_y counts once, not once per lane of its group
      float e[DIM];
      embedding(ts, s, (unsigned)n, e);
#pragma unroll
      for (int j = 0; j < DIM; ++j) { ab[j] += gy[j]; aa = fmaf(gy[j], e[j], aa); }
    }
  }
  // lanes with the same g hold partial sums of the same columns: xor-shuffles over the lane bits above the group
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* rw = red + wave * (DIM * MAXC + DIM + 1);
#pragma unroll
  for (int i = 0; i < CH; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) {
      float4 a = aw[i][j];
#pragma unroll
      for (int o = G; o < 64; o <<= 1) {
        a.x += __shfl_xor(a.x, o, 64); a.y += __shfl_xor(a.y, o, 64); a.z += __shfl_xor(a.z, o, 64); a.w += __shfl_xor(a.w, o, 64);
      }
      const int q = lane + i * G;
      if (lane < G && q < Q) {
        float* p = rw + j * Cin + 4 * q;
        p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
      }
    }
#pragma unroll
  for (int j = 0; j < DIM; ++j) {
    const float r = wave_sum(ab[j]);
    if (lane == 0) rw[DIM * Cin + j] = r;
  }
  {
    const float r = wave_sum(aa);
    if (lane == 0) rw[DIM * Cin + DIM] = r;
  }
  __syncthreads();
  float* prow = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * R;
  constexpr int RS = DIM * MAXC + DIM + 1;
  for (int i = threadIdx.x; i < R; i += BLK) prow[i] = ((red[i] + red[RS + i]) + red[2 * RS + i]) + red[3 * RS + i];
}

// column sums of the partial rows, one wave per column, fixed lane assignment + fixed tree, fp64 (as proj_ln.hip's colsum_kernel)
__global__ __launch_bounds__(64) void posenc_colsum_kernel(const float* __restrict__ part, int rows, int R, float* __restrict__ d_Wt,
                                                           int nW, float* __restrict__ d_bias, float* __restrict__ d_alpha) {
  const int i = blockIdx.x;
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
  int r = threadIdx.x;
  for (; r + 192 < rows; r += 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s4[u] += (double)part[(int64_t)(r + 64 * u) * R + i];
  }
  for (; r < rows; r += 64) s4[0] += (double)part[(int64_t)r * R + i];
  double sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  sum = wave_sum_d(sum);
  if (threadIdx.x != 0) return;
  if (i < nW) d_Wt[i] = (float)sum;
  else if (i < nW + DIM) d_bias[i - nW] = (float)sum;
  else d_alpha[0] = (float)sum;
}

inline int group_of(int Cin) { return Cin <= 16 ? 1 : Cin <= 32 ? 2 : Cin <= 64 ? 4 : 8; }
inline int tile_grid(int64_t N, int G, int cap) {
  const int64_t tiles = cdiv64(N, (int64_t)(BLK / G));
  return (int)(tiles < cap ? tiles : cap);
}
constexpr int STREAM_GRID = 256 * 8;       // 256 CUs x 8 workgroups of 4 waves
constexpr int PARAM_GRID = 256 * 4;        // the parameter kernel carries up to 103 accumulators per lane: fewer, longer workgroups

// MODET_OK when the kernels cover the shape
inline int covered(int B, int D, int H, int W, int Cin, int dim) {
  if (B < 1 || D < 2 || H < 2 || W < 2) return MODET_ERR_DIM;
  if ((int64_t)B * D * H * W >= ((int64_t)1 << 31)) return MODET_ERR_DIM;
  if (dim != DIM || Cin < 4 || Cin % 4 != 0 || Cin > MAXC) return MODET_ERR_UNSUPPORTED;
  if ((int64_t)D + H + W > MAXT) return MODET_ERR_UNSUPPORTED;
  return MODET_OK;
}

#define POSENC_DISPATCH(KERNEL, Cin, ...)                                             \
  do {                                                                                \
    if ((Cin) <= 8) KERNEL(1, 2, __VA_ARGS__);                                        \
    else if ((Cin) <= 16) KERNEL(1, 4, __VA_ARGS__);                                  \
    else if ((Cin) <= 32) KERNEL(2, 4, __VA_ARGS__);                                  \
    else if ((Cin) <= 64) KERNEL(4, 4, __VA_ARGS__);                                  \
    else KERNEL(8, 4, __VA_ARGS__);                                                   \
  } while (0)

}  // namespace

extern "C" {

size_t modet_posenc_ws_bytes(int B, int D, int H, int W, int Cin, int dim) {
  if (covered(B, D, H, W, Cin, dim) != MODET_OK) return 0;
  const int64_t N = (int64_t)B * D * H * W;
  return (size_t)2 * tile_grid(N, group_of(Cin), PARAM_GRID) * (DIM * Cin + DIM + 1) * sizeof(float);
}

int modet_posenc_fwd_pair(const float* x1, const float* x2, const float* Wt, const float* bias, const float* alpha,
                          const float* tab, float* y1, float* y2, int B, int D, int H, int W, int Cin, int dim,
                          modet_stream_t stream) {
  MODET_CHECK_PTR(x1); MODET_CHECK_PTR(Wt); MODET_CHECK_PTR(bias); MODET_CHECK_PTR(alpha); MODET_CHECK_PTR(tab); MODET_CHECK_PTR(y1);
  if ((x2 == nullptr) != (y2 == nullptr)) return MODET_ERR_NULL;
  const int rc = covered(B, D, H, W, Cin, dim);
  if (rc != MODET_OK) return rc;
  const int64_t N = (int64_t)B * D * H * W;
  const int G = group_of(Cin);
  const dim3 grid(tile_grid(N, G, STREAM_GRID), x2 ? 2 : 1);
  const Shape s{D, H, W};
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_FWD(G_, CH_, ...) hipLaunchKernelGGL((posenc_fwd_kernel<G_, CH_>), grid, dim3(BLK), 0, st, __VA_ARGS__)
  POSENC_DISPATCH(LAUNCH_FWD, Cin, x1, x2, Wt, bias, alpha, tab, y1, y2, N, s, Cin);
#undef LAUNCH_FWD
  return modet_launch_status();
}

int modet_posenc_bwd_data_pair(const float* d_y1, const float* d_y2, const float* Wt, float* d_x1, float* d_x2, int B, int D,
                               int H, int W, int Cin, int dim, modet_stream_t stream) {
  MODET_CHECK_PTR(Wt);
  if (d_x1 == nullptr && d_x2 == nullptr) return MODET_ERR_NULL;
  if (d_x1) MODET_CHECK_PTR(d_y1);
  if (d_x2) MODET_CHECK_PTR(d_y2);
  const int rc = covered(B, D, H, W, Cin, dim);
  if (rc != MODET_OK) return rc;
  const int64_t N = (int64_t)B * D * H * W;
  const int G = group_of(Cin);
  const dim3 grid(tile_grid(N, G, STREAM_GRID), (d_x1 && d_x2) ? 2 : 1);
  const int second_only = d_x1 == nullptr;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_BD(G_, CH_, ...) hipLaunchKernelGGL((posenc_bwd_data_kernel<G_, CH_>), grid, dim3(BLK), 0, st, __VA_ARGS__)
  POSENC_DISPATCH(LAUNCH_BD, Cin, d_y1, d_y2, Wt, d_x1, d_x2, N, Cin, second_only);
#undef LAUNCH_BD
  return modet_launch_status();
}

int modet_posenc_bwd_params_pair(const float* x1, const float* d_y1, const float* x2, const float* d_y2, const float* tab,
                                 float* d_Wt, float* d_bias, float* d_alpha, void* ws, size_t ws_bytes, int B, int D, int H,
                                 int W, int Cin, int dim, modet_stream_t stream) {
  MODET_CHECK_PTR(x1); MODET_CHECK_PTR(d_y1); MODET_CHECK_PTR(tab); MODET_CHECK_PTR(d_Wt); MODET_CHECK_PTR(d_bias);
  MODET_CHECK_PTR(d_alpha); MODET_CHECK_PTR(ws);
  if ((x2 == nullptr) != (d_y2 == nullptr)) return MODET_ERR_NULL;
  const int rc = covered(B, D, H, W, Cin, dim);
  if (rc != MODET_OK) return rc;
  if (ws_bytes < modet_posenc_ws_bytes(B, D, H, W, Cin, dim) || ((uintptr_t)ws & 15) != 0) return MODET_ERR_WORKSPACE;
  const int64_t N = (int64_t)B * D * H * W;
  const int G = group_of(Cin), gx = tile_grid(N, G, PARAM_GRID), uses = x2 ? 2 : 1, R = DIM * Cin + DIM + 1;
  const dim3 grid(gx, uses);
  const Shape s{D, H, W};
  float* part = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
#define LAUNCH_BP(G_, CH_, ...) hipLaunchKernelGGL((posenc_bwd_params_kernel<G_, CH_>), grid, dim3(BLK), 0, st, __VA_ARGS__)
  POSENC_DISPATCH(LAUNCH_BP, Cin, x1, d_y1, x2, d_y2, tab, part, N, s, Cin);
#undef LAUNCH_BP
  hipLaunchKernelGGL(posenc_colsum_kernel, dim3(R), dim3(64), 0, st, (const float*)part, uses * gx, R, d_Wt, DIM * Cin, d_bias,
                     d_alpha);
  return modet_launch_status();
}

}  // extern "C"
