// SSIM3D forward + gradient (reference Baseline methods/RCN/losses.py:9-27, 53-74, 103-148; include/modet_hip_ssim.h has the
// definition).
//
// The reference evaluates five dense 11x11x11 conv3d (1331 taps each).  The Gaussian window is an outer product of its 1-D
// taps, so here every filter is three 1-D passes of w taps and nothing of the w^3 window is formed.  One z-marching kernel
// (ssim_march_kernel, the shape of ncc_march_kernel in losses.hip) does a whole direction: a workgroup owns a 16 x 32 (y, x)
// tile and walks z.  Each incoming plane's halo tile (16 + 2p) x (32 + 2p) goes into LDS once, the x filter and then the y
// filter run over two LDS arrays, and every thread keeps the last w (x, y)-filtered planes of its two owned voxels in
// REGISTERS (five fields x 11 planes = 55 per owned voxel), so the z filter is register arithmetic with no halo of its own;
// the pointwise tail finishes the plane.  Planes outside the volume are zero after any filter, so they enter the ring as zeros
// without any work.
//   FWD: reads a, b -> the five fields {G a, G b, G a^2, G b^2, G ab} -> ssim (loss partial per workgroup, fp64) and the
//        coefficient volumes d ssim / d field: c_sq (the same for G a^2 and G b^2), c_x (G ab), c_m1, c_m2 as wanted.
//   BWD: reads three coefficient volumes -> G c_m, G c_sq, G c_x -> d = g (G c_m + 2 self G c_sq + other G c_x), g = -scale / N
//        (the zero-padded symmetric filter is its own adjoint).  One launch per wanted gradient.
// The taps are symmetric: every pass adds the pair and multiplies once, outermost (smallest) taps first.
// The scalar is reduced in two fixed-order stages (fp64 workgroup partials -> one fp64 sum); no atomics, no memset.
#include <math.h>

#include "common.h"
#include "../../include/modet_hip_ssim.h"

namespace {

constexpr int BLK = 256;
constexpr int MT_Y = 16, MT_X = 32;
constexpr int RPT = MT_Y * MT_X / BLK;             // owned voxels per thread: column x, RPT consecutive rows
constexpr int MAX_WIN = 11;

struct Dims { int B, D, H, W; };
struct Taps { float t[MAX_WIN / 2 + 1]; };         // t[j] = tap j = tap w - 1 - j, j = 0 .. p

// NOUT consecutive outputs of the symmetric W_-tap filter over v[0 .. NOUT + W_ - 2]
template <int W_, int NOUT>
__device__ __forceinline__ void filt(const float (&v)[NOUT + W_ - 1], const Taps& t, float (&o)[NOUT]) {
  constexpr int P = W_ / 2;
#pragma unroll
  for (int m = 0; m < NOUT; ++m) {
    if constexpr (P == 0) {
      o[m] = t.t[0] * v[m];
    } else {
      float acc = t.t[0] * (v[m] + v[m + W_ - 1]);
#pragma unroll
      for (int j = 1; j < P; ++j) acc = fmaf(t.t[j], v[m + j] + v[m + W_ - 1 - j], acc);
      o[m] = fmaf(t.t[P], v[m + P], acc);
    }
  }
}

template <int W_, bool FWD>
__global__ __launch_bounds__(BLK, 2) void ssim_march_kernel(const float* __restrict__ in0, const float* __restrict__ in1,
                                                            const float* __restrict__ in2, const float* __restrict__ self,
                                                            const float* __restrict__ other, float* __restrict__ out0,
                                                            float* __restrict__ out1, float* __restrict__ out2,
                                                            float* __restrict__ out3, double* __restrict__ part, Dims d,
                                                            int tiles_x, int tiles_y, int nchunk, int zc, float g, Taps taps) {
  constexpr int P = W_ / 2, HY = MT_Y + 2 * P, HXW = MT_X + 2 * P, NVOX = HY * HXW;
  constexpr int NIN = FWD ? 2 : 3, NF = FWD ? 5 : 3;             // inputs; filtered fields
  constexpr int NV = (NVOX + BLK - 1) / BLK;                     // halo voxels per thread
  static_assert(HY <= BLK / 8, "the x pass gives every halo row eight threads");
  __shared__ float hs[NIN][NVOX + 1];                            // the incoming plane's halo tile (+ a dummy slot)
  __shared__ __attribute__((aligned(16))) float tw[NF][HY * MT_X];      // after the x pass
  __shared__ double red[BLK / 64];
  const int tid = threadIdx.x;
  int t = blockIdx.x;
  const int x0 = (t % tiles_x) * MT_X; t /= tiles_x;
  const int y0 = (t % tiles_y) * MT_Y; t /= tiles_y;
  const int zs0 = (t % nchunk) * zc;
  const int b = t / nchunk;
  const int ze = zs0 + zc < d.D ? zs0 + zc : d.D;
  const int64_t plane = (int64_t)d.H * d.W;
  const int64_t vol = (int64_t)b * d.D * plane;
  const float* src[NIN];
  src[0] = in0 + vol; src[1] = in1 + vol;
  if constexpr (!FWD) src[2] = in2 + vol;

  // this thread's halo voxels: offset inside a plane (-1 = zero padding or past the halo tile) and LDS slot
  int goff[NV], lidx[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = tid + j * BLK;
    const int hy = i / HXW, hx = i - hy * HXW;
    const int y = y0 + hy - P, x = x0 + hx - P;
    const bool ok = i < NVOX && y >= 0 && y < d.H && x >= 0 && x < d.W;
    goff[j] = ok ? y * d.W + x : -1;
    lidx[j] = i < NVOX ? i : NVOX;
  }
  float nxt[NIN][NV];
  auto load_plane = [&](int z) {
    const bool zin = z >= 0 && z < d.D;
#pragma unroll
    for (int v = 0; v < NIN; ++v) {
      const float* p = src[v] + (int64_t)(zin ? z : 0) * plane;
#pragma unroll
      for (int j = 0; j < NV; ++j) nxt[v][j] = (zin && goff[j] >= 0) ? p[goff[j]] : 0.f;
    }
  };

  // the last W_ (x, y)-filtered planes of the owned voxels, oldest first: ring[f][m][k] is plane z - P + k of output plane z
  float ring[NF][RPT][W_];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int m = 0; m < RPT; ++m)
#pragma unroll
      for (int k = 0; k < W_; ++k) ring[f][m][k] = 0.f;

  const int xo = tid & (MT_X - 1), r0 = (tid / MT_X) * RPT;      // the owned column and its first row
  double lsum = 0.0;
  const int zlast = ze - 1 + P;
  load_plane(zs0 - P);
  for (int zp = zs0 - P; zp <= zlast; ++zp) {
    const bool zin = zp >= 0 && zp < d.D;                        // (workgroup-uniform)
    float nf[NF][RPT];
    if (zin) {
#pragma unroll
      for (int v = 0; v < NIN; ++v)
#pragma unroll
        for (int j = 0; j < NV; ++j) hs[v][lidx[j]] = nxt[v][j];
    }
    if (zp < zlast) load_plane(zp + 1);                          // in flight during this plane's arithmetic
    if (zin) {
      __syncthreads();
      // ---- x pass: (halo row r, 4 consecutive outputs) from a register window of 4 + W_ - 1 values
      {
        const int r = tid >> 3, c0 = (tid & 7) * 4;
        if (r < HY) {
          float va[4 + W_ - 1], vb[4 + W_ - 1], vq[4 + W_ - 1], o[4];
#pragma unroll
          for (int k = 0; k < 4 + W_ - 1; ++k) { va[k] = hs[0][r * HXW + c0 + k]; vb[k] = hs[1][r * HXW + c0 + k]; }
          auto put = [&](int f) { *reinterpret_cast<float4*>(&tw[f][r * MT_X + c0]) = make_float4(o[0], o[1], o[2], o[3]); };
          filt<W_, 4>(va, taps, o); put(0);
          filt<W_, 4>(vb, taps, o); put(1);
          if constexpr (FWD) {
#pragma unroll
            for (int k = 0; k < 4 + W_ - 1; ++k) vq[k] = va[k] * va[k];
            filt<W_, 4>(vq, taps, o); put(2);
#pragma unroll
            for (int k = 0; k < 4 + W_ - 1; ++k) vq[k] = vb[k] * vb[k];
            filt<W_, 4>(vq, taps, o); put(3);
#pragma unroll
            for (int k = 0; k < 4 + W_ - 1; ++k) vq[k] = va[k] * vb[k];
            filt<W_, 4>(vq, taps, o); put(4);
          } else {
#pragma unroll
            for (int k = 0; k < 4 + W_ - 1; ++k) vq[k] = hs[2][r * HXW + c0 + k];
            filt<W_, 4>(vq, taps, o); put(2);
          }
        }
      }
      __syncthreads();
      // ---- y pass: column xo, RPT consecutive output rows
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        float v[RPT + W_ - 1];
#pragma unroll
        for (int k = 0; k < RPT + W_ - 1; ++k) v[k] = tw[f][(r0 + k) * MT_X + xo];
        filt<W_, RPT>(v, taps, nf[f]);
      }
    } else {
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int m = 0; m < RPT; ++m) nf[f][m] = 0.f;
    }
    // ---- ring <- the new plane (the taps are tied to the position in the ring, so it is shifted, not rotated)
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int m = 0; m < RPT; ++m) {
#pragma unroll
        for (int k = 0; k + 1 < W_; ++k) ring[f][m][k] = ring[f][m][k + 1];
        ring[f][m][W_ - 1] = nf[f][m];
      }
    const int z = zp - P;
    if (z < zs0) continue;
    // ---- z filter + pointwise tail of plane z
#pragma unroll
    for (int m = 0; m < RPT; ++m) {
      const int y = y0 + r0 + m, xg = x0 + xo;
      if (y >= d.H || xg >= d.W) continue;
      float F[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        float o1[1];
        filt<W_, 1>(ring[f][m], taps, o1);
        F[f] = o1[0];
      }
      const int64_t o = vol + (int64_t)z * plane + (int64_t)y * d.W + xg;
      if constexpr (FWD) {
        constexpr float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
        const float m1 = F[0], m2 = F[1], s11 = F[2], s22 = F[3], s12 = F[4];
        const float m12 = m1 * m2, m1s = m1 * m1, m2s = m2 * m2;
        const float A1 = 2.f * m12 + C1, A2 = 2.f * (s12 - m12) + C2;
        const float B1 = m1s + m2s + C1, B2 = (s11 - m1s) + (s22 - m2s) + C2;
        const float den = B1 * B2;
        const float S = (A1 * A2) / den;
        lsum += (double)S;
        if (out0) {
          // d S / d field, S = A1 A2 / (B1 B2)
          const float rden = 1.f / den, rB1 = 1.f / B1, rB2 = 1.f / B2;
          out0[o] = -S * rB2;                                     // G a^2 and G b^2 alike
          out1[o] = 2.f * A1 * rden;                              // G ab
          const float k = 2.f * (A2 - A1) * rden, h = 2.f * S * (rB1 - rB2);
          if (out2) out2[o] = m2 * k - m1 * h;                    // G a
          if (out3) out3[o] = m1 * k - m2 * h;                    // G b
        }
      } else {
        out0[o] = g * (F[0] + 2.f * self[o] * F[1] + other[o] * F[2]);
      }
    }
  }
  if constexpr (FWD) {
    const double r = block_sum_d<BLK>(lsum, red);
    if (tid == 0) part[blockIdx.x] = r;
  }
}

// loss[0] = 1 - sum(part[0..n)) / count  (fp64, fixed order)
__global__ void ssim_finalize_kernel(const double* __restrict__ part, int n, double count, float* __restrict__ loss) {
  __shared__ double sm[BLK];
  const double r = fixed_order_sum<BLK>(part, n, sm);
  if (threadIdx.x == 0) loss[0] = (float)(1.0 - r / count);
}

inline bool window_ok(int w) { return w >= 1 && w <= MAX_WIN && (w & 1) == 1; }

// the reference's gaussian(): exp in double, rounded to fp32, divided by their fp32 sum.  The sum is the correctly rounded one
// (added in double): equal to torch's sum of the fp32 taps for every window here, where an fp32 chain is one ulp off at w = 11
inline Taps make_taps(int w) {
  const int p = w / 2;
  float gauss[MAX_WIN];
  double acc = 0.0;
  for (int i = 0; i < w; ++i) {
    gauss[i] = (float)exp(-(double)((i - p) * (i - p)) / (2.0 * 1.5 * 1.5));
    acc += (double)gauss[i];
  }
  const float sum = (float)acc;
  Taps t{};
  for (int j = 0; j <= p; ++j) t.t[j] = gauss[j] / sum;
  return t;
}

struct Plan { int tiles_x, tiles_y, nchunk, zc, grid; };
// a function of the shape and the window alone.  z chunks: every chunk filters window - 1 planes in x and y that it does
// not own, so a chunk is at least twice that long; beyond that as many workgroups as fill the chip a few times
inline bool make_plan(int B, int D, int H, int W, int win, Plan& p) {
  if (B < 1 || D < 1 || H < 1 || W < 1 || !window_ok(win)) return false;
  if ((int64_t)B * D * H * W >= (1ll << 31)) return false;       // (the grid and the offsets inside a volume are 32-bit)
  p.tiles_x = cdiv(W, MT_X); p.tiles_y = cdiv(H, MT_Y);
  const int cols = B * p.tiles_x * p.tiles_y;
  int zc = cdiv(D, cdiv(1024, cols));
  if (zc < 2 * (win - 1)) zc = 2 * (win - 1);
  if (zc > D) zc = D;
  if (zc < 1) zc = 1;
  p.zc = zc; p.nchunk = cdiv(D, zc);
  p.grid = cols * p.nchunk;
  return true;
}
inline size_t part_bytes(const Plan& p) { return (((size_t)p.grid * sizeof(double)) + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

size_t modet_ssim_ws_bytes(int B, int D, int H, int W, int window) {
  Plan p;
  if (!make_plan(B, D, H, W, window, p)) return 0;
  return part_bytes(p) + (size_t)4 * (size_t)B * D * H * W * sizeof(float);
}

int modet_ssim_fwd_bwd(const float* a, const float* b, float* loss, float* d_a, float* d_b, void* ws, size_t ws_bytes, int B,
                       int D, int H, int W, int window, float grad_scale, modet_stream_t stream) {
  MODET_CHECK_PTR(a); MODET_CHECK_PTR(b); MODET_CHECK_PTR(loss); MODET_CHECK_PTR(ws);
  MODET_CHECK_DIM(B > 0 && D > 0 && H > 0 && W > 0);
  if (!window_ok(window)) return MODET_ERR_UNSUPPORTED;
  Plan p;
  MODET_CHECK_DIM(make_plan(B, D, H, W, window, p));
  if (ws_bytes < modet_ssim_ws_bytes(B, D, H, W, window) || ((uintptr_t)ws & 7) != 0) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Dims d{B, D, H, W};
  const int64_t N = (int64_t)B * D * H * W;
  double* part = (double*)ws;
  float* c_sq = (float*)((char*)ws + part_bytes(p));
  float* c_x = c_sq + N;
  float* c_m1 = c_x + N;
  float* c_m2 = c_m1 + N;
  const bool any = d_a || d_b;
  const Taps taps = make_taps(window);
  const float g = -grad_scale / (float)N;
  const float* none = nullptr;
#define SSIM_GO(W_)                                                                                                          \
  do {                                                                                                                      \
    hipLaunchKernelGGL((ssim_march_kernel<W_, true>), dim3(p.grid), dim3(BLK), 0, s, a, b, none, none, none,              \
                       any ? c_sq : (float*)nullptr, any ? c_x : (float*)nullptr, d_a ? c_m1 : (float*)nullptr,             \
                       d_b ? c_m2 : (float*)nullptr, part, d, p.tiles_x, p.tiles_y, p.nchunk, p.zc, 0.f, taps);             \
    hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(BLK), 0, s, (const double*)part, p.grid, (double)N, loss);      \
    if (d_a)                                                                                                                \
      hipLaunchKernelGGL((ssim_march_kernel<W_, false>), dim3(p.grid), dim3(BLK), 0, s, (const float*)c_m1,               \
                         (const float*)c_sq, (const float*)c_x, a, b, d_a, (float*)nullptr, (float*)nullptr,               \
                         (float*)nullptr, (double*)nullptr, d, p.tiles_x, p.tiles_y, p.nchunk, p.zc, g, taps);              \
    if (d_b)                                                                                                                \
      hipLaunchKernelGGL((ssim_march_kernel<W_, false>), dim3(p.grid), dim3(BLK), 0, s, (const float*)c_m2,               \
                         (const float*)c_sq, (const float*)c_x, b, a, d_b, (float*)nullptr, (float*)nullptr,               \
                         (float*)nullptr, (double*)nullptr, d, p.tiles_x, p.tiles_y, p.nchunk, p.zc, g, taps);              \
  } while (0)
  switch (window) {
    case 11: SSIM_GO(11); break;
    case 9: SSIM_GO(9); break;
    case 7: SSIM_GO(7); break;
    case 5: SSIM_GO(5); break;
    case 3: SSIM_GO(3); break;
    default: SSIM_GO(1); break;
  }
#undef SSIM_GO
  return modet_launch_status();
}

}  // extern "C"
