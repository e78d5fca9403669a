// 3x3x3 convolution with stride 2 and padding 1 on channels-last voxels, with a fused LeakyReLU(slope): forward, data gradient
// (a gather over the eight parity classes) and weight gradient (partial rows + one fixed-order fp64 column sum), and the
// two-tensor channel concatenation.  The encoder layer of the RDN, PCNet and PR++ baselines ("Baseline methods/RDN/models.py"
// :172-192: ConvBlock(cin, cout, 3, 2, 1)).  include/modet_hip_convs2.h has the contract.
//
// Plain fp32 fused multiply-adds on the values as they are (the first layer reads the raw image).  Every kernel is a flat 1-D
// launch without a grid cap: one thread per (output voxel, 4 output channels) in the forward, per (input voxel, 4 input channels)
// in the data gradient, per (tap, 4 ci, 4 co) item and voxel split in the weight gradient.  The weights are re-laid by a first
// launch so that the 4 channels a thread owns are one 16-byte load and the lanes of a wave read consecutive vectors.
#include "strided.h"
#include "../../include/modet_hip_convs2.h"

namespace {

constexpr int MAXC = MODET_CONVS2_MAX_CHANNELS;
#define FAMILY 27, false, false          // strided.h's T, PAD, CIN_MAJOR: w (Cout,Cin,27), channel counts as they are

struct Dims { int B, D, H, W, Do, Ho, Wo, Cin, Cout; };

// thread t = (output voxel, group of 4 output channels); CI = 1 (Cin == 1) or 4 (Cin % 4 == 0)
template <int CI>
__global__ __launch_bounds__(BLK) void convs2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float* __restrict__ y, Dims s,
                                                         int64_t total, int act, float slope) {
  const int64_t t = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (t >= total) return;
  const int CG = s.Cout >> 2;
  const int cg = (int)(t % CG);
  int64_t v = t / CG;
  const int ow = (int)(v % s.Wo); v /= s.Wo;
  const int oh = (int)(v % s.Ho); v /= s.Ho;
  const int od = (int)(v % s.Do);
  const int b = (int)(v / s.Do);
  float4 tot = f4zero();
  for (int kd = 0; kd < 3; ++kd) {
    const int id = 2 * od - 1 + kd;
    if ((unsigned)id >= (unsigned)s.D) continue;
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = 2 * oh - 1 + kh;
      if ((unsigned)ih >= (unsigned)s.H) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = 2 * ow - 1 + kw;
        if ((unsigned)iw >= (unsigned)s.W) continue;
        const int tap = (kd * 3 + kh) * 3 + kw;
        const float* __restrict__ xp = x + ((((int64_t)b * s.D + id) * s.H + ih) * s.W + iw) * s.Cin;
        const float* __restrict__ wq = wp + (int64_t)tap * s.Cin * s.Cout + 4 * cg;
        if (CI == 1) {
          tot = f4fma(xp[0], ld4(wq), tot);
        } else {
          float4 a0 = f4zero(), a1 = f4zero(), a2 = f4zero(), a3 = f4zero();
          for (int ci = 0; ci < s.Cin; ci += 4) {
            const float4 xv = ld4(xp + ci);
            const float* wr = wq + (int64_t)ci * s.Cout;
            a0 = f4fma(xv.x, ld4(wr), a0);
            a1 = f4fma(xv.y, ld4(wr + s.Cout), a1);
            a2 = f4fma(xv.z, ld4(wr + 2 * s.Cout), a2);
            a3 = f4fma(xv.w, ld4(wr + 3 * s.Cout), a3);
          }
          tot = f4add(tot, f4add(f4add(a0, a1), f4add(a2, a3)));
        }
      }
    }
  }
  if (bias != nullptr) {
    tot.x += bias[4 * cg]; tot.y += bias[4 * cg + 1]; tot.z += bias[4 * cg + 2]; tot.w += bias[4 * cg + 3];
  }
  if (act) {
    tot.x = tot.x > 0.f ? tot.x : slope * tot.x; tot.y = tot.y > 0.f ? tot.y : slope * tot.y;
    tot.z = tot.z > 0.f ? tot.z : slope * tot.z; tot.w = tot.w > 0.f ? tot.w : slope * tot.w;
  }
  st4(y + (t / CG) * s.Cout + 4 * cg, tot);
}

// thread t = (input voxel, group of CI input channels): a gather over the taps whose parity matches, all co of each
template <int CI, bool ACT>
__global__ __launch_bounds__(BLK) void convs2_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              const float* __restrict__ wd, float* __restrict__ dx, Dims s,
                                                              int64_t total, float slope) {
  const int64_t t = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (t >= total) return;
  const int CG = CI == 1 ? 1 : (s.Cin >> 2);
  const int cg = (int)(t % CG);
  int64_t v = t / CG;
  const int iw = (int)(v % s.W); v /= s.W;
  const int ih = (int)(v % s.H); v /= s.H;
  const int id = (int)(v % s.D);
  const int b = (int)(v / s.D);
  float4 totP = f4zero(), totQ = f4zero();
  for (int kd = 0; kd < 3; ++kd) {
    const int nd = id + 1 - kd;                 // 2 od = id + 1 - kd
    if (nd < 0 || (nd & 1)) continue;
    const int od = nd >> 1;
    if (od >= s.Do) continue;
    for (int kh = 0; kh < 3; ++kh) {
      const int nh = ih + 1 - kh;
      if (nh < 0 || (nh & 1)) continue;
      const int oh = nh >> 1;
      if (oh >= s.Ho) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int nw = iw + 1 - kw;
        if (nw < 0 || (nw & 1)) continue;
        const int ow = nw >> 1;
        if (ow >= s.Wo) continue;
        const int tap = (kd * 3 + kh) * 3 + kw;
        const int64_t o = (((int64_t)b * s.Do + od) * s.Ho + oh) * s.Wo + ow;
        const float* __restrict__ gp_ = dy + o * s.Cout;
        const float* __restrict__ yp = y + o * s.Cout;          // (not dereferenced unless ACT)
        const float* __restrict__ wq = wd + (int64_t)tap * s.Cout * s.Cin + CI * cg;
        float4 P[4] = {f4zero(), f4zero(), f4zero(), f4zero()}, Q[4] = {f4zero(), f4zero(), f4zero(), f4zero()};
        for (int co = 0; co < s.Cout; co += 4) {
          const float4 g4 = ld4(gp_ + co);
          const float g[4] = {g4.x, g4.y, g4.z, g4.w};
          float yv[4] = {1.f, 1.f, 1.f, 1.f};
          if (ACT) {
            const float4 y4 = ld4(yp + co);
            yv[0] = y4.x; yv[1] = y4.y; yv[2] = y4.z; yv[3] = y4.w;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float* wr = wq + (int64_t)(co + k) * s.Cin;
            const float4 wv = CI == 1 ? make_float4(wr[0], 0.f, 0.f, 0.f) : ld4(wr);
            if (ACT) {
              float a, q;
              split_pq(g[k], yv[k], a, q);
              P[k] = f4fma(a, wv, P[k]);
              Q[k] = f4fma(q, wv, Q[k]);
            } else {
              P[k] = f4fma(g[k], wv, P[k]);
            }
          }
        }
        totP = f4add(totP, f4add(f4add(P[0], P[1]), f4add(P[2], P[3])));
        if (ACT) totQ = f4add(totQ, f4add(f4add(Q[0], Q[1]), f4add(Q[2], Q[3])));
      }
    }
  }
  if (ACT) totP = f4fma(slope, totQ, totP);
  if (CI == 1) dx[t] = totP.x;
  else st4(dx + (t / CG) * s.Cin + 4 * cg, totP);
}

// Stage 1 of the weight gradient.  Item i < WI: (tap, group of CI input channels, group of 4 output channels), cg fastest;
// item WI + cg: the bias columns of output-channel group cg.  blockIdx.x = voxel split s: output voxels [s * V, (s + 1) * V).
// part[(split * NQ + pq)][R], R = 27 Cin Cout + Cout, column (tap * Cin + ci) * Cout + co, then the bias; NQ = ACT ? 2 : 1.
template <int CI, bool ACT>
__global__ __launch_bounds__(BLK) void convs2_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float* __restrict__ y, float* __restrict__ part, Dims s,
                                                                int64_t N, int V) {
  const int CGo = s.Cout >> 2, CGi = CI == 1 ? 1 : (s.Cin >> 2);
  const int WI = 27 * CGi * CGo;
  const int i = blockIdx.y * BLK + threadIdx.x;
  if (i >= WI + CGo) return;
  const bool is_bias = i >= WI;
  int cg, cig = 0, kd = 1, kh = 1, kw = 1, tap = 13;
  if (is_bias) {
    cg = i - WI;
  } else {
    cg = i % CGo;
    const int r = i / CGo;
    cig = r % CGi;
    tap = r / CGi;
    kd = tap / 9; kh = (tap / 3) % 3; kw = tap % 3;
  }
  const int64_t v0 = (int64_t)blockIdx.x * V, v1 = v0 + V < N ? v0 + V : N;
  float4 P[CI], Q[CI];
#pragma unroll
  for (int c = 0; c < CI; ++c) { P[c] = f4zero(); Q[c] = f4zero(); }
  int64_t r0 = v0;
  int ow = (int)(r0 % s.Wo); r0 /= s.Wo;
  int oh = (int)(r0 % s.Ho); r0 /= s.Ho;
  int od = (int)(r0 % s.Do);
  int b = (int)(r0 / s.Do);
  for (int64_t v = v0; v < v1; ++v) {
    const int id = 2 * od - 1 + kd, ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
    if (is_bias || ((unsigned)id < (unsigned)s.D && (unsigned)ih < (unsigned)s.H && (unsigned)iw < (unsigned)s.W)) {
      const float4 g4 = ld4(dy + v * s.Cout + 4 * cg);
      float4 gp = g4, gq = f4zero();
      if (ACT) {
        const float4 y4 = ld4(y + v * s.Cout + 4 * cg);
        split_pq(g4.x, y4.x, gp.x, gq.x); split_pq(g4.y, y4.y, gp.y, gq.y);
        split_pq(g4.z, y4.z, gp.z, gq.z); split_pq(g4.w, y4.w, gp.w, gq.w);
      }
      if (is_bias) {
        P[0] = f4add(P[0], gp);
        if (ACT) Q[0] = f4add(Q[0], gq);
      } else {
        const float* __restrict__ xp = x + ((((int64_t)b * s.D + id) * s.H + ih) * s.W + iw) * s.Cin + CI * cig;
        float xv[CI];
        if (CI == 1) {
          xv[0] = xp[0];
        } else {
          const float4 x4 = ld4(xp);
          xv[0] = x4.x; xv[CI > 1 ? 1 : 0] = x4.y; xv[CI > 2 ? 2 : 0] = x4.z; xv[CI > 3 ? 3 : 0] = x4.w;
        }
#pragma unroll
        for (int c = 0; c < CI; ++c) {
          P[c] = f4fma(xv[c], gp, P[c]);
          if (ACT) Q[c] = f4fma(xv[c], gq, Q[c]);
        }
      }
    }
    if (++ow == s.Wo) {
      ow = 0;
      if (++oh == s.Ho) {
        oh = 0;
        if (++od == s.Do) { od = 0; ++b; }
      }
    }
  }
  const int64_t R = (int64_t)27 * s.Cin * s.Cout + s.Cout;
  constexpr int NQ = ACT ? 2 : 1;
  float* __restrict__ rowP = part + (int64_t)blockIdx.x * NQ * R;
  if (is_bias) {
    st4(rowP + R - s.Cout + 4 * cg, P[0]);
    if (ACT) st4(rowP + R + R - s.Cout + 4 * cg, Q[0]);
  } else {
#pragma unroll
    for (int c = 0; c < CI; ++c) {
      const int64_t col = ((int64_t)tap * s.Cin + CI * cig + c) * s.Cout + 4 * cg;
      st4(rowP + col, P[c]);
      if (ACT) st4(rowP + R + col, Q[c]);
    }
  }
}

// out[n, :C1] = a[n], out[n, C1:] = b[n]; T = float4 with C1, C2 counted in vectors, or float
template <typename T>
__global__ __launch_bounds__(BLK) void cat2_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                                                       int64_t total, int C1, int C2) {
  const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= total) return;
  const int C = C1 + C2;
  const int64_t n = i / C;
  const int c = (int)(i - n * C);
  out[i] = c < C1 ? a[n * C1 + c] : b[n * C2 + (c - C1)];
}
template <typename T>
__global__ __launch_bounds__(BLK) void cat2_bwd_kernel(const T* __restrict__ d_out, T* __restrict__ d_a, T* __restrict__ d_b,
                                                       int64_t total, int C1, int C2) {
  const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= total) return;
  const int C = C1 + C2;
  const int64_t n = i / C;
  const int c = (int)(i - n * C);
  if (c < C1) {
    if (d_a != nullptr) d_a[n * C1 + c] = d_out[i];
  } else if (d_b != nullptr) {
    d_b[n * C2 + (c - C1)] = d_out[i];
  }
}

inline int split_voxels(int Cout) { return Cout <= 64 ? 256 : Cout <= 128 ? 512 : 1024; }
inline int out_dim(int n) { return (n - 1) / 2 + 1; }

inline int covered(int B, int D, int H, int W, int Cin, int Cout) {
  if (B < 1 || D < 1 || H < 1 || W < 1) return MODET_ERR_DIM;
  if (!(Cin == 1 || (Cin >= 4 && Cin % 4 == 0)) || Cin > MAXC || Cout < 4 || Cout % 4 != 0 || Cout > MAXC) return MODET_ERR_UNSUPPORTED;
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)B * D * H * W * Cin >= lim) return MODET_ERR_DIM;
  if ((int64_t)B * out_dim(D) * out_dim(H) * out_dim(W) * Cout >= lim) return MODET_ERR_DIM;
  return MODET_OK;
}
inline Dims dims_of(int B, int D, int H, int W, int Cin, int Cout) {
  return Dims{B, D, H, W, out_dim(D), out_dim(H), out_dim(W), Cin, Cout};
}

}  // namespace

extern "C" {

size_t modet_convs2_ws_bytes(int B, int D, int H, int W, int Cin, int Cout, int pass) {
  if (covered(B, D, H, W, Cin, Cout) != MODET_OK) return 0;
  const size_t wbytes = (size_t)27 * Cin * Cout * sizeof(float);
  if (pass == MODET_CONVS2_PASS_FWD || pass == MODET_CONVS2_PASS_BWD_DATA) return wbytes;
  if (pass != MODET_CONVS2_PASS_BWD_WEIGHT) return 0;
  const int64_t N = (int64_t)B * out_dim(D) * out_dim(H) * out_dim(W);
  const int64_t S = cdiv64(N, (int64_t)split_voxels(Cout));
  return (size_t)2 * (size_t)S * ((size_t)27 * Cin * Cout + Cout) * sizeof(float);
}

int modet_convs2_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int D, int H,
                     int W, int Cin, int Cout, int act, float slope, modet_stream_t stream) {
  const int rc = check_call(x, y, y, w, bias, ws, ws_bytes, modet_convs2_ws_bytes(B, D, H, W, Cin, Cout, MODET_CONVS2_PASS_FWD),
                            covered(B, D, H, W, Cin, Cout), Cin, Cout, act, slope);
  if (rc != MODET_OK) return rc;
  const Dims s = dims_of(B, D, H, W, Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  float* wp = (float*)ws;
  launch_pack<FAMILY>(w, wp, Cin, Cout, 0, st);
  const int64_t total = (int64_t)B * s.Do * s.Ho * s.Wo * (Cout / 4);
  if (Cin == 1)
    hipLaunchKernelGGL(convs2_fwd_kernel<1>, dim3(blocks_for(total)), dim3(BLK), 0, st, x, (const float*)wp, bias, y, s, total, act, slope);
  else
    hipLaunchKernelGGL(convs2_fwd_kernel<4>, dim3(blocks_for(total)), dim3(BLK), 0, st, x, (const float*)wp, bias, y, s, total, act, slope);
  return modet_launch_status();
}

int modet_convs2_bwd_data(const float* d_y, const float* y, const float* w, float* d_x, void* ws, size_t ws_bytes, int B, int D,
                          int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream) {
  const int rc = check_call(d_x, d_y, y, w, nullptr, ws, ws_bytes, modet_convs2_ws_bytes(B, D, H, W, Cin, Cout, MODET_CONVS2_PASS_BWD_DATA),
                            covered(B, D, H, W, Cin, Cout), Cin, Cout, act, slope);
  if (rc != MODET_OK) return rc;
  const Dims s = dims_of(B, D, H, W, Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  float* wd = (float*)ws;
  launch_pack<FAMILY>(w, wd, Cin, Cout, 1, st);
  const int64_t total = (int64_t)B * D * H * W * (Cin == 1 ? 1 : Cin / 4);
  const dim3 grid(blocks_for(total));
#define LAUNCH_BD(CI_, ACT_) \
  hipLaunchKernelGGL((convs2_bwd_data_kernel<CI_, ACT_>), grid, dim3(BLK), 0, st, d_y, y, (const float*)wd, d_x, s, total, slope)
  if (Cin == 1) { if (act) LAUNCH_BD(1, true); else LAUNCH_BD(1, false); }
  else { if (act) LAUNCH_BD(4, true); else LAUNCH_BD(4, false); }
#undef LAUNCH_BD
  return modet_launch_status();
}

int modet_convs2_bwd_weight(const float* x, const float* d_y, const float* y, float* d_w, float* d_b, void* ws, size_t ws_bytes,
                            int B, int D, int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream) {
  const int rc = check_call(x, d_y, y, d_w, d_b, ws, ws_bytes, modet_convs2_ws_bytes(B, D, H, W, Cin, Cout, MODET_CONVS2_PASS_BWD_WEIGHT),
                            covered(B, D, H, W, Cin, Cout), Cin, Cout, act, slope);
  if (rc != MODET_OK) return rc;
  const Dims s = dims_of(B, D, H, W, Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  const int64_t N = (int64_t)B * s.Do * s.Ho * s.Wo;
  const int V = split_voxels(Cout);
  const int S = (int)cdiv64(N, (int64_t)V);
  const int items = 27 * (Cin == 1 ? 1 : Cin / 4) * (Cout / 4) + Cout / 4;
  const dim3 grid(S, blocks_for(items));      // (items: at most 433 workgroups, inside gridDim.y's limit)
#define LAUNCH_BW(CI_, ACT_) \
  hipLaunchKernelGGL((convs2_bwd_weight_kernel<CI_, ACT_>), grid, dim3(BLK), 0, st, x, d_y, y, part, s, N, V)
  if (Cin == 1) { if (act) LAUNCH_BW(1, true); else LAUNCH_BW(1, false); }
  else { if (act) LAUNCH_BW(4, true); else LAUNCH_BW(4, false); }
#undef LAUNCH_BW
  launch_colsum<FAMILY>(part, S, Cin, Cout, act, slope, d_w, d_b, st);
  return modet_launch_status();
}

static int cat2_check(int64_t N, int C1, int C2) {
  if (N < 1 || C1 < 1 || C2 < 1) return MODET_ERR_DIM;
  if (N * ((int64_t)C1 + C2) >= ((int64_t)1 << 31)) return MODET_ERR_DIM;
  return MODET_OK;
}

int modet_cat_channels2_fwd(const float* a, const float* b, float* out, int64_t N, int C1, int C2, modet_stream_t stream) {
  MODET_CHECK_PTR(a); MODET_CHECK_PTR(b); MODET_CHECK_PTR(out);
  const int rc = cat2_check(N, C1, C2);
  if (rc != MODET_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (C1 % 4 == 0 && C2 % 4 == 0) {
    if (!aligned16(a) || !aligned16(b) || !aligned16(out)) return MODET_ERR_UNSUPPORTED;
    const int64_t total = N * ((C1 + C2) / 4);
    hipLaunchKernelGGL(cat2_fwd_kernel<float4>, dim3(blocks_for(total)), dim3(BLK), 0, st, (const float4*)a, (const float4*)b,
                       (float4*)out, total, C1 / 4, C2 / 4);
  } else {
    if (!aligned4(a) || !aligned4(b) || !aligned4(out)) return MODET_ERR_UNSUPPORTED;
    const int64_t total = N * (C1 + C2);
    hipLaunchKernelGGL(cat2_fwd_kernel<float>, dim3(blocks_for(total)), dim3(BLK), 0, st, a, b, out, total, C1, C2);
  }
  return modet_launch_status();
}

int modet_cat_channels2_bwd(const float* d_out, float* d_a, float* d_b, int64_t N, int C1, int C2, modet_stream_t stream) {
  MODET_CHECK_PTR(d_out);
  if (d_a == nullptr && d_b == nullptr) return MODET_ERR_NULL;
  const int rc = cat2_check(N, C1, C2);
  if (rc != MODET_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (C1 % 4 == 0 && C2 % 4 == 0) {
    if (!aligned16(d_out) || !aligned16(d_a) || !aligned16(d_b)) return MODET_ERR_UNSUPPORTED;
    const int64_t total = N * ((C1 + C2) / 4);
    hipLaunchKernelGGL(cat2_bwd_kernel<float4>, dim3(blocks_for(total)), dim3(BLK), 0, st, (const float4*)d_out, (float4*)d_a,
                       (float4*)d_b, total, C1 / 4, C2 / 4);
  } else {
    if (!aligned4(d_out) || !aligned4(d_a) || !aligned4(d_b)) return MODET_ERR_UNSUPPORTED;
    const int64_t total = N * (C1 + C2);
    hipLaunchKernelGGL(cat2_bwd_kernel<float>, dim3(blocks_for(total)), dim3(BLK), 0, st, d_out, d_a, d_b, total, C1, C2);
  }
  return modet_launch_status();
}

}  // extern "C"
