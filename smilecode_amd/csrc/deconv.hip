// 4x4x4 transposed convolution with stride 2 and padding 1 on channels-last voxels, with a fused LeakyReLU(slope): forward (eight
// parity classes, each a 2x2x2 gather), data gradient (a 4x4x4 stride-2 gather) and weight gradient (partial rows + one fixed-order
// fp64 column sum).  The upsampling layer of the RCN / VTN and PCNet baselines ("Baseline methods/RCN/models.py": ConvTranspose3d(4,
// stride=2) + crop; "PCnet/models.py": UpConvBlock).  include/modet_hip_deconv.h has the contract.
//
// Plain fp32 fused multiply-adds on the values as they are.  Forward and data gradient work on 3-D tiles of INPUT voxels: a
// workgroup of 256 threads stages its window in LDS -- the tile plus a one-voxel halo of x, 16 input channels at a time, for the
// forward; the 2T + 2 window of d_y (split by the sign of y into its P and Q parts), 4 output channels at a time, for the gradient --
// and every read of the eight parity classes / 64 taps and of all the channels the workgroup owns comes from that window.  A
// thread is (voxel of the tile, group of 4 channels); the voxels of a wave share their channel group, so the weights, re-laid and
// zero-padded to multiples of 4 channels by a first launch, are wave-uniform 16-byte loads.  LDS rows: 16 + 4 floats in the forward
// (5 16-byte slots: consecutive voxels of a ds_read_b128 lane group fall on different slots), one slot in the gradient, whose
// lanes are two voxels apart (2-way conflicts: cdna_hip_programming.md's bank rule has no even stride without them).
#include "strided.h"
#include "../../include/modet_hip_deconv.h"

namespace {

#define FAMILY 64, true, true            // strided.h's T, PAD, CIN_MAJOR: w (Cin,Cout,64), channel counts padded to multiples of 4
constexpr int MAXC = MODET_DECONV_MAX_CHANNELS;
constexpr int CK = 16;                   // input channels per staged chunk of the forward
constexpr int LS4 = CK / 4 + 1;          // LDS row of a window voxel in 16-byte slots (one slot of padding)

struct Dims { int B, D, H, W, Cin, Cout; };

// channels [c, c + 4) of a row of C channels: one 16-byte load (VEC: C % 4 == 0) or a scalar tail that stays below C
template <bool VEC>
__device__ __forceinline__ float4 ldc4(const float* __restrict__ row, int c, int C) {
  if (VEC) return ld4(row + c);
  float4 r = f4zero();
  if (c < C) r.x = row[c];
  if (c + 1 < C) r.y = row[c + 1];
  if (c + 2 < C) r.z = row[c + 2];
  if (c + 3 < C) r.w = row[c + 3];
  return r;
}
template <bool VEC>
__device__ __forceinline__ void stc4(float* __restrict__ row, int c, int C, float4 v) {
  if (VEC) { st4(row + c, v); return; }
  if (c < C) row[c] = v.x;
  if (c + 1 < C) row[c + 1] = v.y;
  if (c + 2 < C) row[c + 2] = v.z;
  if (c + 3 < C) row[c + 3] = v.w;
}

// Workgroup = (tile of TD x TH x TW input voxels, 256 / NV groups of 4 output channels); thread = (voxel, group).  Neighbour n in
// {0,1,2} of an axis is input i - 1 + n; it feeds output 2 i + p through tap k = p + 3 - 2 n where that is in 0 .. 3.
template <int TD, int TH, int TW, bool VX, bool VY>
__global__ __launch_bounds__(BLK) void deconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float* __restrict__ y, Dims s, int ntd,
                                                         int nth, int ntw, int act, float slope) {
  constexpr int NV = TD * TH * TW, CGW = BLK / NV, WH = TH + 2, WW = TW + 2, NWV = (TD + 2) * WH * WW;
  static_assert(NV % 64 == 0 && CGW * NV == BLK, "a wave shares its channel group");
  __shared__ float4 win[NWV * LS4];
  const int tid = threadIdx.x;
  const int v = tid % NV;
  const int cg = blockIdx.y * CGW + __builtin_amdgcn_readfirstlane(tid / NV);
  const int lw = v % TW, lh = (v / TW) % TH, ld = v / (TW * TH);
  int t = blockIdx.x;
  const int w0 = (t % ntw) * TW; t /= ntw;
  const int h0 = (t % nth) * TH; t /= nth;
  const int dd0 = (t % ntd) * TD;
  const int b = t / ntd;
  const int CiP = pad4(s.Cin), CoP = pad4(s.Cout), CoG = CoP >> 2;
  const int gd = dd0 + ld, gh = h0 + lh, gw = w0 + lw;
  const bool mine = cg < CoG && gd < s.D && gh < s.H && gw < s.W;
  float4 acc[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) acc[p] = f4zero();
  for (int c0 = 0; c0 < s.Cin; c0 += CK) {
    const int nci = s.Cin - c0 < CK ? s.Cin - c0 : CK;
    const int nslots = (nci + 3) >> 2;
    __syncthreads();                                          // the previous chunk's reads are done
    for (int idx = tid; idx < NWV * nslots; idx += BLK) {
      const int sl = idx % nslots, wv = idx / nslots;
      const int id = dd0 - 1 + wv / (WW * WH), ih = h0 - 1 + (wv / WW) % WH, iw = w0 - 1 + wv % WW;
      float4 val = f4zero();
      if ((unsigned)id < (unsigned)s.D && (unsigned)ih < (unsigned)s.H && (unsigned)iw < (unsigned)s.W)
        val = ldc4<VX>(x + ((((int64_t)b * s.D + id) * s.H + ih) * s.W + iw) * s.Cin, c0 + 4 * sl, s.Cin);
      win[wv * LS4 + sl] = val;
    }
    __syncthreads();
    if (mine) {
      const float* __restrict__ wbase = wp + c0 * CoP + 4 * cg;
      for (int sl = 0; sl < nslots; ++sl) {
#pragma unroll
        for (int nd = 0; nd < 3; ++nd) {
#pragma unroll
          for (int nh = 0; nh < 3; ++nh) {
#pragma unroll
            for (int nw = 0; nw < 3; ++nw) {
              const float4 xv = win[(((ld + nd) * WH + lh + nh) * WW + lw + nw) * LS4 + sl];
              const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
              for (int pd = 0; pd < 2; ++pd) {
                const int kd = pd + 3 - 2 * nd;
                if (kd < 0 || kd > 3) continue;
#pragma unroll
                for (int ph = 0; ph < 2; ++ph) {
                  const int kh = ph + 3 - 2 * nh;
                  if (kh < 0 || kh > 3) continue;
#pragma unroll
                  for (int pw = 0; pw < 2; ++pw) {
                    const int kw = pw + 3 - 2 * nw;
                    if (kw < 0 || kw > 3) continue;
                    const int tap = (kd * 4 + kh) * 4 + kw, p = (pd * 2 + ph) * 2 + pw;
                    const float* __restrict__ wr = wbase + (tap * CiP + 4 * sl) * CoP;
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[p] = f4fma(xs[c], ld4(wr + c * CoP), acc[p]);
                  }
                }
              }
            }
          }
        }
      }
    }
  }
  if (!mine) return;
  float4 bv = f4zero();
  if (bias != nullptr) bv = ldc4<false>(bias, 4 * cg, s.Cout);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    float4 z = f4add(acc[p], bv);
    if (act) {
      z.x = z.x > 0.f ? z.x : slope * z.x; z.y = z.y > 0.f ? z.y : slope * z.y;
      z.z = z.z > 0.f ? z.z : slope * z.z; z.w = z.w > 0.f ? z.w : slope * z.w;
    }
    const int od = 2 * gd + (p >> 2), oh = 2 * gh + ((p >> 1) & 1), ow = 2 * gw + (p & 1);
    stc4<VY>(y + ((((int64_t)b * 2 * s.D + od) * 2 * s.H + oh) * 2 * s.W + ow) * s.Cout, 4 * cg, s.Cout, z);
  }
}

// Workgroup = (tile of TD x TH x TW input voxels, 256 / NV groups of 4 input channels); thread = (voxel, group).  The window holds
// output voxels 2 t0 - 1 .. 2 (t0 + T), 4 output channels per round; input voxel i reads window index 2 (i - t0) + k for tap k.
template <int TD, int TH, int TW, bool ACT, bool VX, bool VY>
__global__ __launch_bounds__(BLK) void deconv_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                              const float* __restrict__ wd, float* __restrict__ dx, Dims s,
                                                              int ntd, int nth, int ntw, float slope) {
  constexpr int NV = TD * TH * TW, CGW = BLK / NV, WH = 2 * TH + 2, WW = 2 * TW + 2, NWV = (2 * TD + 2) * WH * WW;
  constexpr int NQ = ACT ? 2 : 1;
  static_assert(NV % 64 == 0 && CGW * NV == BLK, "a wave shares its channel group");
  __shared__ float4 win[NQ * NWV];
  const int tid = threadIdx.x;
  const int v = tid % NV;
  const int cig = blockIdx.y * CGW + __builtin_amdgcn_readfirstlane(tid / NV);
  const int lw = v % TW, lh = (v / TW) % TH, ld = v / (TW * TH);
  int t = blockIdx.x;
  const int w0 = (t % ntw) * TW; t /= ntw;
  const int h0 = (t % nth) * TH; t /= nth;
  const int d0 = (t % ntd) * TD;
  const int b = t / ntd;
  const int CiP = pad4(s.Cin), CoP = pad4(s.Cout), CiG = CiP >> 2;
  const int gd = d0 + ld, gh = h0 + lh, gw = w0 + lw;
  const bool mine = cig < CiG && gd < s.D && gh < s.H && gw < s.W;
  const int OD = 2 * s.D, OH = 2 * s.H, OW = 2 * s.W;
  float4 P0 = f4zero(), P1 = f4zero(), Q0 = f4zero(), Q1 = f4zero();
  for (int co0 = 0; co0 < s.Cout; co0 += 4) {
    __syncthreads();                                          // the previous round's reads are done
    for (int idx = tid; idx < NWV; idx += BLK) {
      const int od = 2 * d0 - 1 + idx / (WW * WH), oh = 2 * h0 - 1 + (idx / WW) % WH, ow = 2 * w0 - 1 + idx % WW;
      float4 gp = f4zero(), gq = f4zero();
      if ((unsigned)od < (unsigned)OD && (unsigned)oh < (unsigned)OH && (unsigned)ow < (unsigned)OW) {
        const int64_t o = ((((int64_t)b * OD + od) * OH + oh) * OW + ow) * s.Cout;
        gp = ldc4<VY>(dy + o, co0, s.Cout);
        if (ACT) {
          const float4 g = gp;
          split_pq4(g, ldc4<VY>(y + o, co0, s.Cout), gp, gq);    // (a channel beyond Cout: g = 0 on either side)
        }
      }
      win[idx] = gp;
      if (ACT) win[NWV + idx] = gq;
    }
    __syncthreads();
    if (mine) {
      const float* __restrict__ wbase = wd + co0 * CiP + 4 * cig;
#pragma unroll
      for (int kd = 0; kd < 4; ++kd) {
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
#pragma unroll
          for (int kw = 0; kw < 4; ++kw) {
            const int at = ((2 * ld + kd) * WH + 2 * lh + kh) * WW + 2 * lw + kw;
            const int tap = (kd * 4 + kh) * 4 + kw;
            const float* __restrict__ wr = wbase + tap * CoP * CiP;
            const float4 w0v = ld4(wr), w1v = ld4(wr + CiP), w2v = ld4(wr + 2 * CiP), w3v = ld4(wr + 3 * CiP);
            const float4 gp = win[at];
            P0 = f4fma(gp.x, w0v, P0); P1 = f4fma(gp.y, w1v, P1); P0 = f4fma(gp.z, w2v, P0); P1 = f4fma(gp.w, w3v, P1);
            if (ACT) {
              const float4 gq = win[NWV + at];
              Q0 = f4fma(gq.x, w0v, Q0); Q1 = f4fma(gq.y, w1v, Q1); Q0 = f4fma(gq.z, w2v, Q0); Q1 = f4fma(gq.w, w3v, Q1);
            }
          }
        }
      }
    }
  }
  if (!mine) return;
  float4 tot = f4add(P0, P1);
  if (ACT) tot = f4fma(slope, f4add(Q0, Q1), tot);
  stc4<VX>(dx + ((((int64_t)b * s.D + gd) * s.H + gh) * s.W + gw) * s.Cin, 4 * cig, s.Cin, tot);
}

// Stage 1 of the weight gradient.  Item i < WI: (tap, group of 4 input channels, group of 4 output channels), co group fastest;
// item WI + cg: the bias columns of output-channel group cg.  blockIdx.x = voxel split: INPUT voxels [split * V, (split + 1) * V).
// part[(split * NQ + pq)][R], R = 64 CiP CoP + CoP, column (tap * CiP + ci) * CoP + co, then the bias; NQ = ACT ? 2 : 1.
template <bool ACT, bool VX, bool VY>
__global__ __launch_bounds__(BLK) void deconv_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                const float* __restrict__ y, float* __restrict__ part, Dims s,
                                                                int64_t N, int V) {
  const int CiP = pad4(s.Cin), CoP = pad4(s.Cout), CoG = CoP >> 2, CiG = CiP >> 2;
  const int WI = 64 * CiG * CoG;
  const int i = blockIdx.y * BLK + threadIdx.x;
  if (i >= WI + CoG) return;
  const bool is_bias = i >= WI;
  int cg, cig = 0, kd = 0, kh = 0, kw = 0, tap = 0;
  if (is_bias) {
    cg = i - WI;
  } else {
    cg = i % CoG;
    const int r = i / CoG;
    cig = r % CiG;
    tap = r / CiG;
    kd = tap >> 4; kh = (tap >> 2) & 3; kw = tap & 3;
  }
  const int OD = 2 * s.D, OH = 2 * s.H, OW = 2 * s.W;
  const int64_t v0 = (int64_t)blockIdx.x * V, v1 = v0 + V < N ? v0 + V : N;
  float4 P[4], Q[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { P[c] = f4zero(); Q[c] = f4zero(); }
  int64_t r0 = v0;
  int iw = (int)(r0 % s.W); r0 /= s.W;
  int ih = (int)(r0 % s.H); r0 /= s.H;
  int id = (int)(r0 % s.D);
  int b = (int)(r0 / s.D);
  for (int64_t v = v0; v < v1; ++v) {
    if (is_bias) {
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int64_t o = ((((int64_t)b * OD + 2 * id + (p >> 2)) * OH + 2 * ih + ((p >> 1) & 1)) * OW + 2 * iw + (p & 1)) * s.Cout;
        float4 gp = ldc4<VY>(dy + o, 4 * cg, s.Cout), gq = f4zero();
        if (ACT) {
          const float4 g = gp;
          split_pq4(g, ldc4<VY>(y + o, 4 * cg, s.Cout), gp, gq);
        }
        P[p & 3] = f4add(P[p & 3], gp);
        if (ACT) Q[p & 3] = f4add(Q[p & 3], gq);
      }
    } else {
      const int od = 2 * id - 1 + kd, oh = 2 * ih - 1 + kh, ow = 2 * iw - 1 + kw;
      if ((unsigned)od < (unsigned)OD && (unsigned)oh < (unsigned)OH && (unsigned)ow < (unsigned)OW) {
        const int64_t o = ((((int64_t)b * OD + od) * OH + oh) * OW + ow) * s.Cout;
        float4 gp = ldc4<VY>(dy + o, 4 * cg, s.Cout), gq = f4zero();
        if (ACT) {
          const float4 g = gp;
          split_pq4(g, ldc4<VY>(y + o, 4 * cg, s.Cout), gp, gq);
        }
        const float4 x4 = ldc4<VX>(x + v * s.Cin, 4 * cig, s.Cin);
        P[0] = f4fma(x4.x, gp, P[0]); P[1] = f4fma(x4.y, gp, P[1]); P[2] = f4fma(x4.z, gp, P[2]); P[3] = f4fma(x4.w, gp, P[3]);
        if (ACT) {
          Q[0] = f4fma(x4.x, gq, Q[0]); Q[1] = f4fma(x4.y, gq, Q[1]); Q[2] = f4fma(x4.z, gq, Q[2]); Q[3] = f4fma(x4.w, gq, Q[3]);
        }
      }
    }
    if (++iw == s.W) {
      iw = 0;
      if (++ih == s.H) {
        ih = 0;
        if (++id == s.D) { id = 0; ++b; }
      }
    }
  }
  const int64_t R = (int64_t)64 * CiP * CoP + CoP;
  constexpr int NQ = ACT ? 2 : 1;
  float* __restrict__ rowP = part + (int64_t)blockIdx.x * NQ * R;
  if (is_bias) {
    st4(rowP + R - CoP + 4 * cg, f4add(f4add(P[0], P[1]), f4add(P[2], P[3])));
    if (ACT) st4(rowP + R + R - CoP + 4 * cg, f4add(f4add(Q[0], Q[1]), f4add(Q[2], Q[3])));
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t col = ((int64_t)tap * CiP + 4 * cig + c) * CoP + 4 * cg;
      st4(rowP + col, P[c]);
      if (ACT) st4(rowP + R + col, Q[c]);
    }
  }
}

inline int covered(int B, int D, int H, int W, int Cin, int Cout) {
  if (B < 1 || D < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return MODET_ERR_DIM;
  if (Cin > MAXC || Cout > MAXC) return MODET_ERR_UNSUPPORTED;
  const int64_t lim = (int64_t)1 << 31;
  const int64_t n = (int64_t)B * D * H * W;
  if (n >= lim || n * Cin >= lim || n * 8 >= lim || n * 8 * Cout >= lim) return MODET_ERR_DIM;
  return MODET_OK;
}
inline int split_voxels(int64_t N) { const int64_t v = cdiv64(N, 256); return v < 256 ? 256 : (int)v; }
inline size_t packed_bytes(int Cin, int Cout) { return (size_t)64 * pad4(Cin) * pad4(Cout) * sizeof(float); }

// THE ROUTING of the forward and of the data gradient: the tile by the number of 4-channel groups a workgroup can fill
inline int fwd_tile(int Cout) { return Cout <= 4 ? 0 : Cout <= 8 ? 1 : 2; }            // 4x8x8 | 4x4x8 | 4x4x4
inline int bwd_data_tile(int Cin) { return Cin <= 8 ? 1 : 2; }                          // 4x4x8 | 4x4x4

}  // namespace

extern "C" {

size_t modet_deconv4s2_ws_bytes(int B, int D, int H, int W, int Cin, int Cout, int pass) {
  if (covered(B, D, H, W, Cin, Cout) != MODET_OK) return 0;
  if (pass == MODET_DECONV_PASS_FWD || pass == MODET_DECONV_PASS_BWD_DATA) return packed_bytes(Cin, Cout);
  if (pass != MODET_DECONV_PASS_BWD_WEIGHT) return 0;
  const int64_t N = (int64_t)B * D * H * W;
  const int64_t S = cdiv64(N, (int64_t)split_voxels(N));
  return (size_t)2 * (size_t)S * ((size_t)64 * pad4(Cin) * pad4(Cout) + pad4(Cout)) * sizeof(float);
}

int modet_deconv4s2_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int D, int H,
                        int W, int Cin, int Cout, int act, float slope, modet_stream_t stream) {
  const int rc = check_call(x, y, y, w, bias, ws, ws_bytes, modet_deconv4s2_ws_bytes(B, D, H, W, Cin, Cout, MODET_DECONV_PASS_FWD),
                            covered(B, D, H, W, Cin, Cout), Cin, Cout, act, slope);
  if (rc != MODET_OK) return rc;
  const Dims s{B, D, H, W, Cin, Cout};
  hipStream_t st = (hipStream_t)stream;
  float* wp = (float*)ws;
  launch_pack<FAMILY>(w, wp, Cin, Cout, 0, st);
  const int CoG = pad4(Cout) / 4;
  const bool vx = Cin % 4 == 0, vy = Cout % 4 == 0;
#define LAUNCH_F3(TD_, TH_, TW_, VX_, VY_)                                                                                      \
  do {                                                                                                                          \
    const int ntd = cdiv(D, TD_), nth = cdiv(H, TH_), ntw = cdiv(W, TW_);                                                       \
    const dim3 grid((unsigned)((int64_t)B * ntd * nth * ntw), (unsigned)cdiv(CoG, BLK / (TD_ * TH_ * TW_)));                    \
    hipLaunchKernelGGL((deconv_fwd_kernel<TD_, TH_, TW_, VX_, VY_>), grid, dim3(BLK), 0, st, x, (const float*)wp, bias, y, s, ntd, \
                       nth, ntw, act, slope);                                                                                   \
  } while (0)
#define LAUNCH_F(TD_, TH_, TW_)                                                        \
  do {                                                                                 \
    if (vx) { if (vy) LAUNCH_F3(TD_, TH_, TW_, true, true); else LAUNCH_F3(TD_, TH_, TW_, true, false); }  \
    else { if (vy) LAUNCH_F3(TD_, TH_, TW_, false, true); else LAUNCH_F3(TD_, TH_, TW_, false, false); }   \
  } while (0)
  switch (fwd_tile(Cout)) {
    case 0: LAUNCH_F(4, 8, 8); break;
    case 1: LAUNCH_F(4, 4, 8); break;
    default: LAUNCH_F(4, 4, 4); break;
  }
#undef LAUNCH_F
#undef LAUNCH_F3
  return modet_launch_status();
}

int modet_deconv4s2_bwd_data(const float* d_y, const float* y, const float* w, float* d_x, void* ws, size_t ws_bytes, int B, int D,
                             int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream) {
  const int rc = check_call(d_x, d_y, y, w, nullptr, ws, ws_bytes, modet_deconv4s2_ws_bytes(B, D, H, W, Cin, Cout, MODET_DECONV_PASS_BWD_DATA),
                            covered(B, D, H, W, Cin, Cout), Cin, Cout, act, slope);
  if (rc != MODET_OK) return rc;
  const Dims s{B, D, H, W, Cin, Cout};
  hipStream_t st = (hipStream_t)stream;
  float* wd = (float*)ws;
  launch_pack<FAMILY>(w, wd, Cin, Cout, 1, st);
  const int CiG = pad4(Cin) / 4;
  const bool vx = Cin % 4 == 0, vy = Cout % 4 == 0;
#define LAUNCH_D4(TD_, TH_, TW_, ACT_, VX_, VY_)                                                                                \
  do {                                                                                                                          \
    const int ntd = cdiv(D, TD_), nth = cdiv(H, TH_), ntw = cdiv(W, TW_);                                                       \
    const dim3 grid((unsigned)((int64_t)B * ntd * nth * ntw), (unsigned)cdiv(CiG, BLK / (TD_ * TH_ * TW_)));                    \
    hipLaunchKernelGGL((deconv_bwd_data_kernel<TD_, TH_, TW_, ACT_, VX_, VY_>), grid, dim3(BLK), 0, st, d_y, y, (const float*)wd, \
                       d_x, s, ntd, nth, ntw, slope);                                                                           \
  } while (0)
#define LAUNCH_D2(TD_, TH_, TW_, ACT_)                                                 \
  do {                                                                                 \
    if (vx) { if (vy) LAUNCH_D4(TD_, TH_, TW_, ACT_, true, true); else LAUNCH_D4(TD_, TH_, TW_, ACT_, true, false); }  \
    else { if (vy) LAUNCH_D4(TD_, TH_, TW_, ACT_, false, true); else LAUNCH_D4(TD_, TH_, TW_, ACT_, false, false); }   \
  } while (0)
  if (bwd_data_tile(Cin) == 1) { if (act) LAUNCH_D2(4, 4, 8, true); else LAUNCH_D2(4, 4, 8, false); }
  else { if (act) LAUNCH_D2(4, 4, 4, true); else LAUNCH_D2(4, 4, 4, false); }
#undef LAUNCH_D2
#undef LAUNCH_D4
  return modet_launch_status();
}

int modet_deconv4s2_bwd_weight(const float* x, const float* d_y, const float* y, float* d_w, float* d_b, void* ws, size_t ws_bytes,
                               int B, int D, int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream) {
  const int rc = check_call(x, d_y, y, d_w, d_b, ws, ws_bytes, modet_deconv4s2_ws_bytes(B, D, H, W, Cin, Cout, MODET_DECONV_PASS_BWD_WEIGHT),
                            covered(B, D, H, W, Cin, Cout), Cin, Cout, act, slope);
  if (rc != MODET_OK) return rc;
  const Dims s{B, D, H, W, Cin, Cout};
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  const int64_t N = (int64_t)B * D * H * W;
  const int V = split_voxels(N);
  const int S = (int)cdiv64(N, (int64_t)V);
  const int items = 64 * (pad4(Cin) / 4) * (pad4(Cout) / 4) + pad4(Cout) / 4;
  const dim3 grid(S, blocks_for(items));      // (items: at most 16 385 workgroups, inside gridDim.y's limit)
  const bool vx = Cin % 4 == 0, vy = Cout % 4 == 0;
#define LAUNCH_W3(ACT_, VX_, VY_) \
  hipLaunchKernelGGL((deconv_bwd_weight_kernel<ACT_, VX_, VY_>), grid, dim3(BLK), 0, st, x, d_y, y, part, s, N, V)
#define LAUNCH_W(ACT_)                                                                 \
  do {                                                                                 \
    if (vx) { if (vy) LAUNCH_W3(ACT_, true, true); else LAUNCH_W3(ACT_, true, false); }  \
    else { if (vy) LAUNCH_W3(ACT_, false, true); else LAUNCH_W3(ACT_, false, false); }   \
  } while (0)
  if (act) LAUNCH_W(true); else LAUNCH_W(false);
#undef LAUNCH_W
#undef LAUNCH_W3
  launch_colsum<FAMILY>(part, S, Cin, Cout, act, slope, d_w, d_b, st);
  return modet_launch_status();
}

}  // extern "C"
