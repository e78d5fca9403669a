// The PR++ family (include/modet_hip_prpp.h; "Baseline methods/PR++/models.py":113-352, PRNetplusplus): the decoder's nearest
// upsampling + concatenation, ReLU and x + relu(res), the block's stack [mov | correlation | fix] as one channels-last row, and the
// composition of a flow on a coarser grid with a field on the finer one.  All memory traffic: fp32, channels-last, 64-bit element
// offsets, 256-thread workgroups, no float atomics, every sum in a fixed order (the scatter of the composition's backward adds
// 64-bit fixed-point integers, as modet_warp_bwd_det does: integer addition has no order).  The correlation's box sums, dot
// products and transposed gathers are corr3d.hip's own (corr3d_internal.h).
#include "corr3d_internal.h"

#include "../../include/modet_hip_prpp.h"

namespace {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

template <bool VEC> struct Unit;
template <> struct Unit<true> { using T = float4; static constexpr int N = 4; };
template <> struct Unit<false> { using T = float; static constexpr int N = 1; };

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float add4(float a, float b) { return a + b; }

// ------------------------------------------------------------------------------------------------ nearest x2 + concatenation
// one thread per (fine voxel, unit of the output row); a unit is a channel quad (VEC) or one channel
template <bool VEC>
__global__ __launch_bounds__(BLK) void upcat_fwd_kernel(const float* __restrict__ x, const float* __restrict__ skip, float* __restrict__ out,
                                                        int d, int h, int w, int C1, int C2, int64_t total) {
  using T = typename Unit<VEC>::T;
  constexpr int U = Unit<VEC>::N;
  const int Q1 = C1 / U, Q = (C1 + C2) / U;
  const int H = 2 * h, W = 2 * w, D = 2 * d;
  for (int64_t idx = (int64_t)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * BLK) {
    const int q = (int)(idx % Q);
    const int64_t n = idx / Q;
    const T* from;
    if (q < Q1) {
      const int xo = (int)(n % W);
      int64_t r = n / W;
      const int yo = (int)(r % H); r /= H;
      const int zo = (int)(r % D);
      const int64_t b = r / D;
      from = reinterpret_cast<const T*>(x + ((((b * d + (zo >> 1)) * h + (yo >> 1)) * w + (xo >> 1)) * C1)) + q;
    } else {
      from = reinterpret_cast<const T*>(skip + n * C2) + (q - Q1);
    }
    reinterpret_cast<T*>(out + n * (C1 + C2))[q] = *from;
  }
}

// d_x: one thread per (coarse voxel, unit of C1); the eight children in the order (dz, dy, dx) = (0,0,0), (0,0,1) .. (1,1,1)
template <bool VEC>
__global__ __launch_bounds__(BLK) void upcat_bwd_x_kernel(const float* __restrict__ d_out, float* __restrict__ d_x, int d, int h, int w,
                                                          int C1, int C2, int64_t total) {
  using T = typename Unit<VEC>::T;
  constexpr int U = Unit<VEC>::N;
  const int Q1 = C1 / U;
  const int64_t R = C1 + C2, sx = R, sy = (int64_t)2 * w * R, sz = (int64_t)4 * h * w * R;
  for (int64_t idx = (int64_t)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * BLK) {
    const int q = (int)(idx % Q1);
    const int64_t n = idx / Q1;
    const int xc = (int)(n % w);
    int64_t r = n / w;
    const int yc = (int)(r % h); r /= h;
    const int zc = (int)(r % d);
    const int64_t b = r / d;
    const float* base = d_out + (((b * 2 * d + 2 * zc) * 2 * h + 2 * yc) * 2 * w + 2 * xc) * R;
    T v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = reinterpret_cast<const T*>(base + ((k >> 2) ? sz : 0) + (((k >> 1) & 1) ? sy : 0) + ((k & 1) ? sx : 0))[q];
    T acc = v[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) acc = add4(acc, v[k]);
    reinterpret_cast<T*>(d_x + n * C1)[q] = acc;
  }
}

template <bool VEC>
__global__ __launch_bounds__(BLK) void upcat_bwd_skip_kernel(const float* __restrict__ d_out, float* __restrict__ d_skip, int C1, int C2,
                                                             int64_t total) {
  using T = typename Unit<VEC>::T;
  constexpr int U = Unit<VEC>::N;
  const int Q2 = C2 / U;
  for (int64_t idx = (int64_t)blockIdx.x * BLK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * BLK) {
    const int q = (int)(idx % Q2);
    const int64_t n = idx / Q2;
    reinterpret_cast<T*>(d_skip + n * C2)[q] = reinterpret_cast<const T*>(d_out + n * (C1 + C2) + C1)[q];
  }
}

// ------------------------------------------------------------------------------------------------ ReLU
// `t <= 0 ? 0 : t`: a NaN fails the comparison and passes through, -0 becomes +0
__device__ __forceinline__ float relu1(float t) { return t <= 0.f ? 0.f : t; }
__device__ __forceinline__ float gate1(float g, float y) { return y <= 0.f ? 0.f : g; }

// MODE 0: o = relu(b);  1: o = a + relu(b);  2: o = a gated by b > 0.  Thread i owns floats [4 i, 4 i + 4); the n % 4 floats of
// the tail belong to the first threads of workgroup 0
template <int MODE>
__global__ __launch_bounds__(BLK) void relu_kernel(const float* a, const float* b, float* o, int64_t n) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n4; i += (int64_t)gridDim.x * BLK) {
    const float4 bv = reinterpret_cast<const float4*>(b)[i];
    float4 r;
    if constexpr (MODE == 0) {
      r = make_float4(relu1(bv.x), relu1(bv.y), relu1(bv.z), relu1(bv.w));
    } else {
      const float4 av = reinterpret_cast<const float4*>(a)[i];
      if constexpr (MODE == 1) r = make_float4(av.x + relu1(bv.x), av.y + relu1(bv.y), av.z + relu1(bv.z), av.w + relu1(bv.w));
      else r = make_float4(gate1(av.x, bv.x), gate1(av.y, bv.y), gate1(av.z, bv.z), gate1(av.w, bv.w));
    }
    reinterpret_cast<float4*>(o)[i] = r;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    if constexpr (MODE == 0) o[i] = relu1(b[i]);
    else if constexpr (MODE == 1) o[i] = a[i] + relu1(b[i]);
    else o[i] = gate1(a[i], b[i]);
  }
}

template <int MODE>
inline int relu_call(const float* a, const float* b, float* o, int64_t n, modet_stream_t stream) {
  if (MODE != 0) MODET_CHECK_PTR(a);
  MODET_CHECK_PTR(b); MODET_CHECK_PTR(o);
  MODET_CHECK_DIM(n >= 1);
  if (!aligned16(a) || !aligned16(b) || !aligned16(o)) return MODET_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(relu_kernel<MODE>, dim3(flat_grid((n >> 2) + 1, BLK)), dim3(BLK), 0, (hipStream_t)stream, a, b, o, n);
  return modet_launch_status();
}

// ------------------------------------------------------------------------------------------------ the stack
// One workgroup per strip of CS_V = 32 consecutive voxels: corr_strip leaves the 27 x 32 dot products in LDS; they are stored
// voxel by voxel, so that 27 consecutive lanes write the 27 consecutive floats of a row's middle slice; then the two outer slices,
// lanes along the channels of a row (rows of 2 C + 27 floats start on 4-byte boundaries only: scalar stores, contiguous per row)
__global__ __launch_bounds__(BLK) void stack_fwd_kernel(const float* __restrict__ mov, const float* __restrict__ fix,
                                                        const float* __restrict__ pm, const float* __restrict__ pfx, float* __restrict__ out,
                                                        int D, int H, int W, int C, int64_t N) {
  __shared__ float res[27 * CS_V];
  const int64_t n0 = (int64_t)blockIdx.x * CS_V;
  const int64_t R = 2 * C + 27;
  corr_strip(pm, pfx, res, D, H, W, C, N, n0);
  __syncthreads();
  for (int i = threadIdx.x; i < 27 * CS_V; i += BLK) {
    const int v = i / 27, t = i - v * 27;
    const int64_t n = n0 + v;
    if (n < N) out[n * R + C + t] = res[t * CS_V + v] * (1.f / 27.f);
  }
  for (int i = threadIdx.x; i < CS_V * C; i += BLK) {
    const int v = i / C, c = i - v * C;
    const int64_t n = n0 + v;
    if (n < N) {
      out[n * R + c] = mov[n * C + c];
      out[n * R + C + 27 + c] = fix[n * C + c];
    }
  }
}

inline int stack_check(int B, int D, int H, int W, int C) {
  if (const int e = corr_check(B, D, H, W, C)) return e;
  if (C > MODET_PRPP_MAX_C) return MODET_ERR_UNSUPPORTED;
  return MODET_OK;
}

// ------------------------------------------------------------------------------------------------ cross-grid composition
struct Tri {            // trilinear footprint of one sample point (warp.hip's)
  int z0, y0, x0;
  float fz, fy, fx;
};
__device__ __forceinline__ Tri tri_setup(float z, float y, float x) {
  Tri t;
  const float zf = floorf(z), yf = floorf(y), xf = floorf(x);
  t.fz = z - zf; t.fy = y - yf; t.fx = x - xf;
  // clamp before the int conversion so wild fields cannot overflow; anything outside [-2, dim] is invalid anyway
  t.z0 = (int)fminf(fmaxf(zf, -2.f), 1.0e9f);
  t.y0 = (int)fminf(fmaxf(yf, -2.f), 1.0e9f);
  t.x0 = (int)fminf(fmaxf(xf, -2.f), 1.0e9f);
  return t;
}

struct Grids {
  int Dc, Hc, Wc, Df, Hf, Wf;
  float rz, ry, rx;     // (Sc - 1) / (Sf - 1) per axis: exactly 1 on equal grids, exactly 1/2 where Sf - 1 = 2 (Sc - 1)
};

// the eight corners of fine voxel n's sample point: element offsets inside the sample's coarse field (clamped to a valid voxel
// where the corner is outside), validity and weights; returns the sample
struct Corners {
  int64_t off[8];
  bool ok[8];
  float wz[2], wy[2], wx[2];
};
__device__ __forceinline__ void corners_of(const Grids& g, int zi, int yi, int xi, float f0, float f1, float f2, Corners& c) {
  // with a ratio of exactly 1 the product is the sum itself: modet_warp_fwd's sample point, bit for bit
  const float z = ((float)zi + f0) * g.rz, y = ((float)yi + f1) * g.ry, x = ((float)xi + f2) * g.rx;
  const Tri t = tri_setup(z, y, x);
  int64_t zo[2], yo[2], xo[2];
  bool zk[2], yk[2], xk[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const int zz = t.z0 + d, yy = t.y0 + d, xx = t.x0 + d;
    zk[d] = zz >= 0 && zz < g.Dc; yk[d] = yy >= 0 && yy < g.Hc; xk[d] = xx >= 0 && xx < g.Wc;
    zo[d] = (int64_t)(zk[d] ? zz : 0) * g.Hc * g.Wc * 3;
    yo[d] = (int64_t)(yk[d] ? yy : 0) * g.Wc * 3;
    xo[d] = (int64_t)(xk[d] ? xx : 0) * 3;
    c.wz[d] = d ? t.fz : 1.f - t.fz;
    c.wy[d] = d ? t.fy : 1.f - t.fy;
    c.wx[d] = d ? t.fx : 1.f - t.fx;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c.off[q] = zo[q >> 2] + yo[(q >> 1) & 1] + xo[q & 1];
    c.ok[q] = zk[q >> 2] && yk[(q >> 1) & 1] && xk[q & 1];
  }
}

// one thread per fine voxel; the accumulation is warp_fwd_kernel's (corner order, fmaf, the field added last)
__global__ __launch_bounds__(BLK) void compose_fwd_kernel(const float* __restrict__ src, const float* __restrict__ w, float* __restrict__ out,
                                                          Grids g, int64_t total) {
  const int64_t Vf = (int64_t)g.Df * g.Hf * g.Wf, Vc = (int64_t)g.Dc * g.Hc * g.Wc;
  for (int64_t n = (int64_t)blockIdx.x * BLK + threadIdx.x; n < total; n += (int64_t)gridDim.x * BLK) {
    const int64_t b = n / Vf, p = n - b * Vf;
    const int xi = (int)(p % g.Wf);
    const int64_t r = p / g.Wf;
    const int yi = (int)(r % g.Hf), zi = (int)(r / g.Hf);
    const float f0 = w[n * 3], f1 = w[n * 3 + 1], f2 = w[n * 3 + 2];
    Corners c;
    corners_of(g, zi, yi, xi, f0, f1, f2, c);
    const float* sb = src + b * Vc * 3;
    float s[8][3];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      s[q][0] = sb[c.off[q]]; s[q][1] = sb[c.off[q] + 1]; s[q][2] = sb[c.off[q] + 2];
    }
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float wgt = c.wz[q >> 2] * c.wy[(q >> 1) & 1] * c.wx[q & 1];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] = fmaf(wgt, c.ok[q] ? s[q][ch] : 0.f, acc[ch]);
    }
    out[n * 3] = acc[0] + f0; out[n * 3 + 1] = acc[1] + f1; out[n * 3 + 2] = acc[2] + f2;
  }
}

// The fixed-point unit of the scatter, PER SAMPLE (header[b]: a batch of two gives the bits of two batches of one): m = max |d_out|
// of the sample < 2^e, a coarse element receives at most one contribution per fine voxel of its sample and each is at most m, so
// with 2^lg >= the voxel count the sums stay below 2^(e + lg): unit 2^-(62 - e - lg).
__device__ __forceinline__ double fixed_scale(const unsigned* header, int lg) {
  const float m = __uint_as_float(header[0]);                       // (bit pattern: the integer maximum of non-negative floats is exact)
  int e;
  frexpf(m > 0.f ? m : 1.f, &e);
  return ldexp(1.0, 62 - lg - e);
}
// grid (blocks, B): sample blockIdx.y's n floats
__global__ __launch_bounds__(BLK) void absmax_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ header) {
  const float* xb = x + (int64_t)blockIdx.y * n;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLK) m = fmaxf(m, fabsf(xb[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(header + blockIdx.y, __float_as_uint(m));       // an integer maximum: no order
}
__global__ __launch_bounds__(BLK) void decode_kernel(const long long* __restrict__ acc, float* __restrict__ out, int64_t n,
                                                     const unsigned* __restrict__ header, int lg) {
  const long long* ab = acc + (int64_t)blockIdx.y * n;
  float* ob = out + (int64_t)blockIdx.y * n;
  const double inv = 1.0 / fixed_scale(header + blockIdx.y, lg);
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLK) ob[i] = (float)((double)ab[i] * inv);
}

// one thread per fine voxel: its d_w (a gather over its own eight corners) and, with acc, its 24 contributions to d_src
__global__ __launch_bounds__(BLK) void compose_bwd_kernel(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ d_out,
                                                          float* __restrict__ d_w, long long* __restrict__ acc,
                                                          const unsigned* __restrict__ header, int lg, Grids g, int64_t total) {
  const int64_t Vf = (int64_t)g.Df * g.Hf * g.Wf, Vc = (int64_t)g.Dc * g.Hc * g.Wc;
  for (int64_t n = (int64_t)blockIdx.x * BLK + threadIdx.x; n < total; n += (int64_t)gridDim.x * BLK) {
    const int64_t b = n / Vf, p = n - b * Vf;
    const double scale = acc ? fixed_scale(header + b, lg) : 0.0;
    const int xi = (int)(p % g.Wf);
    const int64_t r = p / g.Wf;
    const int yi = (int)(r % g.Hf), zi = (int)(r / g.Hf);
    const float f0 = w[n * 3], f1 = w[n * 3 + 1], f2 = w[n * 3 + 2];
    const float go[3] = {d_out[n * 3], d_out[n * 3 + 1], d_out[n * 3 + 2]};
    Corners c;
    corners_of(g, zi, yi, xi, f0, f1, f2, c);
    if (d_w) {
      const float* sb = src + b * Vc * 3;
      float dot[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float s0 = sb[c.off[q]], s1 = sb[c.off[q] + 1], s2 = sb[c.off[q] + 2];
        dot[q] = c.ok[q] ? fmaf(go[2], s2, fmaf(go[1], s1, go[0] * s0)) : 0.f;
      }
      float dz = 0.f, dy = 0.f, dx = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float az = c.wy[(q >> 1) & 1] * c.wx[q & 1], ay = c.wz[q >> 2] * c.wx[q & 1], ax = c.wz[q >> 2] * c.wy[(q >> 1) & 1];
        dz = fmaf((q >> 2) ? az : -az, dot[q], dz);
        dy = fmaf(((q >> 1) & 1) ? ay : -ay, dot[q], dy);
        dx = fmaf((q & 1) ? ax : -ax, dot[q], dx);
      }
      d_w[n * 3] = fmaf(g.rz, dz, go[0]); d_w[n * 3 + 1] = fmaf(g.ry, dy, go[1]); d_w[n * 3 + 2] = fmaf(g.rx, dx, go[2]);
    }
    if (acc) {
      unsigned long long* ab = reinterpret_cast<unsigned long long*>(acc) + b * Vc * 3;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (!c.ok[q]) continue;
        const float wgt = c.wz[q >> 2] * c.wy[(q >> 1) & 1] * c.wx[q & 1];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float v = wgt * go[ch];
          if (v != 0.f) atomicAdd(ab + c.off[q] + ch, (unsigned long long)__double2ll_rn((double)v * scale));
        }
      }
    }
  }
}

inline int compose_check(int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf) {
  if (B < 1 || B > 65535 || Dc < 1 || Hc < 1 || Wc < 1 || Df < 2 || Hf < 2 || Wf < 2) return MODET_ERR_DIM;      // (B is a grid dimension)
  return MODET_OK;
}
inline size_t header_bytes(int B) { return ((size_t)B * sizeof(unsigned) + 63) / 64 * 64; }      // one maximum per sample
inline Grids grids_of(int Dc, int Hc, int Wc, int Df, int Hf, int Wf) {
  Grids g;
  g.Dc = Dc; g.Hc = Hc; g.Wc = Wc; g.Df = Df; g.Hf = Hf; g.Wf = Wf;
  g.rz = (float)(Dc - 1) / (float)(Df - 1); g.ry = (float)(Hc - 1) / (float)(Hf - 1); g.rx = (float)(Wc - 1) / (float)(Wf - 1);
  return g;
}

}  // namespace

extern "C" {

int modet_prpp_upcat_fwd(const float* x, const float* skip, float* out, int B, int d, int h, int w, int C1, int C2, modet_stream_t stream) {
  MODET_CHECK_PTR(x); MODET_CHECK_PTR(skip); MODET_CHECK_PTR(out);
  MODET_CHECK_DIM(B >= 1 && d >= 1 && h >= 1 && w >= 1 && C1 >= 1 && C2 >= 1);
  if (!aligned4(x) || !aligned4(skip) || !aligned4(out)) return MODET_ERR_UNSUPPORTED;
  const bool vec = C1 % 4 == 0 && C2 % 4 == 0 && aligned16(x) && aligned16(skip) && aligned16(out);
  const int64_t nf = (int64_t)B * d * h * w * 8;
  const int64_t total = nf * ((C1 + C2) / (vec ? 4 : 1));
  hipStream_t s = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(upcat_fwd_kernel<true>, dim3(flat_grid(total, BLK)), dim3(BLK), 0, s, x, skip, out, d, h, w, C1, C2, total);
  else hipLaunchKernelGGL(upcat_fwd_kernel<false>, dim3(flat_grid(total, BLK)), dim3(BLK), 0, s, x, skip, out, d, h, w, C1, C2, total);
  return modet_launch_status();
}

int modet_prpp_upcat_bwd(const float* d_out, float* d_x, float* d_skip, int B, int d, int h, int w, int C1, int C2, modet_stream_t stream) {
  MODET_CHECK_PTR(d_out);
  if (d_x == nullptr && d_skip == nullptr) return MODET_ERR_NULL;
  MODET_CHECK_DIM(B >= 1 && d >= 1 && h >= 1 && w >= 1 && C1 >= 1 && C2 >= 1);
  if (!aligned4(d_out) || !aligned4(d_x) || !aligned4(d_skip)) return MODET_ERR_UNSUPPORTED;
  const bool vec = C1 % 4 == 0 && C2 % 4 == 0 && aligned16(d_out) && aligned16(d_x) && aligned16(d_skip);
  const int64_t nc = (int64_t)B * d * h * w, nf = nc * 8;
  const int U = vec ? 4 : 1;
  hipStream_t s = (hipStream_t)stream;
  if (d_x) {
    const int64_t total = nc * (C1 / U);
    if (vec) hipLaunchKernelGGL(upcat_bwd_x_kernel<true>, dim3(flat_grid(total, BLK)), dim3(BLK), 0, s, d_out, d_x, d, h, w, C1, C2, total);
    else hipLaunchKernelGGL(upcat_bwd_x_kernel<false>, dim3(flat_grid(total, BLK)), dim3(BLK), 0, s, d_out, d_x, d, h, w, C1, C2, total);
  }
  if (d_skip) {
    const int64_t total = nf * (C2 / U);
    if (vec) hipLaunchKernelGGL(upcat_bwd_skip_kernel<true>, dim3(flat_grid(total, BLK)), dim3(BLK), 0, s, d_out, d_skip, C1, C2, total);
    else hipLaunchKernelGGL(upcat_bwd_skip_kernel<false>, dim3(flat_grid(total, BLK)), dim3(BLK), 0, s, d_out, d_skip, C1, C2, total);
  }
  return modet_launch_status();
}

int modet_prpp_relu_fwd(const float* t, float* y, int64_t n, modet_stream_t stream) { return relu_call<0>(nullptr, t, y, n, stream); }
int modet_prpp_relu_add_fwd(const float* x, const float* t, float* out, int64_t n, modet_stream_t stream) {
  return relu_call<1>(x, t, out, n, stream);
}
int modet_prpp_relu_bwd(const float* d_y, const float* y_or_t, float* d_t, int64_t n, modet_stream_t stream) {
  return relu_call<2>(d_y, y_or_t, d_t, n, stream);
}

size_t modet_prpp_stack_ws_bytes(int B, int D, int H, int W, int C) {
  return stack_check(B, D, H, W, C) == MODET_OK ? corr_ws_bytes(B, D, H, W, C) : 0;
}

int modet_prpp_stack_fwd(const float* mov, const float* fix, float* out, void* ws, size_t ws_bytes, int B, int D, int H, int W, int C,
                         modet_stream_t stream) {
  MODET_CHECK_PTR(mov); MODET_CHECK_PTR(fix); MODET_CHECK_PTR(out); MODET_CHECK_PTR(ws);
  if (const int e = stack_check(B, D, H, W, C)) return e;
  if (!aligned16(mov) || !aligned16(fix) || !aligned4(out)) return MODET_ERR_UNSUPPORTED;
  if (ws_bytes < corr_ws_bytes(B, D, H, W, C) || !aligned16(ws)) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * D * H * W;
  float* pm = (float*)ws;
  float* pfx = pm + n * C;
  launch_box_pair(mov, fix, pm, pfx, B, D, H, W, C, s);
  hipLaunchKernelGGL(stack_fwd_kernel, dim3((unsigned)cdiv64(n, CS_V)), dim3(BLK), 0, s, mov, fix, (const float*)pm, (const float*)pfx, out, D,
                     H, W, C, n);
  return modet_launch_status();
}

int modet_prpp_stack_bwd(const float* mov, const float* fix, const float* d_out, float* d_mov, float* d_fix, void* ws, size_t ws_bytes,
                         int B, int D, int H, int W, int C, modet_stream_t stream) {
  MODET_CHECK_PTR(mov); MODET_CHECK_PTR(fix); MODET_CHECK_PTR(d_out); MODET_CHECK_PTR(ws);
  if (d_mov == nullptr && d_fix == nullptr) return MODET_ERR_NULL;
  if (const int e = stack_check(B, D, H, W, C)) return e;
  if (!aligned16(mov) || !aligned16(fix) || !aligned16(d_mov) || !aligned16(d_fix) || !aligned4(d_out)) return MODET_ERR_UNSUPPORTED;
  if (ws_bytes < corr_ws_bytes(B, D, H, W, C) || !aligned16(ws)) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * D * H * W, ne = ext_elems(B, D, H, W, C) / C;
  const unsigned G = C / 4;
  const int ld = 2 * C + 27;
  float* pm = (float*)ws;
  float* pfx = pm + n * C;
  float* dpm = pfx + ne * C;
  float* dpfx = dpm + n * C;
  launch_box_pair(mov, fix, pm, pfx, B, D, H, W, C, s);
  // as modet_corr3d_bwd, the cotangent read from channels [C, C + 27) of the rows; the last box sums add the rows' outer slices
  if (d_mov) {
    hipLaunchKernelGGL(corr_bwd_pm_kernel, dim3(flat_grid(n * G, BLK)), dim3(BLK), 0, s, d_out, (const float*)pfx, dpm, D, H, W, C,
                       (unsigned)(n * G), ld, C);
    hipLaunchKernelGGL(box3_kernel<true>, dim3(flat_grid(n * G, BLK)), dim3(BLK), 0, s, (const float*)dpm, d_mov, D, H, W, C, 0, 0,
                       (unsigned)(n * G), d_out, ld, 0);
  }
  if (d_fix) {
    hipLaunchKernelGGL(corr_bwd_pf_kernel, dim3(flat_grid(ne * G, BLK)), dim3(BLK), 0, s, d_out, (const float*)pm, dpfx, D, H, W, C,
                       (unsigned)(ne * G), ld, C);
    hipLaunchKernelGGL(box3_kernel<true>, dim3(flat_grid(n * G, BLK)), dim3(BLK), 0, s, (const float*)dpfx, d_fix, D, H, W, C, 1, 0,
                       (unsigned)(n * G), d_out, ld, C + 27);
  }
  return modet_launch_status();
}

size_t modet_prpp_compose_ws_bytes(int B, int Dc, int Hc, int Wc) {
  if (B < 1 || B > 65535 || Dc < 1 || Hc < 1 || Wc < 1) return 0;
  return header_bytes(B) + (size_t)B * Dc * Hc * Wc * 3 * sizeof(long long);
}

int modet_prpp_compose_fwd(const float* src, const float* w, float* out, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf,
                           modet_stream_t stream) {
  MODET_CHECK_PTR(src); MODET_CHECK_PTR(w); MODET_CHECK_PTR(out);
  if (const int e = compose_check(B, Dc, Hc, Wc, Df, Hf, Wf)) return e;
  if (!aligned4(src) || !aligned4(w) || !aligned4(out)) return MODET_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)B * Df * Hf * Wf;
  hipLaunchKernelGGL(compose_fwd_kernel, dim3(flat_grid(total, BLK)), dim3(BLK), 0, (hipStream_t)stream, src, w, out,
                     grids_of(Dc, Hc, Wc, Df, Hf, Wf), total);
  return modet_launch_status();
}

int modet_prpp_compose_bwd(const float* src, const float* w, const float* d_out, float* d_src, float* d_w, void* ws, size_t ws_bytes, int B,
                           int Dc, int Hc, int Wc, int Df, int Hf, int Wf, modet_stream_t stream) {
  MODET_CHECK_PTR(src); MODET_CHECK_PTR(w); MODET_CHECK_PTR(d_out);
  if (d_src == nullptr && d_w == nullptr) return MODET_ERR_NULL;
  if (d_src) MODET_CHECK_PTR(ws);
  if (const int e = compose_check(B, Dc, Hc, Wc, Df, Hf, Wf)) return e;
  if (!aligned4(src) || !aligned4(w) || !aligned4(d_out) || !aligned4(d_src) || !aligned4(d_w)) return MODET_ERR_UNSUPPORTED;
  const size_t need = modet_prpp_compose_ws_bytes(B, Dc, Hc, Wc);
  if (d_src && (ws_bytes < need || !aligned16(ws))) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)B * Df * Hf * Wf, nsrc = (int64_t)Dc * Hc * Wc * 3, nout = (int64_t)Df * Hf * Wf * 3;
  int lg = 0;
  while (((int64_t)1 << lg) < (int64_t)Df * Hf * Wf) ++lg;
  unsigned* hdr = (unsigned*)ws;
  long long* acc = d_src ? (long long*)((char*)ws + header_bytes(B)) : nullptr;
  if (d_src) {
    modet_zero_async(ws, need, s);
    hipLaunchKernelGGL(absmax_kernel, dim3(flat_grid(nout, BLK) > 256 ? 256 : flat_grid(nout, BLK), B), dim3(BLK), 0, s, d_out, nout, hdr);
  }
  hipLaunchKernelGGL(compose_bwd_kernel, dim3(flat_grid(total, BLK)), dim3(BLK), 0, s, src, w, d_out, d_w, acc, (const unsigned*)hdr, lg,
                     grids_of(Dc, Hc, Wc, Df, Hf, Wf), total);
  if (d_src)
    hipLaunchKernelGGL(decode_kernel, dim3(flat_grid(nsrc, BLK) > 256 ? 256 : flat_grid(nsrc, BLK), B), dim3(BLK), 0, s, (const long long*)acc, d_src,
                       nsrc, (const unsigned*)hdr, lg);
  return modet_launch_status();
}

}  // extern "C"
