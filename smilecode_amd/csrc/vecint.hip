// Scaling and squaring of a stationary velocity field (the reference's VecInt, ModeT/models.py:70-87): include/modet_hip_vecint.h.
// A step is the flow composition v + sample(v, p + v) of warp.hip (modet_warp_fwd with src = flow, add_flow = 1) with the field
// read ONCE, as displacement and addend, and step 0's 2^-nsteps folded into its loads; a backward step writes the identity term,
// the flow term and the transposed sample of that composition with one store -- the composed path's autograd add of d_src and
// d_flow, and its scale pass, have no counterpart here.  Conventions of warp.hip: 256-thread workgroups, 32-bit index arithmetic
// (the entry points refuse 2^31 elements), clamped loads with the VALUE masked afterwards, no allocation, no synchronisation.
#include <math.h>

#include "common.h"
#include "../../include/modet_hip_vecint.h"

namespace {

constexpr int BLK = 256;

// the trilinear footprint of warp.hip, restated (that file's own stays untouched: its kernels keep their code bit for bit)
struct Tri {
  int z0, y0, x0;
  float fz, fy, fx;
};
__device__ __forceinline__ Tri tri_setup(float z, float y, float x) {
  Tri t;
  const float zf = floorf(z), yf = floorf(y), xf = floorf(x);
  t.fz = z - zf; t.fy = y - yf; t.fx = x - xf;
  // clamp before the int conversion so wild fields cannot overflow (NaN -> -2); anything outside [-1, dim - 1] has no valid corner
  t.z0 = (int)fminf(fmaxf(zf, -2.f), 1.0e9f);
  t.y0 = (int)fminf(fmaxf(yf, -2.f), 1.0e9f);
  t.x0 = (int)fminf(fmaxf(xf, -2.f), 1.0e9f);
  return t;
}

// the eight corners of one footprint inside sample b's field: clamped element offsets (always inside the field) and validity
struct Corners {
  unsigned off[8];
  bool ok[8];
};
__device__ __forceinline__ Corners corners(const Tri& t, int D, int H, int W) {
  Corners c;
  unsigned zo[2], yo[2], xo[2];
  bool zk[2], yk[2], xk[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const int zz = t.z0 + d, yy = t.y0 + d, xx = t.x0 + d;
    zk[d] = zz >= 0 && zz < D; yk[d] = yy >= 0 && yy < H; xk[d] = xx >= 0 && xx < W;
    zo[d] = (unsigned)(zk[d] ? zz : 0) * (unsigned)(H * W);
    yo[d] = (unsigned)(yk[d] ? yy : 0) * (unsigned)W;
    xo[d] = (unsigned)(xk[d] ? xx : 0);
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    c.off[q] = (zo[q >> 2] + yo[(q >> 1) & 1] + xo[q & 1]) * 3u;
    c.ok[q] = zk[q >> 2] && yk[(q >> 1) & 1] && xk[q & 1];
  }
  return c;
}

// ------------------------------------------------------------------------------------------------ forward step
// out[p] = v[p] + sample(v, p + v[p]) with v = scale * in.  One lane per voxel: its own vector once, 8 corners of 12 B.
// The arithmetic of warp_fwd_kernel<3> with add_flow: corner terms in the order q = 0 .. 7 into a zero accumulator, then + v.
__global__ __launch_bounds__(BLK) void vecint_step_kernel(const float* __restrict__ in, float* __restrict__ out, int D, int H,
                                                          int W, unsigned nvox, float scale) {
  const unsigned uW = (unsigned)W, uH = (unsigned)H, uD = (unsigned)D, V = uD * uH * uW;
  for (unsigned n = blockIdx.x * BLK + threadIdx.x; n < nvox; n += gridDim.x * BLK) {
    const int xi = (int)(n % uW);
    const unsigned t2 = n / uW;
    const int yi = (int)(t2 % uH);
    const unsigned t3 = t2 / uH;
    const int zi = (int)(t3 % uD);
    const unsigned b = t3 / uD;
    const float* fp = in + (size_t)n * 3;
    const float v0 = scale * fp[0], v1 = scale * fp[1], v2 = scale * fp[2];
    const Tri t = tri_setup((float)zi + v0, (float)yi + v1, (float)xi + v2);
    const Corners c = corners(t, D, H, W);
    const float* sb = in + (size_t)b * V * 3;
    float s[8][3];
#pragma unroll
    for (int q = 0; q < 8; ++q) {                     // issued back to back, always valid addresses
      const float* p = sb + c.off[q];
      s[q][0] = p[0]; s[q][1] = p[1]; s[q][2] = p[2];
    }
    const float wz[2] = {1.f - t.fz, t.fz}, wy[2] = {1.f - t.fy, t.fy}, wx[2] = {1.f - t.fx, t.fx};
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float wgt = wz[q >> 2] * wy[(q >> 1) & 1] * wx[q & 1];
      a0 = fmaf(wgt, c.ok[q] ? scale * s[q][0] : 0.f, a0);
      a1 = fmaf(wgt, c.ok[q] ? scale * s[q][1] : 0.f, a1);
      a2 = fmaf(wgt, c.ok[q] ? scale * s[q][2] : 0.f, a2);
    }
    float* op = out + (size_t)n * 3;
    op[0] = a0 + v0; op[1] = a1 + v1; op[2] = a2 + v2;
  }
}

__global__ __launch_bounds__(BLK) void vecint_scale_kernel(const float* __restrict__ in, float* __restrict__ out, unsigned n,
                                                           float scale) {
  for (unsigned i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) out[i] = scale * in[i];
}

// the flow term of one voxel: sum_c g_c * d sample_c / d x at p = y + v[y], from the eight corners of v = scale * in
__device__ __forceinline__ void flow_term(const float* __restrict__ sb, float scale, int zi, int yi, int xi, float v0, float v1,
                                          float v2, float g0, float g1, float g2, int D, int H, int W, float& gz, float& gy,
                                          float& gx) {
  const Tri tr = tri_setup((float)zi + v0, (float)yi + v1, (float)xi + v2);
  const Corners c = corners(tr, D, H, W);
  float sp[8][3];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float* p = sb + c.off[q];
    sp[q][0] = p[0]; sp[q][1] = p[1]; sp[q][2] = p[2];
  }
  gz = 0.f; gy = 0.f; gx = 0.f;
#pragma unroll
  for (int dz = 0; dz < 2; ++dz) {
    const float wz = dz ? tr.fz : 1.f - tr.fz;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const float wy = dy ? tr.fy : 1.f - tr.fy;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float wx = dx ? tr.fx : 1.f - tr.fx;
        const int q = dz * 4 + dy * 2 + dx;
        const float dot = c.ok[q] ? (scale * sp[q][0]) * g0 + (scale * sp[q][1]) * g1 + (scale * sp[q][2]) * g2 : 0.f;
        gz += (dz ? 1.f : -1.f) * wy * wx * dot;
        gy += (dy ? 1.f : -1.f) * wz * wx * dot;
        gx += (dx ? 1.f : -1.f) * wz * wy * dot;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward step, bounded
// |v| <= 1: the sample point of x lies within one voxel of x, so y only receives from the 27 voxels x = y + d, d in {-1,0,1}^3,
// with the weight prod_a max(0, 1 - |d_a + v_a[x]|) (the trilinear hat).  The scheme of warp.hip's bounded backward: 4x4x16 voxel
// tiles, v and g of the tile + 1-voxel halo staged in LDS once (6 floats per voxel; g = 0 outside the volume, so the neighbour
// loop needs no bounds tests and reads LDS at fixed offsets whatever the values are).  One thread per voxel, one store:
//   d_v[y] = scale * ((flow term + g[y]) + neighbour sum).
constexpr int TZ = 4, TY = 4, TX = 16, HZ = TZ + 2, HY = TY + 2, HX = TX + 2, HV = HZ * HY * HX;
__global__ __launch_bounds__(BLK) void vecint_bwd_bounded_kernel(const float* __restrict__ in, const float* __restrict__ g,
                                                                 float* __restrict__ dv, int D, int H, int W, int tiles_x,
                                                                 int tiles_y, float scale) {
  __shared__ __attribute__((aligned(8))) float fg[HV * 6];
  const unsigned V = (unsigned)D * (unsigned)H * (unsigned)W;
  const unsigned b = blockIdx.y;
  int t = blockIdx.x;
  const int x0 = (t % tiles_x) * TX; t /= tiles_x;
  const int y0 = (t % tiles_y) * TY;
  const int z0 = (t / tiles_y) * TZ;
  // staging, branch-free: every load of a thread is issued before the first LDS write (clamped addresses, the halo outside the
  // volume selected to zero afterwards)
  constexpr int NST = (HV * 3 + BLK - 1) / BLK;
  float2 stg[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    const int i = min((int)threadIdx.x + j * BLK, HV * 3 - 1);
    const int v = i / 3, part = i - v * 3;               // part 0: v[0..1]; 1: v[2], g[0]; 2: g[1..2]
    const int hx = v % HX, r = v / HX;
    const int hy = r % HY, hz = r / HY;
    const int z = z0 + hz - 1, y = y0 + hy - 1, x = x0 + hx - 1;
    const bool in_vol = z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W;
    const size_t n = ((size_t)b * V + (in_vol ? ((unsigned)z * (unsigned)H + (unsigned)y) * (unsigned)W + (unsigned)x : 0u)) * 3;
    const float* pa = part == 0 ? in + n : (part == 1 ? in + n + 2 : g + n + 1);
    const float* pb = part == 0 ? in + n + 1 : (part == 1 ? g + n : g + n + 2);
    const float va = *pa * (part <= 1 ? scale : 1.f), vb = *pb * (part == 0 ? scale : 1.f);
    stg[j] = in_vol ? make_float2(va, vb) : make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    const int i = threadIdx.x + j * BLK;
    if (i < HV * 3) *reinterpret_cast<float2*>(fg + i * 2) = stg[j];       // fg + v * 6 + part * 2 with i = v * 3 + part
  }
  __syncthreads();
  const int tx = threadIdx.x % TX, ty = (threadIdx.x / TX) % TY, tz = threadIdx.x / (TX * TY);
  const int zi = z0 + tz, yi = y0 + ty, xi = x0 + tx;
  if (zi >= D || yi >= H || xi >= W) return;
  const int lc = ((tz + 1) * HY + ty + 1) * HX + tx + 1;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const float* p = fg + (lc + (dz * HY + dy) * HX + dx) * 6;
        const float2 q0 = *reinterpret_cast<const float2*>(p), q1 = *reinterpret_cast<const float2*>(p + 2),
                     q2 = *reinterpret_cast<const float2*>(p + 4);
        const float wz = 1.f - fabsf((float)dz + q0.x);
        const float wy = 1.f - fabsf((float)dy + q0.y);
        const float wx = 1.f - fabsf((float)dx + q1.x);
        if (wz > 0.f && wy > 0.f && wx > 0.f) {
          const float wgt = wz * wy * wx;
          a0 = fmaf(wgt, q1.y, a0); a1 = fmaf(wgt, q2.x, a1); a2 = fmaf(wgt, q2.y, a2);
        }
      }
  const float* pc = fg + lc * 6;
  const float g0 = pc[3], g1 = pc[4], g2 = pc[5];
  float gz, gy, gx;
  flow_term(in + (size_t)b * V * 3, scale, zi, yi, xi, pc[0], pc[1], pc[2], g0, g1, g2, D, H, W, gz, gy, gx);
  float* op = dv + ((size_t)b * V + ((unsigned)zi * (unsigned)H + (unsigned)yi) * (unsigned)W + (unsigned)xi) * 3;
  op[0] = scale * ((gz + g0) + a0); op[1] = scale * ((gy + g1) + a1); op[2] = scale * ((gx + g2) + a2);
}

// ------------------------------------------------------------------------------------------------ backward step, general
// the transposed sample arrives scattered (ds, from the deterministic machinery of the warp backward, on v = scale * in); this
// adds the identity and the flow term: one read of v, g and ds per voxel, 8 corners of v, one store
__global__ __launch_bounds__(BLK) void vecint_bwd_general_kernel(const float* __restrict__ in, const float* __restrict__ g,
                                                                 const float* __restrict__ ds, float* __restrict__ dv, int D,
                                                                 int H, int W, unsigned nvox, float scale) {
  const unsigned uW = (unsigned)W, uH = (unsigned)H, uD = (unsigned)D, V = uD * uH * uW;
  for (unsigned n = blockIdx.x * BLK + threadIdx.x; n < nvox; n += gridDim.x * BLK) {
    const int xi = (int)(n % uW);
    const unsigned t2 = n / uW;
    const int yi = (int)(t2 % uH);
    const unsigned t3 = t2 / uH;
    const int zi = (int)(t3 % uD);
    const unsigned b = t3 / uD;
    const size_t e = (size_t)n * 3;
    const float v0 = scale * in[e], v1 = scale * in[e + 1], v2 = scale * in[e + 2];
    const float g0 = g[e], g1 = g[e + 1], g2 = g[e + 2];
    const float s0 = ds[e], s1 = ds[e + 1], s2 = ds[e + 2];
    float gz, gy, gx;
    flow_term(in + (size_t)b * V * 3, scale, zi, yi, xi, v0, v1, v2, g0, g1, g2, D, H, W, gz, gy, gx);
    dv[e] = scale * ((gz + g0) + s0); dv[e + 1] = scale * ((gy + g1) + s1); dv[e + 2] = scale * ((gx + g2) + s2);
  }
}

// ------------------------------------------------------------------------------------------------ host
inline bool args_ok(int B, int D, int H, int W, int nsteps) {
  if (B < 1 || D < 1 || H < 1 || W < 1 || nsteps < 0 || nsteps > MODET_VECINT_MAX_STEPS) return false;
  return (double)B * D * H * W * 3.0 < 2147483648.0 && B <= 65535;
}
inline bool bound_ok(float bound) { return bound >= 0.f && bound <= 3.0e38f; }     // (NaN fails the first, +inf the second)
// steps 0 .. first_general - 1 run the bounded kernel: bound * 2^(k - nsteps) grows with k
inline int first_general(int nsteps, float bound) {
  int k = 0;
  while (k < nsteps && bound > 0.f && ldexp((double)bound, k - nsteps) <= 1.0) ++k;
  return k;
}
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
struct BwdWs { size_t field, v0_off, sub_off, sub_bytes, bytes; bool tiles; };
inline BwdWs bwd_ws(int B, int D, int H, int W, int nsteps, float bound) {
  BwdWs w{};
  const int kg = first_general(nsteps, bound);
  if (kg >= nsteps) return w;                                         // every step bounded: nothing
  w.field = up256((size_t)B * D * H * W * 3 * sizeof(float));
  w.v0_off = kg == 0 ? w.field : 0;                                   // [d_src][v_0 when step 0 is general][scatter workspace]
  w.sub_off = w.field + (kg == 0 ? w.field : 0);
  const size_t tb = modet_warp_bwd_dsrc_tiles_ws_bytes(B, D, H, W, 3);
  w.tiles = tb != 0;
  w.sub_bytes = w.tiles ? tb : modet_warp_bwd_det_ws_bytes(B, D, H, W, 3);
  w.bytes = w.sub_off + up256(w.sub_bytes);
  return w;
}

}  // namespace

extern "C" {

int modet_vecint_fwd(const float* vec, float* out, float* steps, float* scratch, int B, int D, int H, int W, int nsteps,
                     modet_stream_t stream) {
  MODET_CHECK_PTR(vec); MODET_CHECK_PTR(out);
  MODET_CHECK_DIM(args_ok(B, D, H, W, nsteps));
  if (nsteps >= 2 && !steps) MODET_CHECK_PTR(scratch);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nvox = (unsigned)B * D * H * W;
  const size_t F = (size_t)nvox * 3;
  if (nsteps == 0) {
    hipLaunchKernelGGL(vecint_scale_kernel, dim3(flat_grid((int64_t)F, BLK)), dim3(BLK), 0, s, vec, out, (unsigned)F, 1.f);
    return modet_launch_status();
  }
  const float* in = vec;
  for (int k = 0; k < nsteps; ++k) {
    float* dst;
    if (k == nsteps - 1) dst = out;
    else if (steps) dst = steps + (size_t)k * F;
    else dst = ((nsteps - 1 - k) & 1) ? scratch : out;
    hipLaunchKernelGGL(vecint_step_kernel, dim3(flat_grid(nvox, BLK)), dim3(BLK), 0, s, in, dst, D, H, W, nvox,
                       k == 0 ? ldexpf(1.f, -nsteps) : 1.f);
    in = dst;
  }
  return modet_launch_status();
}

size_t modet_vecint_ws_bytes(int B, int D, int H, int W, int nsteps, float bound) {
  if (!args_ok(B, D, H, W, nsteps) || !bound_ok(bound)) return 0;
  return bwd_ws(B, D, H, W, nsteps, bound).bytes;
}

int modet_vecint_bwd(const float* vec, const float* steps, const float* d_out, float* d_vec, float* scratch, void* ws,
                     size_t ws_bytes, int B, int D, int H, int W, int nsteps, float bound, modet_stream_t stream) {
  MODET_CHECK_PTR(vec); MODET_CHECK_PTR(d_out); MODET_CHECK_PTR(d_vec);
  MODET_CHECK_DIM(args_ok(B, D, H, W, nsteps) && bound_ok(bound));
  if (nsteps >= 2) { MODET_CHECK_PTR(steps); MODET_CHECK_PTR(scratch); }
  const BwdWs w = bwd_ws(B, D, H, W, nsteps, bound);
  if (w.bytes) {
    MODET_CHECK_PTR(ws);
    if (ws_bytes < w.bytes || ((uintptr_t)ws & 7) != 0) return MODET_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const unsigned nvox = (unsigned)B * D * H * W;
  const size_t F = (size_t)nvox * 3;
  if (nsteps == 0) {
    hipLaunchKernelGGL(vecint_scale_kernel, dim3(flat_grid((int64_t)F, BLK)), dim3(BLK), 0, s, d_out, d_vec, (unsigned)F, 1.f);
    return modet_launch_status();
  }
  const int kg = first_general(nsteps, bound);
  const int tx = cdiv(W, TX), ty = cdiv(H, TY), tz = cdiv(D, TZ);
  float* ds = (float*)ws;
  const float* g = d_out;
  for (int k = nsteps - 1; k >= 0; --k) {
    const float* in = k == 0 ? vec : steps + (size_t)(k - 1) * F;
    const float scale = k == 0 ? ldexpf(1.f, -nsteps) : 1.f;
    float* dst = (k & 1) ? scratch : d_vec;                            // ends in d_vec at k = 0; g is never dst
    if (k < kg) {
      hipLaunchKernelGGL(vecint_bwd_bounded_kernel, dim3(tx * ty * tz, B), dim3(BLK), 0, s, in, g, dst, D, H, W, tx, ty, scale);
    } else {
      const float* v = in;                                             // the field the scatter runs on: v_k itself
      if (k == 0) {
        float* v0 = (float*)((char*)ws + w.v0_off);
        hipLaunchKernelGGL(vecint_scale_kernel, dim3(flat_grid((int64_t)F, BLK)), dim3(BLK), 0, s, vec, v0, (unsigned)F, scale);
        v = v0;
      }
      void* sub = (char*)ws + w.sub_off;
      const int rc = w.tiles ? modet_warp_bwd_dsrc_tiles(v, g, ds, sub, w.sub_bytes, B, D, H, W, 3, stream)
                             : modet_warp_bwd_det(v, 0, v, g, ds, nullptr, nullptr, sub, w.sub_bytes, B, D, H, W, 3, 0, stream);
      if (rc != MODET_OK) return rc;
      hipLaunchKernelGGL(vecint_bwd_general_kernel, dim3(flat_grid(nvox, BLK)), dim3(BLK), 0, s, in, g, (const float*)ds, dst, D,
                         H, W, nvox, scale);
    }
    g = dst;
  }
  return modet_launch_status();
}

}  // extern "C"
