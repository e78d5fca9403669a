// The label-overlap (soft Dice) training term of include/modet_hip_segdice.h: the moving labels warped trilinearly by the flow
// against the fixed labels, without the one-hot volume the ATen composition (one_hot -> grid_sample -> per-label sums) builds.
//
// At a voxel at most eight labels have a non-zero weight, so the forward is three per-label sums and the backward a gather with a
// per-label coefficient table; both read the 12-byte flow, the 2-byte fixed label and eight 2-byte moving labels per voxel.
//
//   segdice_sums_kernel    one visit per voxel; the corner weights in 64-bit fixed point (2^-32), equal labels combined per voxel
//                          and, where a whole wave sees one label (the inside of a region), across the wave, then integer LDS
//                          atomics; one row of 3 (L+1) sums per workgroup in the workspace.  Integer sums: any order, same bits.
//   segdice_colsum_kernel  the column sums of the workgroups' rows -> the (B,3,L+1) float64 table [I, P, T]
//   segdice_finalize_kernel  the fp32 loss and the two fp32 coefficients per label (one workgroup, fp64, fixed order)
//   segdice_grad_kernel    the coefficients of the batch item in LDS; per voxel a gather of the eight corner labels: no scatter
//
// No FMA contraction in this file: the sums and the gradient pass form the same weights, and "add into" is the separate write
// followed by one fp32 addition, bit for bit.
#include "common.h"

#include "../../include/modet_hip_segdice.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;
constexpr int MAX_WG = 1024;                        // workgroups of the sums launch over all batch items: rows of the workspace
constexpr int MAXL1 = MODET_SEGDICE_MAX_LABELS + 1;
constexpr float FIX_ONE = 4294967296.f;             // 2^32
typedef unsigned long long u64;

struct Corner8 {
  float wz[2], wy[2], wx[2];     // wz[0] = 1 - fz, wz[1] = fz
  int m[8];                      // the moving label at corner 4 dz + 2 dy + dx, 0 = outside the volume or not in 1..L
};

// the flow of voxel v (of V) in either layout
template <bool CL>
__device__ __forceinline__ void load_flow(const float* __restrict__ fl, int64_t v, int64_t V, float (&f)[3]) {
  if (CL) { f[0] = fl[v * 3]; f[1] = fl[v * 3 + 1]; f[2] = fl[v * 3 + 2]; }
  else { f[0] = fl[v]; f[1] = fl[V + v]; f[2] = fl[2 * V + v]; }
}

// false: the voxel lands outside the volume with all eight corners, or a flow component is not finite (no comparison with NaN
// holds; +-inf fails one).  p in [-1, n) while it is a float, so the base corner is in [-1, n - 1] as an int.
__device__ __forceinline__ bool gather_corners(const int16_t* __restrict__ lm, int z, int y, int x, const float (&f)[3], int D, int H,
                                               int W, int L, Corner8& c) {
  const float pz = (float)z + f[0], py = (float)y + f[1], px = (float)x + f[2];
  const bool in = pz >= -1.f && pz < (float)D && py >= -1.f && py < (float)H && px >= -1.f && px < (float)W;
  if (!in) return false;
  const float z0 = floorf(pz), y0 = floorf(py), x0 = floorf(px);
  const float fz = pz - z0, fy = py - y0, fx = px - x0;
  c.wz[0] = 1.f - fz; c.wz[1] = fz; c.wy[0] = 1.f - fy; c.wy[1] = fy; c.wx[0] = 1.f - fx; c.wx[1] = fx;
  const int iz = (int)z0, iy = (int)y0, ix = (int)x0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int cz = iz + (k >> 2), cy = iy + ((k >> 1) & 1), cx = ix + (k & 1);
    const bool ok = cz >= 0 && cz < D && cy >= 0 && cy < H && cx >= 0 && cx < W;
    int m = 0;
    if (ok) m = lm[((int64_t)cz * H + cy) * W + cx];
    c.m[k] = (m >= 1 && m <= L) ? m : 0;
  }
  return true;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
  unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned olo = __shfl_xor(lo, o, 64), ohi = __shfl_xor(hi, o, 64);
    v += ((u64)ohi << 32) | olo;
    lo = (unsigned)v; hi = (unsigned)(v >> 32);
  }
  return v;
}

// grid (G, B).  part[(b G + g)][3][L1] = this workgroup's fixed-point sums [I, P, T]; every column is written.
template <bool CL>
__global__ __launch_bounds__(BLK) void segdice_sums_kernel(const int16_t* __restrict__ mov, const float* __restrict__ flow,
                                                           const int16_t* __restrict__ fix, u64* __restrict__ part, int D, int H,
                                                           int W, int L) {
  __shared__ u64 acc[3 * MAXL1];
  const int L1 = L + 1, b = blockIdx.y;
  for (int i = threadIdx.x; i < 3 * L1; i += BLK) acc[i] = 0ull;
  __syncthreads();
  const int64_t V = (int64_t)D * H * W;
  const int16_t* lm = mov + (int64_t)b * V;
  const int16_t* lf = fix + (int64_t)b * V;
  const float* fl = flow + (int64_t)b * V * 3;
  u64* aI = acc; u64* aP = acc + L1; u64* aT = acc + 2 * L1;
  const int lane = threadIdx.x & 63;
  // every lane of a wave runs the same number of rounds (the wave-wide steps below need all of them); `live` marks a voxel
  for (int64_t v0 = (int64_t)blockIdx.x * BLK; v0 < V; v0 += (int64_t)gridDim.x * BLK) {
    const int64_t v = v0 + threadIdx.x;
    const bool live = v < V;
    int tl = 0;
    int m[8];
    u64 q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { m[k] = 0; q[k] = 0ull; }
    if (live) {
      const unsigned vox = (unsigned)v;
      const unsigned t1 = vox / (unsigned)W, t2 = t1 / (unsigned)H;
      const int x = (int)(vox - t1 * (unsigned)W), y = (int)(t1 - t2 * (unsigned)H), z = (int)t2;
      const int t = lf[v];
      tl = (t >= 1 && t <= L) ? t : 0;
      float f[3];
      load_flow<CL>(fl, v, V, f);
      Corner8 c;
      if (gather_corners(lm, z, y, x, f, D, H, W, L, c)) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float w = (c.wz[k >> 2] * c.wy[(k >> 1) & 1]) * c.wx[k & 1];
          const u64 qk = __float2ull_rn(w * FIX_ONE);
          m[k] = qk ? c.m[k] : 0;
          q[k] = qk;
        }
      }
    }
    // equal labels of the voxel combined: m[k] != 0 afterwards only at the first corner of each distinct label
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
      for (int j = k + 1; j < 8; ++j) {
        const bool same = m[k] != 0 && m[j] == m[k];
        q[k] += same ? q[j] : 0ull;
        m[j] = same ? 0 : m[j];
      }
    int n = 0, first = 0;
    u64 qf = 0ull;
#pragma unroll
    for (int k = 7; k >= 0; --k)
      if (m[k]) { ++n; first = m[k]; qf = q[k]; }
    // the inside of a region: every voxel of the wave sees one and the same label -> one pair of atomics per wave
    const u64 has = __ballot(n > 0);
    if (has) {
      const int lab0 = __shfl(first, __ffsll((long long)has) - 1, 64);
      if (__all(n == 0 || (n == 1 && first == lab0))) {
        const u64 sp = wave_sum_u64(n ? qf : 0ull);
        const u64 si = wave_sum_u64((n && first == tl) ? qf : 0ull);
        if (lane == 0) {
          atomicAdd(&aP[lab0], sp);
          if (si) atomicAdd(&aI[lab0], si);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (m[k]) {
            atomicAdd(&aP[m[k]], q[k]);
            if (m[k] == tl) atomicAdd(&aI[m[k]], q[k]);
          }
      }
    }
    const u64 hasT = __ballot(tl != 0);
    if (hasT) {
      const int t0 = __shfl(tl, __ffsll((long long)hasT) - 1, 64);
      if (__all(tl == 0 || tl == t0)) {
        if (lane == 0) atomicAdd(&aT[t0], (u64)__popcll(hasT) << 32);
      } else if (tl) {
        atomicAdd(&aT[tl], 1ull << 32);
      }
    }
  }
  __syncthreads();
  u64* row = part + ((int64_t)b * gridDim.x + blockIdx.x) * (3 * L1);
  for (int i = threadIdx.x; i < 3 * L1; i += BLK) row[i] = acc[i];
}

// grid (cdiv(3 L1, 32), B), 256 threads = 8 row lanes x 32 columns.  table[b][col] = (sum over the G rows) / 2^32
__global__ __launch_bounds__(BLK) void segdice_colsum_kernel(const u64* __restrict__ part, double* __restrict__ table, int G, int ncol) {
  __shared__ u64 sm[BLK];
  const int b = blockIdx.y, cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cl;
  u64 s = 0ull;
  if (col < ncol)
    for (int g = rl; g < G; g += 8) s += part[((int64_t)b * G + g) * ncol + col];
  sm[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0 && col < ncol) {
    u64 t = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += sm[k * 32 + cl];
    table[(int64_t)b * ncol + col] = (double)t * (1.0 / 4294967296.0);
  }
}

// one workgroup.  coef[b][0][m] = -(2 / (B L)) / S_m (the [m == f] term), coef[b][1][m] = (2 / (B L)) I_m / S_m^2; [.][0] = 0.
__global__ __launch_bounds__(BLK) void segdice_finalize_kernel(const double* __restrict__ table, float* __restrict__ coef,
                                                               float* __restrict__ loss, int B, int L) {
  __shared__ double sm[BLK];
  const int L1 = L + 1;
  const double k2 = 2.0 / ((double)B * (double)L);
  double s = 0.0;
  for (int i = threadIdx.x; i < B * L1; i += BLK) {
    const int b = i / L1, m = i - b * L1;
    const double* t = table + (int64_t)b * 3 * L1;
    float ca = 0.f, cc = 0.f;
    if (m >= 1) {
      const double I = t[m], S = t[L1 + m] + t[2 * L1 + m] + 1e-5;
      s += 2.0 * I / S;
      ca = (float)(-k2 / S);
      cc = (float)(k2 * I / (S * S));
    }
    coef[(int64_t)b * 2 * L1 + m] = ca;
    coef[(int64_t)b * 2 * L1 + L1 + m] = cc;
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    for (int i = 0; i < BLK; ++i) r += sm[i];
    loss[0] = (float)(1.0 - r / ((double)B * (double)L));
  }
}

// grid (G, B).  d_flow in the flow's layout: gs * sum_c (d t_c / d p_a) g(m_c, f), added to what is there when ADD.
template <bool CL, bool ADD>
__global__ __launch_bounds__(BLK) void segdice_grad_kernel(const int16_t* __restrict__ mov, const float* __restrict__ flow,
                                                           const int16_t* __restrict__ fix, const float* __restrict__ coef,
                                                           float* __restrict__ dflow, int D, int H, int W, int L, float gs) {
  __shared__ float tab[2 * MAXL1];
  const int L1 = L + 1, b = blockIdx.y;
  for (int i = threadIdx.x; i < 2 * L1; i += BLK) tab[i] = coef[(int64_t)b * 2 * L1 + i];
  __syncthreads();
  const int64_t V = (int64_t)D * H * W;
  const int16_t* lm = mov + (int64_t)b * V;
  const int16_t* lf = fix + (int64_t)b * V;
  const float* fl = flow + (int64_t)b * V * 3;
  float* df = dflow + (int64_t)b * V * 3;
  for (int64_t v = (int64_t)blockIdx.x * BLK + threadIdx.x; v < V; v += (int64_t)gridDim.x * BLK) {
    const unsigned vox = (unsigned)v;
    const unsigned t1 = vox / (unsigned)W, t2 = t1 / (unsigned)H;
    const int x = (int)(vox - t1 * (unsigned)W), y = (int)(t1 - t2 * (unsigned)H), z = (int)t2;
    const int tl = lf[v];                        // compared with labels in 1..L only: never an index
    float f[3];
    load_flow<CL>(fl, v, V, f);
    Corner8 c;
    float g[3] = {0.f, 0.f, 0.f};
    if (gather_corners(lm, z, y, x, f, D, H, W, L, c)) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int m = c.m[k];                    // 0 or in 1..L: tab[0] = tab[L1] = 0
        const float gk = (m == tl ? tab[m] : 0.f) + tab[L1 + m];
        const int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
        const float tz = (c.wy[dy] * c.wx[dx]) * gk, ty = (c.wz[dz] * c.wx[dx]) * gk, tx = (c.wz[dz] * c.wy[dy]) * gk;
        g[0] += dz ? tz : -tz;
        g[1] += dy ? ty : -ty;
        g[2] += dx ? tx : -tx;
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int64_t o = CL ? v * 3 + a : (int64_t)a * V + v;
      const float r = g[a] * gs;
      df[o] = ADD ? df[o] + r : r;
    }
  }
}

struct Plan { int64_t V; int G, L1; size_t part_bytes, coef_bytes; };
// a function of the shape and L alone; false for what the entry points refuse
inline bool make_plan(int B, int D, int H, int W, int L, Plan& p) {
  if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1 || L < 1 || L > MODET_SEGDICE_MAX_LABELS) return false;   // B: grid.y
  const double n = (double)B * D * H * W;
  if (n >= 2147483648.0) return false;
  p.V = (int64_t)D * H * W;
  p.L1 = L + 1;
  int64_t g = cdiv64(p.V, BLK);
  const int64_t cap = MAX_WG / B > 1 ? MAX_WG / B : 1;
  if (g > cap) g = cap;
  p.G = (int)g;
  p.part_bytes = (size_t)B * p.G * 3 * p.L1 * sizeof(u64);
  p.coef_bytes = (((size_t)B * 2 * p.L1 * sizeof(float)) + 15) & ~(size_t)15;
  return true;
}

int check(int B, int D, int H, int W, int L, const void* ws, size_t ws_bytes, Plan& p) {
  if (L < 1 || L > MODET_SEGDICE_MAX_LABELS) return MODET_ERR_UNSUPPORTED;
  MODET_CHECK_DIM(make_plan(B, D, H, W, L, p));
  if (ws_bytes < p.part_bytes + p.coef_bytes || ((uintptr_t)ws & 7) != 0) return MODET_ERR_WORKSPACE;
  return MODET_OK;
}

void launch_sums(const int16_t* mov, const float* flow, const int16_t* fix, double* table, u64* part, const Plan& p, int B, int D,
                 int H, int W, int L, int cl, hipStream_t s) {
  if (cl) hipLaunchKernelGGL(segdice_sums_kernel<true>, dim3(p.G, B), dim3(BLK), 0, s, mov, flow, fix, part, D, H, W, L);
  else hipLaunchKernelGGL(segdice_sums_kernel<false>, dim3(p.G, B), dim3(BLK), 0, s, mov, flow, fix, part, D, H, W, L);
  hipLaunchKernelGGL(segdice_colsum_kernel, dim3(cdiv(3 * p.L1, 32), B), dim3(BLK), 0, s, (const u64*)part, table, p.G, 3 * p.L1);
}

}  // namespace

extern "C" {

size_t modet_segdice_ws_bytes(int B, int D, int H, int W, int nlabels) {
  Plan p;
  if (!make_plan(B, D, H, W, nlabels, p)) return 0;
  return p.part_bytes + p.coef_bytes;
}

int modet_segdice_sums(const int16_t* mov_lab, const float* flow, const int16_t* fix_lab, double* table, void* ws, size_t ws_bytes,
                       int B, int D, int H, int W, int nlabels, int channels_last, modet_stream_t stream) {
  MODET_CHECK_PTR(mov_lab); MODET_CHECK_PTR(flow); MODET_CHECK_PTR(fix_lab); MODET_CHECK_PTR(table); MODET_CHECK_PTR(ws);
  Plan p;
  const int rc = check(B, D, H, W, nlabels, ws, ws_bytes, p);
  if (rc != MODET_OK) return rc;
  launch_sums(mov_lab, flow, fix_lab, table, (u64*)ws, p, B, D, H, W, nlabels, channels_last, (hipStream_t)stream);
  return modet_launch_status();
}

int modet_segdice_fwd_bwd(const int16_t* mov_lab, const float* flow, const int16_t* fix_lab, float* loss, double* table,
                          float* d_flow, void* ws, size_t ws_bytes, int B, int D, int H, int W, int nlabels, int channels_last,
                          float grad_scale, int add_into, modet_stream_t stream) {
  MODET_CHECK_PTR(mov_lab); MODET_CHECK_PTR(flow); MODET_CHECK_PTR(fix_lab); MODET_CHECK_PTR(loss); MODET_CHECK_PTR(table);
  MODET_CHECK_PTR(ws);
  Plan p;
  const int rc = check(B, D, H, W, nlabels, ws, ws_bytes, p);
  if (rc != MODET_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* coef = (float*)((char*)ws + p.part_bytes);
  launch_sums(mov_lab, flow, fix_lab, table, (u64*)ws, p, B, D, H, W, nlabels, channels_last, s);
  hipLaunchKernelGGL(segdice_finalize_kernel, dim3(1), dim3(BLK), 0, s, (const double*)table, coef, loss, B, nlabels);
  if (d_flow) {
    int g = flat_grid(p.V, BLK);
    const int cap = 4096 / B > 1 ? 4096 / B : 1;
    if (g > cap) g = cap;
#define SEG_GRAD(CL_, ADD_)                                                                                                     \
  hipLaunchKernelGGL((segdice_grad_kernel<CL_, ADD_>), dim3(g, B), dim3(BLK), 0, s, mov_lab, flow, fix_lab, (const float*)coef, \
                     d_flow, D, H, W, nlabels, grad_scale)
    if (channels_last) { if (add_into) SEG_GRAD(true, true); else SEG_GRAD(true, false); }
    else { if (add_into) SEG_GRAD(false, true); else SEG_GRAD(false, false); }
#undef SEG_GRAD
  }
  return modet_launch_status();
}

}  // extern "C"
