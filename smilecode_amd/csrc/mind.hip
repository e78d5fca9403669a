// MIND-SSC descriptor, the MIND loss and its gradient (reference Baseline methods/RCN/losses.py:333-399; include/modet_hip_losses.h
// has the definition).  The reference runs ~20 ATen launches per image over 12-channel volumes and reads two bounds back to
// the host; here an image goes through
//   mind_ssd_kernel     image tile (reach 4) in LDS -> per channel: d^2 on the tile + reach 2, separable 5^3 box sum through two
//                       LDS buffers -> m_c = ssd_c - min (12 planes) + one partial sum of v = mean_c m_c per workgroup
//   mind_bounds_kernel  g = fixed-order fp64 sum of the partials / N -> the clamp bounds {0.001 g, 1000 g}, in device memory
// and a pair of images through
//   mind_point_kernel   both m tensors -> loss partials and G_c = d loss / d ssd_c of the differentiated image (exp, clamp mask,
//                       channel mean, argmin routing), written over that image's m
//   mind_adjoint_kernel G tile (reach 2) -> adjoint of the clamped box sum (the replicated border folded back as integer
//                       weights) -> E_c = 2/125 A_c d_c, summed with sign per NEIGHBOUR: F_k = sum_{c: i_c = k} E_c - sum_{c: j_c = k} E_c
//   mind_gather_kernel  adjoint of the six clamped shifts in gather form: voxel u collects F_k from the at most three source
//                       positions whose clamped shift lands on u
// Every sum has a fixed order (no atomics): two runs are bit-identical.  fp32 storage and accumulation; the two scalar
// reductions finish in fp64.  m is STORED, not recomputed: 48 B per voxel and image (DESIGN.md section 4.4 has the byte count).
#include "common.h"
#include "../../include/modet_hip_losses.h"

namespace {

constexpr int BLK = 256;
constexpr int TZ = 8, TY = 8, TX = 32;                       // output tile: thread (x = tid & 31, y = tid >> 5) owns a z column of 8
constexpr int RZ = TZ + 4, RY = TY + 4, RX = TX + 4;         // + the box's reach of 2
constexpr int IZ = TZ + 8, IY = TY + 8, IX = TX + 8;         // + the dilated neighbours' reach of 2
constexpr int NCH = 12, NNB = 6;
static_assert(TX * TY == BLK, "one thread per (y, x) column of the tile");

struct Dims { int B, D, H, W; };

// neighbour k: axis (0 = z, 1 = y, 2 = x) and direction of its shift of two voxels
__device__ __forceinline__ constexpr int nb_axis(int k) { constexpr int t[NNB] = {0, 2, 1, 2, 0, 1}; return t[k]; }
__device__ __forceinline__ constexpr int nb_sign(int k) { constexpr int t[NNB] = {-1, -1, -1, 1, 1, 1}; return t[k]; }
__device__ __forceinline__ constexpr int ch_i(int c) { constexpr int t[NCH] = {1, 2, 2, 3, 3, 4, 4, 4, 5, 5, 5, 5}; return t[c]; }
__device__ __forceinline__ constexpr int ch_j(int c) { constexpr int t[NCH] = {0, 0, 1, 0, 2, 1, 2, 3, 0, 1, 3, 4}; return t[c]; }
// the reference's final channel permutation: output channel k = channel out_perm(k) of the order above
__device__ __forceinline__ constexpr int out_perm(int k) { constexpr int t[NCH] = {6, 8, 1, 11, 2, 10, 0, 7, 9, 4, 5, 3}; return t[k]; }

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// v = mean_c m_c, the one association every kernel uses (the pointwise pass recomputes what the descriptor pass summed)
__device__ __forceinline__ float channel_mean(const float (&m)[NCH]) {
  float s = m[0];
#pragma unroll
  for (int c = 1; c < NCH; ++c) s += m[c];
  return s / (float)NCH;
}

// weight of source p in the adjoint of the clamped 5-box at q along an axis of n voxels: the number of offsets o in [-2, 2]
// with clamp(p + o) = q, for |p - q| <= 2 (p outside the axis meets a zero in the tile: any finite weight does)
__device__ __forceinline__ float adj_weight(int q, int p, int n) {
  int w = 1;
  if (q == 0) w += max(0, 2 - p);
  if (q == n - 1) w += max(0, 2 - (n - 1 - p));
  return (float)w;
}

__device__ __forceinline__ void tile_origin(int blk, int tiles_x, int tiles_y, int tiles_z, int& b, int& z0, int& y0, int& x0) {
  x0 = (blk % tiles_x) * TX; blk /= tiles_x;
  y0 = (blk % tiles_y) * TY; blk /= tiles_y;
  z0 = (blk % tiles_z) * TZ;
  b = blk / tiles_z;
}

// The separable 5^3 sum over a tile in LDS: b0 [RZ][RY][RX] -> (x) b1 [RZ][RY][TX] -> (y) b0 [RZ][TY][TX] -> (z) out[TZ] of this
// thread's column.  ADJ: the sums carry the border weights of the box's adjoint (q = the output's global coordinate).
// Ends with a barrier: b0 may be refilled right away.
template <bool ADJ>
__device__ __forceinline__ void box5_tile(float* __restrict__ b0, float* __restrict__ b1, float (&out)[TZ], const Dims d, int z0,
                                          int y0, int x0) {
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll 2
  for (int e = tid; e < RZ * RY * TX; e += BLK) {
    const int x = e % TX, row = e / TX;
    const float* s = b0 + row * RX + x;
    float acc;
    if constexpr (ADJ) {
      const int q = x0 + x;
      acc = adj_weight(q, q - 2, d.W) * s[0];
#pragma unroll
      for (int t = 1; t < 5; ++t) acc = fmaf(adj_weight(q, q - 2 + t, d.W), s[t], acc);
    } else {
      acc = (((s[0] + s[1]) + s[2]) + s[3]) + s[4];
    }
    b1[e] = acc;
  }
  __syncthreads();
#pragma unroll 2
  for (int e = tid; e < RZ * TY * TX; e += BLK) {
    const int x = e % TX, t1 = e / TX, y = t1 % TY, rz = t1 / TY;
    const float* s = b1 + (rz * RY + y) * TX + x;
    float acc;
    if constexpr (ADJ) {
      const int q = y0 + y;
      acc = adj_weight(q, q - 2, d.H) * s[0];
#pragma unroll
      for (int t = 1; t < 5; ++t) acc = fmaf(adj_weight(q, q - 2 + t, d.H), s[t * TX], acc);
    } else {
      acc = (((s[0] + s[TX]) + s[2 * TX]) + s[3 * TX]) + s[4 * TX];
    }
    b0[e] = acc;
  }
  __syncthreads();
  {
    float col[RZ];
#pragma unroll
    for (int k = 0; k < RZ; ++k) col[k] = b0[k * TY * TX + tid];       // tid = y * TX + x
#pragma unroll
    for (int k = 0; k < TZ; ++k) {
      if constexpr (ADJ) {
        const int q = z0 + k;
        float acc = adj_weight(q, q - 2, d.D) * col[k];
#pragma unroll
        for (int t = 1; t < 5; ++t) acc = fmaf(adj_weight(q, q - 2 + t, d.D), col[k + t], acc);
        out[k] = acc;
      } else {
        out[k] = (((col[k] + col[k + 1]) + col[k + 2]) + col[k + 3]) + col[k + 4];
      }
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ descriptor pass
// m (B,12,D,H,W): m_c = ssd_c - min_c ssd_c in the channel order of the header; part[blockIdx.x] = this tile's sum of v.
__global__ __launch_bounds__(BLK) void mind_ssd_kernel(const float* __restrict__ img, float* __restrict__ m, float* __restrict__ part,
                                                       const Dims d, int tiles_x, int tiles_y, int tiles_z) {
  __shared__ float simg[IZ * IY * IX];            // I(clamp(u)) for u in [tile - 4, tile + T + 4)
  __shared__ float b0[RZ * RY * RX];
  __shared__ float b1[RZ * RY * TX];
  __shared__ float red[BLK / 64];
  const int tid = threadIdx.x;
  int b, z0, y0, x0;
  tile_origin(blockIdx.x, tiles_x, tiles_y, tiles_z, b, z0, y0, x0);
  const int64_t DHW = (int64_t)d.D * d.H * d.W;
  const float* I = img + (int64_t)b * DHW;
  for (int e = tid; e < IZ * IY * IX; e += BLK) {
    const int ix = e % IX, t1 = e / IX, iy = t1 % IY, iz = t1 / IY;
    const int z = clampi(z0 - 4 + iz, d.D), y = clampi(y0 - 4 + iy, d.H), x = clampi(x0 - 4 + ix, d.W);
    simg[e] = I[((int64_t)z * d.H + y) * d.W + x];
  }
  // (box5_tile starts with a barrier)
  float ssd[NCH][TZ];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    constexpr int stride[3] = {IY * IX, IX, 1};
    const int oi = 2 * nb_sign(ch_i(c)) * stride[nb_axis(ch_i(c))], oj = 2 * nb_sign(ch_j(c)) * stride[nb_axis(ch_j(c))];
    if (c == 0) __syncthreads();                  // simg complete before the first fill reads it
    // d_c^2 at q = clamp(r) for every r of the tile + 2: q stays inside [tile - 2, tile + T + 2), q + shift inside simg
#pragma unroll 2
    for (int e = tid; e < RZ * RY * RX; e += BLK) {
      const int rx = e % RX, t1 = e / RX, ry = t1 % RY, rz = t1 / RY;
      const int qz = clampi(z0 - 2 + rz, d.D) - (z0 - 4), qy = clampi(y0 - 2 + ry, d.H) - (y0 - 4), qx = clampi(x0 - 2 + rx, d.W) - (x0 - 4);
      const int s = (qz * IY + qy) * IX + qx;
      const float dd = simg[s + oi] - simg[s + oj];
      b0[e] = dd * dd;
    }
    float o[TZ];
    box5_tile<false>(b0, b1, o, d, z0, y0, x0);
#pragma unroll
    for (int k = 0; k < TZ; ++k) ssd[c][k] = o[k] / 125.f;
  }
  const int x = x0 + (tid & (TX - 1)), y = y0 + tid / TX;
  float lsum = 0.f;
#pragma unroll
  for (int k = 0; k < TZ; ++k) {
    const int z = z0 + k;
    float mn = ssd[0][k];
#pragma unroll
    for (int c = 1; c < NCH; ++c) mn = fminf(mn, ssd[c][k]);
    float mc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) mc[c] = ssd[c][k] - mn;
    if (z < d.D && y < d.H && x < d.W) {
      lsum += channel_mean(mc);
      const int64_t o = (int64_t)b * NCH * DHW + ((int64_t)z * d.H + y) * d.W + x;
#pragma unroll
      for (int c = 0; c < NCH; ++c) m[o + c * DHW] = mc[c];
    }
  }
  const float r = block_sum(lsum, red);
  if (tid == 0) part[blockIdx.x] = r;
}

// bnd[0] = 0.001 g, bnd[1] = 1000 g with g = sum(part) / N: fp64, fixed order, one workgroup
__global__ __launch_bounds__(BLK) void mind_bounds_kernel(const float* __restrict__ part, int n, double inv_n, float* __restrict__ bnd) {
  __shared__ double sm[BLK];
  const double r = fixed_order_sum<BLK>(part, n, sm);
  if (threadIdx.x == 0) {
    const float g = (float)(r * inv_n);
    bnd[0] = g * 0.001f;
    bnd[1] = g * 1000.f;
  }
}

// ------------------------------------------------------------------------------------------------ pointwise passes
// descriptor: mind (B,12,D,H,W) in the reference's channel order
__global__ __launch_bounds__(BLK) void mind_exp_kernel(const float* __restrict__ m, const float* __restrict__ bnd, float* __restrict__ out,
                                                       int64_t N, int64_t DHW) {
  const float lo = bnd[0], hi = bnd[1];
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < N; i += (int64_t)gridDim.x * BLK) {
    const int64_t b = i / DHW, o = b * NCH * DHW + (i - b * DHW);
    float mc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) mc[c] = m[o + c * DHW];
    const float vc = fminf(fmaxf(channel_mean(mc), lo), hi);
#pragma unroll
    for (int k = 0; k < NCH; ++k) out[o + k * DHW] = expf(-(mc[out_perm(k)] / vc));
  }
}

// loss partials of mean (mind(x) - mind(a))^2 and, when GRAD, G_c = grad_scale * d loss / d ssd_c(x), written OVER mx (each thread
// reads its voxel's twelve values before it writes them).  bnd = {lo_a, hi_a, lo_x, hi_x}; gcoef = 2 grad_scale / (12 N).
template <bool GRAD>
__global__ __launch_bounds__(BLK) void mind_point_kernel(const float* __restrict__ ma, float* __restrict__ mx, const float* __restrict__ bnd,
                                                         float* __restrict__ part, int64_t N, int64_t DHW, float gcoef) {
  __shared__ float red[BLK / 64];
  const float lo_a = bnd[0], hi_a = bnd[1], lo_x = bnd[2], hi_x = bnd[3];
  float lsum = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < N; i += (int64_t)gridDim.x * BLK) {
    const int64_t b = i / DHW, o = b * NCH * DHW + (i - b * DHW);
    float a[NCH], x[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) { a[c] = ma[o + c * DHW]; x[c] = mx[o + c * DHW]; }
    const float va = channel_mean(a), vx = channel_mean(x);
    const float vca = fminf(fmaxf(va, lo_a), hi_a), vcx = fminf(fmaxf(vx, lo_x), hi_x);
    float q[NCH], ex[NCH], diff[NCH];
    float vsum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      q[c] = x[c] / vcx;
      ex[c] = expf(-q[c]);
      diff[c] = ex[c] - expf(-(a[c] / vca));
      vsum = fmaf(diff[c], diff[c], vsum);
    }
    lsum += vsum;
    if constexpr (GRAD) {
      // e = exp(-q), q = m / vc:  d/dq_c = -ge_c e_c;  d/dm_c = (d/dq_c) / vc + [lo <= v <= hi] (1/12) d/dvc,  d/dvc = -sum_c (d/dq_c) q_c / vc
      float gq[NCH];
      float dv = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        gq[c] = -(gcoef * diff[c]) * ex[c];
        dv = fmaf(gq[c], q[c], dv);
      }
      const float gv = (vx >= lo_x && vx <= hi_x) ? -dv / vcx / (float)NCH : 0.f;
      float gm[NCH];
      float gs = 0.f;
      int amin = NCH;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        gm[c] = gq[c] / vcx + gv;
        gs += gm[c];
        if (amin == NCH && x[c] == 0.f) amin = c;            // m_c = ssd_c - min: exactly 0 at the minimum; the lowest index wins a tie
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) mx[o + c * DHW] = gm[c] - (c == amin ? gs : 0.f);
    }
  }
  const float r = block_sum(lsum, red);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// ------------------------------------------------------------------------------------------------ adjoint passes
// G (B,12,D,H,W) -> F (B,6,D,H,W): F_k(q) = sum_c [i_c = k] E_c(q) - [j_c = k] E_c(q),  E_c = (2/125) A_c d_c,
// A_c(q) = sum over (p, o) with clamp(p + o) = q of G_c(p)  (the box sum's adjoint, separable, integer border weights)
__global__ __launch_bounds__(BLK) void mind_adjoint_kernel(const float* __restrict__ G, const float* __restrict__ img, float* __restrict__ F,
                                                           const Dims d, int tiles_x, int tiles_y, int tiles_z) {
  __shared__ float b0[RZ * RY * RX];
  __shared__ float b1[RZ * RY * TX];
  const int tid = threadIdx.x;
  int b, z0, y0, x0;
  tile_origin(blockIdx.x, tiles_x, tiles_y, tiles_z, b, z0, y0, x0);
  const int64_t DHW = (int64_t)d.D * d.H * d.W;
  const float* I = img + (int64_t)b * DHW;
  const int x = x0 + (tid & (TX - 1)), y = y0 + tid / TX;
  const int xc = clampi(x, d.W), yc = clampi(y, d.H);             // (columns past the volume compute on clamped addresses, write nothing)
  // S_k(q) = I(clamp(q + shift_k)) for this thread's column
  float S[NNB][TZ];
#pragma unroll
  for (int k = 0; k < NNB; ++k) {
#pragma unroll
    for (int t = 0; t < TZ; ++t) {
      const int zc = clampi(z0 + t, d.D);
      const int zz = nb_axis(k) == 0 ? clampi(zc + 2 * nb_sign(k), d.D) : zc;
      const int yy = nb_axis(k) == 1 ? clampi(yc + 2 * nb_sign(k), d.H) : yc;
      const int xx = nb_axis(k) == 2 ? clampi(xc + 2 * nb_sign(k), d.W) : xc;
      S[k][t] = I[((int64_t)zz * d.H + yy) * d.W + xx];
    }
  }
  float Fk[NNB][TZ];
#pragma unroll
  for (int k = 0; k < NNB; ++k)
#pragma unroll
    for (int t = 0; t < TZ; ++t) Fk[k][t] = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const float* Gc = G + ((int64_t)b * NCH + c) * DHW;
#pragma unroll 2
    for (int e = tid; e < RZ * RY * RX; e += BLK) {
      const int rx = e % RX, t1 = e / RX, ry = t1 % RY, rz = t1 / RY;
      const int pz = z0 - 2 + rz, py = y0 - 2 + ry, px = x0 - 2 + rx;
      const bool in = pz >= 0 && pz < d.D && py >= 0 && py < d.H && px >= 0 && px < d.W;
      b0[e] = in ? Gc[((int64_t)pz * d.H + py) * d.W + px] : 0.f;
    }
    float A[TZ];
    box5_tile<true>(b0, b1, A, d, z0, y0, x0);
#pragma unroll
    for (int t = 0; t < TZ; ++t) {
      const float E = (2.f / 125.f) * A[t] * (S[ch_i(c)][t] - S[ch_j(c)][t]);
      Fk[ch_i(c)][t] += E;
      Fk[ch_j(c)][t] -= E;
    }
  }
  if (y < d.H && x < d.W) {
#pragma unroll
    for (int t = 0; t < TZ; ++t) {
      const int z = z0 + t;
      if (z >= d.D) break;
      const int64_t o = (int64_t)b * NNB * DHW + ((int64_t)z * d.H + y) * d.W + x;
#pragma unroll
      for (int k = 0; k < NNB; ++k) F[o + k * DHW] = Fk[k][t];
    }
  }
}

// sum of f over the positions q along an axis of n voxels (stride st) with clamp(q + 2 sign) = u, in ascending q
__device__ __forceinline__ float gather_axis(const float* __restrict__ f, int u, int n, int64_t st, int sign) {
  float s = 0.f;
  if (sign > 0) {
    if (u - 2 >= 0) s += f[(int64_t)(u - 2) * st];
    if (u == n - 1) {
      if (n - 2 >= 0) s += f[(int64_t)(n - 2) * st];
      s += f[(int64_t)(n - 1) * st];
    }
  } else {
    if (u == 0) {
      s += f[0];
      if (1 <= n - 1) s += f[st];
    }
    if (u + 2 <= n - 1) s += f[(int64_t)(u + 2) * st];
  }
  return s;
}

// d_img(u) = sum_k sum_{q : clamp(q + shift_k) = u} F_k(q)
__global__ __launch_bounds__(BLK) void mind_gather_kernel(const float* __restrict__ F, float* __restrict__ dimg, const Dims d, int64_t N) {
  const int64_t HW = (int64_t)d.H * d.W, DHW = HW * d.D;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < N; i += (int64_t)gridDim.x * BLK) {
    const int64_t b = i / DHW, r = i - b * DHW;
    const int z = (int)(r / HW), y = (int)((r - z * HW) / d.W), x = (int)(r - z * HW - (int64_t)y * d.W);
    const float* Fb = F + b * NNB * DHW;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < NNB; ++k) {
      const float* f = Fb + k * DHW;
      if (nb_axis(k) == 0) acc += gather_axis(f + (int64_t)y * d.W + x, z, d.D, HW, nb_sign(k));
      else if (nb_axis(k) == 1) acc += gather_axis(f + (int64_t)z * HW + x, y, d.H, d.W, nb_sign(k));
      else acc += gather_axis(f + (int64_t)z * HW + (int64_t)y * d.W, x, d.W, 1, nb_sign(k));
    }
    dimg[i] = acc;
  }
}

struct Plan { int tiles_x, tiles_y, tiles_z, tiles, pgrid; int64_t N; };
inline Plan make_plan(int B, int D, int H, int W) {
  Plan p;
  p.tiles_x = cdiv(W, TX); p.tiles_y = cdiv(H, TY); p.tiles_z = cdiv(D, TZ);
  p.N = (int64_t)B * D * H * W;
  const int64_t t = (int64_t)B * p.tiles_x * p.tiles_y * p.tiles_z;
  p.tiles = t < (1ll << 30) ? (int)t : -1;
  p.pgrid = flat_grid(p.N, BLK) < 2048 ? flat_grid(p.N, BLK) : 2048;
  return p;
}
inline bool dims_ok(int B, int D, int H, int W) {
  return B > 0 && D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < (1ll << 31) && make_plan(B, D, H, W).tiles > 0;
}
constexpr int SCALARS = 64;      // floats kept for the clamp bounds

}  // namespace

extern "C" {

size_t modet_mind_ws_bytes(int B, int D, int H, int W, int images) {
  if (!dims_ok(B, D, H, W) || images < 1 || images > 2) return 0;
  const Plan p = make_plan(B, D, H, W);
  // per image: m (12 volumes) + one partial of v per tile;  the loss partials;  the bounds
  return ((size_t)images * ((size_t)NCH * p.N + p.tiles) + 2048 + SCALARS) * sizeof(float);
}

int modet_mind_descriptor(const float* img, float* mind, void* ws, size_t ws_bytes, int B, int D, int H, int W, int radius,
                          int dilation, modet_stream_t stream) {
  MODET_CHECK_PTR(img); MODET_CHECK_PTR(mind); MODET_CHECK_PTR(ws);
  MODET_CHECK_DIM(dims_ok(B, D, H, W));
  if (radius != 2 || dilation != 2) return MODET_ERR_UNSUPPORTED;
  if (ws_bytes < modet_mind_ws_bytes(B, D, H, W, 1)) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Dims d{B, D, H, W};
  const Plan p = make_plan(B, D, H, W);
  float* m = (float*)ws;
  float* part = m + (size_t)NCH * p.N;
  float* bnd = part + p.tiles + 2048;
  hipLaunchKernelGGL(mind_ssd_kernel, dim3(p.tiles), dim3(BLK), 0, s, img, m, part, d, p.tiles_x, p.tiles_y, p.tiles_z);
  hipLaunchKernelGGL(mind_bounds_kernel, dim3(1), dim3(BLK), 0, s, (const float*)part, p.tiles, 1.0 / (double)p.N, bnd);
  hipLaunchKernelGGL(mind_exp_kernel, dim3(p.pgrid), dim3(BLK), 0, s, (const float*)m, (const float*)bnd, mind, p.N, p.N / B);
  return modet_launch_status();
}

int modet_mind_fwd_bwd(const float* a, const float* b, float* loss, float* d_b, void* ws, size_t ws_bytes, int B, int D, int H,
                       int W, int radius, int dilation, float grad_scale, modet_stream_t stream) {
  MODET_CHECK_PTR(a); MODET_CHECK_PTR(b); MODET_CHECK_PTR(loss); MODET_CHECK_PTR(ws);
  MODET_CHECK_DIM(dims_ok(B, D, H, W));
  if (radius != 2 || dilation != 2) return MODET_ERR_UNSUPPORTED;
  if (ws_bytes < modet_mind_ws_bytes(B, D, H, W, 2)) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Dims d{B, D, H, W};
  const Plan p = make_plan(B, D, H, W);
  float* ma = (float*)ws;
  float* mb = ma + (size_t)NCH * p.N;
  float* part_a = mb + (size_t)NCH * p.N;
  float* part_b = part_a + p.tiles;
  float* part_l = part_b + p.tiles;
  float* bnd = part_l + 2048;
  hipLaunchKernelGGL(mind_ssd_kernel, dim3(p.tiles), dim3(BLK), 0, s, a, ma, part_a, d, p.tiles_x, p.tiles_y, p.tiles_z);
  hipLaunchKernelGGL(mind_bounds_kernel, dim3(1), dim3(BLK), 0, s, (const float*)part_a, p.tiles, 1.0 / (double)p.N, bnd);
  hipLaunchKernelGGL(mind_ssd_kernel, dim3(p.tiles), dim3(BLK), 0, s, b, mb, part_b, d, p.tiles_x, p.tiles_y, p.tiles_z);
  hipLaunchKernelGGL(mind_bounds_kernel, dim3(1), dim3(BLK), 0, s, (const float*)part_b, p.tiles, 1.0 / (double)p.N, bnd + 2);
  const double n_all = (double)NCH * (double)p.N;
  const float gcoef = (float)(2.0 * (double)grad_scale / n_all);
  if (d_b)
    hipLaunchKernelGGL((mind_point_kernel<true>), dim3(p.pgrid), dim3(BLK), 0, s, (const float*)ma, mb, (const float*)bnd, part_l, p.N,
                       p.N / B, gcoef);
  else
    hipLaunchKernelGGL((mind_point_kernel<false>), dim3(p.pgrid), dim3(BLK), 0, s, (const float*)ma, mb, (const float*)bnd, part_l, p.N,
                       p.N / B, gcoef);
  hipLaunchKernelGGL(scalar_finalize_kernel<float>, dim3(1), dim3(BLK), 0, s, (const float*)part_l, p.pgrid, 1.0 / n_all, loss);
  if (d_b) {
    float* F = ma;                                // m(a) is consumed: its first six volumes per sample take F
    hipLaunchKernelGGL(mind_adjoint_kernel, dim3(p.tiles), dim3(BLK), 0, s, (const float*)mb, b, F, d, p.tiles_x, p.tiles_y, p.tiles_z);
    hipLaunchKernelGGL(mind_gather_kernel, dim3(p.pgrid), dim3(BLK), 0, s, (const float*)F, d_b, d, p.N);
  }
  return modet_launch_status();
}

}  // extern "C"
