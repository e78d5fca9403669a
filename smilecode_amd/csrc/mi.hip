// Mutual information with Parzen windows, global and per patch (reference Baseline methods/RCN/losses.py:401-556;
// include/modet_hip_mi.h has the definition).  The ATen composition stores two (B, N, 32) weight tensors and runs a bmm over
// them; here the 32 weights of a voxel exist in registers only and both products run on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32: D[32][32] += A[32][2] B[2][32], bit for bit an fmaf chain).
//
//   global form
//   mi_hist_kernel      pab = sum_k I_a(k) (x) I_b(k): lane l supplies bin l & 31 of voxel l >> 5 for both operands, two voxels
//                       per instruction; the normaliser is a sum over the 32 lanes of a half.  A wave owns 1024 voxels, the
//                       four waves of a workgroup are added in wave order: one partial (pab, pa, pb) per 4096 voxels
//   mi_reduce_kernel    the partials of a batch element in 32 slices, fixed order, fp64
//   mi_final_kernel     the slices -> pab, pa, pb, the loss, and per batch element the two 32 x 32 matrices
//                       Gb[i][j] = d mi / d pab_ij + d mi / d pb_j and GaT[j][i] = d mi / d pab_ij + d mi / d pa_i (fp64 throughout)
//   mi_grad_kernel      U^T = Gb^T I_a^T per tile of 32 voxels: the OUTPUT has the voxel on the lane and 16 of the 32 bins in
//                       the registers, so the chain through normaliser, exp and clamp is register sums plus one exchange
//                       between the lane halves.  d_a the same with GaT and the images' roles swapped.
//   local form
//   lmi_kernel          one wave per patch: histogram as above into one accumulator tile (a second, transposed one when d_a
//                       is wanted), the tile's finalisation in registers -- it then IS the A operand of the gradient product
//                       (row i of the tile on register r of lane half h = k index of step r) -- and the gradient tiles
//   lmi_loss_kernel     the patches' mi in a fixed order, fp64
// Every sum has a fixed order (no atomics): two runs are bit-identical.
#include "common.h"
#include "../../include/modet_hip_mi.h"

#include <math.h>

namespace {

constexpr int NB = 32;                       // bins: the MFMA tile's edge
constexpr int BLK = 256, WAVES = BLK / 64;
constexpr int WAVE_VOX = 1024;               // voxels of a wave in the global passes: an fp32 chain of 512 per accumulator element
constexpr int CHUNK = WAVES * WAVE_VOX;      // voxels of a workgroup = voxels per partial
constexpr int PART = NB * NB + 2 * NB;       // floats of a partial: pab row-major, pa, pb
constexpr int SLICES = 32;
constexpr int MAX_PATCH = 16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

struct Params {
  float c[NB];        // bin centres
  float k2;           // -preterm * log2(e): w = exp2(k2 (x - c)^2)
  float maxval;
};

// row of the 32 x 32 accumulator tile that register r of lane half h holds (the column is lane & 31)
__device__ __forceinline__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ float clampv(float x, float maxval) { return fminf(fmaxf(x, 0.f), maxval); }
__device__ __forceinline__ bool clamp_passes(float x, float maxval) { return x >= 0.f && x <= maxval; }
__device__ __forceinline__ float weight(float x, float c, float k2) {
  const float d = x - c;
  return __builtin_amdgcn_exp2f(d * d * k2);
}
// sum over the 32 lanes of a wave half, the same value in all of them
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float other_half(float v) { return __shfl_xor(v, 32, 64); }
// lane half h takes the value of lane `l0 + h` (l0 a constant)
__device__ __forceinline__ float pick_pair(float v, int l0, int h) {
  const float v0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l0));
  const float v1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l0 + 1));
  return h ? v1 : v0;
}
__device__ __forceinline__ float centre_of_lane(const Params& P, int bin) {
  float c = 0.f;
#pragma unroll
  for (int q = 0; q < NB; ++q) c = bin == q ? P.c[q] : c;
  return c;
}

// 64 voxels into the histogram: xa / xb = this lane's clamped voxel, the first nvalid of the 64 exist.  The tail feeds zero
// WEIGHTS (a zero value would count as a voxel of value 0).  accT (TR) is the transposed tile: the same products, the same order.
template <bool TR>
__device__ __forceinline__ void hist_64(float xa, float xb, int nvalid, float cl, float k2, int h, f32x16& acc, f32x16& accT,
                                        float& pa, float& pb) {
#pragma unroll
  for (int s = 0; s < 32; ++s) {
    if (2 * s >= nvalid) break;
    const float va = pick_pair(xa, 2 * s, h), vb = pick_pair(xb, 2 * s, h);
    const float wa = weight(va, cl, k2), wb = weight(vb, cl, k2);
    const float sa = half_sum(wa), sb = half_sum(wb);
    const bool ok = 2 * s + h < nvalid;
    const float ia = ok ? wa * __builtin_amdgcn_rcpf(sa) : 0.f;
    const float ib = ok ? wb * __builtin_amdgcn_rcpf(sb) : 0.f;
    pa += ia;
    pb += ib;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ia, ib, acc, 0, 0, 0);
    if (TR) accT = __builtin_amdgcn_mfma_f32_32x32x2f32(ib, ia, accT, 0, 0, 0);
  }
}

// The gradient of 32 voxels (lane & 31 = the voxel, both halves hold it).  ra / rb: the raw values.  g*[r] = the matrix's row
// acc_row(r, h), column lane & 31 (the A operand of step r); cs[r] = the centre of bin acc_row(r, h).  The product's k index of
// step r and lane half h is bin acc_row(r, h) for both operands; the output tile has those same bins in its registers.
template <bool DA, bool DB>
__device__ __forceinline__ void grad_32(float ra, float rb, const float (&gA)[16], const float (&gB)[16], const float (&cs)[16],
                                        float k2, float maxval, float coef, float& da, float& db) {
  const float xa = clampv(ra, maxval), xb = clampv(rb, maxval);
  float wa[16], wb[16];
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    wa[r] = weight(xa, cs[r], k2);
    wb[r] = weight(xb, cs[r], k2);
    sa += wa[r];
    sb += wb[r];
  }
  sa += other_half(sa);
  sb += other_half(sb);
  const float ia = __builtin_amdgcn_rcpf(sa), ib = __builtin_amdgcn_rcpf(sb);
  if (DB) {
    f32x16 u = {0};
#pragma unroll
    for (int r = 0; r < 16; ++r) u = __builtin_amdgcn_mfma_f32_32x32x2f32(gB[r], wa[r] * ia, u, 0, 0, 0);
    float ubar = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) ubar += u[r] * wb[r];
    ubar += other_half(ubar);
    ubar *= ib;
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += (u[r] - ubar) * wb[r] * (xb - cs[r]);
    t += other_half(t);
    db = clamp_passes(rb, maxval) ? coef * t * ib : 0.f;
  }
  if (DA) {
    f32x16 u = {0};
#pragma unroll
    for (int r = 0; r < 16; ++r) u = __builtin_amdgcn_mfma_f32_32x32x2f32(gA[r], wb[r] * ib, u, 0, 0, 0);
    float ubar = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) ubar += u[r] * wa[r];
    ubar += other_half(ubar);
    ubar *= ia;
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += (u[r] - ubar) * wa[r] * (xa - cs[r]);
    t += other_half(t);
    da = clamp_passes(ra, maxval) ? coef * t * ia : 0.f;
  }
}

__device__ __forceinline__ void centres_of_half(const Params& P, int h, float (&cs)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) cs[r] = h ? P.c[acc_row(r, 1)] : P.c[acc_row(r, 0)];
}

// ------------------------------------------------------------------------------------------------ global form
__global__ __launch_bounds__(BLK) void mi_hist_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      float* __restrict__ part, int64_t N, int nchunk, Params P) {
  __shared__ float sm[WAVES][PART];
  const int lane = threadIdx.x & 63, h = lane >> 5, bin = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bi = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
  const float* ab = a + (int64_t)bi * N;
  const float* bb = b + (int64_t)bi * N;
  const float cl = centre_of_lane(P, bin);
  f32x16 acc = {0}, none = {0};
  float pa = 0.f, pb = 0.f;
  const int64_t v0 = (int64_t)ch * CHUNK + (int64_t)w * WAVE_VOX;
  const int64_t v1 = v0 + WAVE_VOX < N ? v0 + WAVE_VOX : N;
  for (int64_t base = v0; base < v1; base += 64) {
    const int64_t k = base + lane;
    const float xa = k < v1 ? clampv(ab[k], P.maxval) : 0.f;
    const float xb = k < v1 ? clampv(bb[k], P.maxval) : 0.f;
    const int nvalid = v1 - base < 64 ? (int)(v1 - base) : 64;
    hist_64<false>(xa, xb, nvalid, cl, P.k2, h, acc, none, pa, pb);
  }
  pa += other_half(pa);
  pb += other_half(pb);
#pragma unroll
  for (int r = 0; r < 16; ++r) sm[w][acc_row(r, h) * NB + bin] = acc[r];
  if (h == 0) {
    sm[w][NB * NB + bin] = pa;
    sm[w][NB * NB + NB + bin] = pb;
  }
  __syncthreads();
  float* out = part + (int64_t)blockIdx.x * PART;
  for (int e = threadIdx.x; e < PART; e += BLK) {
    float t = sm[0][e];
#pragma unroll
    for (int q = 1; q < WAVES; ++q) t += sm[q][e];
    out[e] = t;
  }
}

// grid (SLICES, B): slice s of batch element b adds its share of the partials in order
__global__ __launch_bounds__(BLK) void mi_reduce_kernel(const float* __restrict__ part, double* __restrict__ red, int nchunk) {
  const int per = (nchunk + SLICES - 1) / SLICES;
  const int p0 = blockIdx.x * per, p1 = p0 + per < nchunk ? p0 + per : nchunk;
  const float* src = part + (int64_t)blockIdx.y * nchunk * PART;
  double* dst = red + ((int64_t)blockIdx.y * SLICES + blockIdx.x) * PART;
  for (int e = threadIdx.x; e < PART; e += BLK) {
    double t = 0.0;
    for (int p = p0; p < p1; ++p) t += (double)src[(int64_t)p * PART + e];
    dst[e] = t;
  }
}

// one workgroup of 1024 threads, thread t = element (i, j) = (t >> 5, t & 31); the batch elements one after the other
__global__ __launch_bounds__(1024) void mi_final_kernel(const double* __restrict__ red, float* __restrict__ G,
                                                         float* __restrict__ loss, int B, double inv_n) {
  __shared__ double s_dq[NB * NB], s_red[NB * NB], s_pa[NB], s_pb[NB], s_ga[NB], s_gb[NB];
  const int t = threadIdx.x, i = t >> 5, j = t & 31;
  double total = 0.0;
  for (int b = 0; b < B; ++b) {
    const double* src = red + (int64_t)b * SLICES * PART;
    double p = 0.0;
    for (int s = 0; s < SLICES; ++s) p += src[s * PART + t];
    p *= inv_n;
    if (t < 2 * NB) {
      double q = 0.0;
      for (int s = 0; s < SLICES; ++s) q += src[s * PART + NB * NB + t];
      q *= inv_n;
      if (t < NB) s_pa[t] = q; else s_pb[t - NB] = q;
    }
    __syncthreads();
    const double Q = s_pa[i] * s_pb[j] + 1e-6;
    const double R = p / Q + 1e-6;
    const double lg = log(R);
    const double gp = lg + p / (R * Q);          // d mi / d pab_ij
    s_dq[t] = -p * p / (R * Q * Q);              // d mi / d papb_ij
    s_red[t] = p * lg;
    __syncthreads();
    if (t < NB) {
      double g = 0.0;
      for (int q = 0; q < NB; ++q) g += s_dq[t * NB + q] * s_pb[q];
      s_ga[t] = g;
    } else if (t < 2 * NB) {
      double g = 0.0;
      for (int q = 0; q < NB; ++q) g += s_dq[q * NB + (t - NB)] * s_pa[q];
      s_gb[t - NB] = g;
    }
    for (int o = NB * NB / 2; o > 0; o >>= 1) {
      __syncthreads();
      if (t < o) s_red[t] += s_red[t + o];
    }
    __syncthreads();
    float* Gb = G + (int64_t)b * 2 * NB * NB;
    Gb[i * NB + j] = (float)(gp + s_gb[j]);
    Gb[NB * NB + j * NB + i] = (float)(gp + s_ga[i]);
    if (t == 0) total += s_red[0];
    __syncthreads();
  }
  if (t == 0) loss[0] = (float)(-total / (double)B);
}

template <bool DA, bool DB>
__global__ __launch_bounds__(BLK) void mi_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ G, float* __restrict__ d_a,
                                                      float* __restrict__ d_b, int64_t N, int nchunk, float coef, Params P) {
  const int lane = threadIdx.x & 63, h = lane >> 5, v = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bi = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
  const float* ab = a + (int64_t)bi * N;
  const float* bb = b + (int64_t)bi * N;
  const float* Gb = G + (int64_t)bi * 2 * NB * NB;
  float cs[16], gA[16], gB[16];
  centres_of_half(P, h, cs);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = h ? acc_row(r, 1) : acc_row(r, 0);
    gB[r] = DB ? Gb[row * NB + v] : 0.f;
    gA[r] = DA ? Gb[NB * NB + row * NB + v] : 0.f;
  }
  const int64_t v0 = (int64_t)ch * CHUNK + (int64_t)w * WAVE_VOX;
  const int64_t v1 = v0 + WAVE_VOX < N ? v0 + WAVE_VOX : N;
  for (int64_t base = v0; base < v1; base += 32) {
    const int64_t k = base + v;
    const bool valid = k < v1;
    const float ra = valid ? ab[k] : 0.f, rb = valid ? bb[k] : 0.f;
    float da = 0.f, db = 0.f;
    grad_32<DA, DB>(ra, rb, gA, gB, cs, P.k2, P.maxval, coef, da, db);
    if (valid && h == 0) {
      if (DA) d_a[(int64_t)bi * N + k] = da;
      if (DB) d_b[(int64_t)bi * N + k] = db;
    }
  }
}

// ------------------------------------------------------------------------------------------------ local form
struct Patches {
  int D, H, W, p, p3;
  int nz, ny, nx;      // patches per axis
  int oz, oy, ox;      // low-side padding
  int total;           // B nz ny nx
};

// One 32 x 32 tile of a patch's histogram -> its share of mi and the tile of d mi / d pab + the term of the COLUMN's marginal.
// The tile's rows index prow and its columns pcol (both given per lane as element lane & 31, already divided by N):
// (pa, pb) for pab, (pb, pa) for its transpose.
__device__ __forceinline__ void finish_tile(const f32x16& acc, float prow_l, float pcol_l, float inv_n, int h, float (&g)[16],
                                            float& mi_l) {
  float gp[16];
  float gcol = 0.f;
  mi_l = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float pr = __shfl(prow_l, h ? acc_row(r, 1) : acc_row(r, 0), 64);      // every lane takes part: the sources sit in half 0
    const float p = acc[r] * inv_n;
    const float Q = pr * pcol_l + 1e-6f;
    const float R = p / Q + 1e-6f;
    const float lg = logf(R);
    mi_l += p * lg;
    gp[r] = lg + p / (R * Q);
    gcol += -p * p / (R * Q * Q) * pr;
  }
  gcol += other_half(gcol);
#pragma unroll
  for (int r = 0; r < 16; ++r) g[r] = gp[r] + gcol;
}

// voxel t of patch (bi, pz, py, px): its offset in the volume, or -1 for padding and for t >= p^3
__device__ __forceinline__ int64_t patch_voxel(const Patches& q, int bi, int pz, int py, int px, int t) {
  if (t >= q.p3) return -1;
  const int dx = t % q.p, dy = (t / q.p) % q.p, dz = t / (q.p * q.p);
  const int z = pz * q.p + dz - q.oz, y = py * q.p + dy - q.oy, x = px * q.p + dx - q.ox;
  if (z < 0 || z >= q.D || y < 0 || y >= q.H || x < 0 || x >= q.W) return -1;
  return (((int64_t)bi * q.D + z) * q.H + y) * q.W + x;
}

template <bool DA, bool DB>
__global__ __launch_bounds__(BLK) void lmi_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ part, float* __restrict__ d_a, float* __restrict__ d_b,
                                                  Patches q, float coef, Params P) {
  const int lane = threadIdx.x & 63, h = lane >> 5, bin = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int patch = blockIdx.x * WAVES + w;
  if (patch >= q.total) return;                  // whole waves leave; the kernel has no barrier
  int rest = patch;
  const int px = rest % q.nx; rest /= q.nx;
  const int py = rest % q.ny; rest /= q.ny;
  const int pz = rest % q.nz;
  const int bi = rest / q.nz;

  const float cl = centre_of_lane(P, bin);
  f32x16 acc = {0}, accT = {0};
  float pa = 0.f, pb = 0.f;
  for (int base = 0; base < q.p3; base += 64) {
    const int64_t off = patch_voxel(q, bi, pz, py, px, base + lane);
    const float xa = off >= 0 ? clampv(a[off], P.maxval) : 0.f;      // padding follows the clamp: value 0
    const float xb = off >= 0 ? clampv(b[off], P.maxval) : 0.f;
    const int nvalid = q.p3 - base < 64 ? q.p3 - base : 64;
    hist_64<DA>(xa, xb, nvalid, cl, P.k2, h, acc, accT, pa, pb);
  }
  const float inv_n = 1.f / (float)q.p3;
  pa = (pa + other_half(pa)) * inv_n;
  pb = (pb + other_half(pb)) * inv_n;
  float gA[16] = {}, gB[16], mi_l, unused;
  finish_tile(acc, pa, pb, inv_n, h, gB, mi_l);
  const float mi = wave_sum(mi_l);
  if (lane == 0) part[patch] = mi;
  if (!DA && !DB) return;
  if (DA) finish_tile(accT, pb, pa, inv_n, h, gA, unused);

  float cs[16];
  centres_of_half(P, h, cs);
  for (int base = 0; base < q.p3; base += 32) {
    const int64_t off = patch_voxel(q, bi, pz, py, px, base + bin);
    const float ra = off >= 0 ? a[off] : 0.f, rb = off >= 0 ? b[off] : 0.f;
    float da = 0.f, db = 0.f;
    grad_32<DA, DB>(ra, rb, gA, gB, cs, P.k2, P.maxval, coef, da, db);
    if (off >= 0 && h == 0) {
      if (DA) d_a[off] = da;
      if (DB) d_b[off] = db;
    }
  }
}

__global__ __launch_bounds__(1024) void lmi_loss_kernel(const float* __restrict__ part, int n, float* __restrict__ loss) {
  __shared__ double s[1024];
  double t = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) t += (double)part[i];
  s[threadIdx.x] = t;
  for (int o = 512; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
  }
  if (threadIdx.x == 0) loss[0] = (float)(-s[0] / (double)n);
}

// ------------------------------------------------------------------------------------------------ host side
inline bool dims_ok(int B, int D, int H, int W) {
  return B > 0 && D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < (1ll << 31) && (int64_t)B * D * H * W < (1ll << 40);
}
inline int chunks_of(int D, int H, int W) { return (int)cdiv64((int64_t)D * H * W, CHUNK); }
inline bool grid_ok(int B, int D, int H, int W) { return (int64_t)B * chunks_of(D, H, W) < (1ll << 30); }

inline bool make_patches(int B, int D, int H, int W, int p, Patches& q) {
  if (p < 1 || p > MAX_PATCH) return false;
  const int rz = (p - D % p) % p, ry = (p - H % p) % p, rx = (p - W % p) % p;
  q.D = D; q.H = H; q.W = W; q.p = p; q.p3 = p * p * p;
  q.nz = (D + rz) / p; q.ny = (H + ry) / p; q.nx = (W + rx) / p;
  q.oz = rz / 2; q.oy = ry / 2; q.ox = rx / 2;
  const int64_t total = (int64_t)B * q.nz * q.ny * q.nx;
  if (total >= (1ll << 30)) return false;
  q.total = (int)total;
  return true;
}

inline bool params_ok(int num_bins, float minval, float maxval, float sigma_ratio) {
  return num_bins == NB && maxval > 0.f && maxval > minval && sigma_ratio > 0.f;      // (a NaN fails every comparison)
}

// The centres as torch.linspace(minval, maxval, 32) has them in fp32: the step in fp32, the lower half counted up from the
// start and the upper half down from the end, each with one rounding.
inline Params make_params(float minval, float maxval, float sigma_ratio) {
  Params P;
  const float step = (maxval - minval) / (float)(NB - 1);
  for (int i = 0; i < NB; ++i) P.c[i] = i < NB / 2 ? fmaf(step, (float)i, minval) : fmaf(-step, (float)(NB - 1 - i), maxval);
  const double sigma = ((double)maxval - (double)minval) / (double)(NB - 1) * (double)sigma_ratio;
  P.k2 = (float)(-1.0 / (2.0 * sigma * sigma) * 1.4426950408889634);
  P.maxval = maxval;
  return P;
}
inline double preterm_of(float minval, float maxval, float sigma_ratio) {
  const double sigma = ((double)maxval - (double)minval) / (double)(NB - 1) * (double)sigma_ratio;
  return 1.0 / (2.0 * sigma * sigma);
}

// workspace of the global form: [ red: B SLICES PART doubles | part: B nchunk PART floats | G: B 2 32 32 floats ]
inline size_t global_ws(int B, int nchunk) {
  return (size_t)B * SLICES * PART * sizeof(double) + ((size_t)B * nchunk * PART + (size_t)B * 2 * NB * NB) * sizeof(float);
}

}  // namespace

extern "C" {

size_t modet_mi_ws_bytes(int B, int D, int H, int W, int patch_size) {
  if (!dims_ok(B, D, H, W)) return 0;
  if (patch_size == 0) return grid_ok(B, D, H, W) ? global_ws(B, chunks_of(D, H, W)) : 0;
  Patches q;
  if (!make_patches(B, D, H, W, patch_size, q)) return 0;
  return (size_t)q.total * sizeof(float);
}

int modet_mi_fwd_bwd(const float* a, const float* b, float* loss, float* d_a, float* d_b, void* ws, size_t ws_bytes, int B,
                     int D, int H, int W, int num_bins, float minval, float maxval, float sigma_ratio, float grad_scale,
                     modet_stream_t stream) {
  MODET_CHECK_PTR(a); MODET_CHECK_PTR(b); MODET_CHECK_PTR(loss); MODET_CHECK_PTR(ws);
  MODET_CHECK_DIM(dims_ok(B, D, H, W) && grid_ok(B, D, H, W));
  if (!params_ok(num_bins, minval, maxval, sigma_ratio)) return MODET_ERR_UNSUPPORTED;
  if (ws_bytes < modet_mi_ws_bytes(B, D, H, W, 0) || ((uintptr_t)ws & 7) != 0) return MODET_ERR_WORKSPACE;   // (it begins with doubles)
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = (int64_t)D * H * W;
  const int nchunk = chunks_of(D, H, W);
  const Params P = make_params(minval, maxval, sigma_ratio);
  double* red = (double*)ws;
  float* part = (float*)(red + (size_t)B * SLICES * PART);
  float* G = part + (size_t)B * nchunk * PART;
  hipLaunchKernelGGL(mi_hist_kernel, dim3(B * nchunk), dim3(BLK), 0, s, a, b, part, N, nchunk, P);
  hipLaunchKernelGGL(mi_reduce_kernel, dim3(SLICES, B), dim3(BLK), 0, s, (const float*)part, red, nchunk);
  hipLaunchKernelGGL(mi_final_kernel, dim3(1), dim3(1024), 0, s, (const double*)red, G, loss, B, 1.0 / (double)N);
  // loss = -mean_b mi;  d mi / d x = (1 / N) (-2 preterm) sum_j (U_j - Ubar) (x - c_j) w_j / s
  const float coef = (float)((double)grad_scale * 2.0 * preterm_of(minval, maxval, sigma_ratio) / ((double)B * (double)N));
  if (d_a && d_b)
    hipLaunchKernelGGL((mi_grad_kernel<true, true>), dim3(B * nchunk), dim3(BLK), 0, s, a, b, (const float*)G, d_a, d_b, N, nchunk, coef, P);
  else if (d_b)
    hipLaunchKernelGGL((mi_grad_kernel<false, true>), dim3(B * nchunk), dim3(BLK), 0, s, a, b, (const float*)G, d_a, d_b, N, nchunk, coef, P);
  else if (d_a)
    hipLaunchKernelGGL((mi_grad_kernel<true, false>), dim3(B * nchunk), dim3(BLK), 0, s, a, b, (const float*)G, d_a, d_b, N, nchunk, coef, P);
  return modet_launch_status();
}

int modet_lmi_fwd_bwd(const float* a, const float* b, float* loss, float* d_a, float* d_b, void* ws, size_t ws_bytes, int B,
                      int D, int H, int W, int num_bins, float minval, float maxval, float sigma_ratio, int patch_size,
                      float grad_scale, modet_stream_t stream) {
  MODET_CHECK_PTR(a); MODET_CHECK_PTR(b); MODET_CHECK_PTR(loss); MODET_CHECK_PTR(ws);
  MODET_CHECK_DIM(dims_ok(B, D, H, W));
  if (!params_ok(num_bins, minval, maxval, sigma_ratio) || patch_size < 1 || patch_size > MAX_PATCH) return MODET_ERR_UNSUPPORTED;
  Patches q;
  MODET_CHECK_DIM(make_patches(B, D, H, W, patch_size, q));
  if (ws_bytes < modet_mi_ws_bytes(B, D, H, W, patch_size) || ((uintptr_t)ws & 3) != 0) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Params P = make_params(minval, maxval, sigma_ratio);
  float* part = (float*)ws;
  const float coef = (float)((double)grad_scale * 2.0 * preterm_of(minval, maxval, sigma_ratio) / ((double)q.total * (double)q.p3));
  const dim3 grid(cdiv(q.total, WAVES));
  if (d_a && d_b)
    hipLaunchKernelGGL((lmi_kernel<true, true>), grid, dim3(BLK), 0, s, a, b, part, d_a, d_b, q, coef, P);
  else if (d_b)
    hipLaunchKernelGGL((lmi_kernel<false, true>), grid, dim3(BLK), 0, s, a, b, part, d_a, d_b, q, coef, P);
  else if (d_a)
    hipLaunchKernelGGL((lmi_kernel<true, false>), grid, dim3(BLK), 0, s, a, b, part, d_a, d_b, q, coef, P);
  else
    hipLaunchKernelGGL((lmi_kernel<false, false>), grid, dim3(BLK), 0, s, a, b, part, d_a, d_b, q, coef, P);
  hipLaunchKernelGGL(lmi_loss_kernel, dim3(1), dim3(1024), 0, s, (const float*)part, q.total, loss);
  return modet_launch_status();
}

}  // extern "C"
