// The flow regularisers of the reference's Baseline methods/RCN/losses.py beside Grad3d: Grad3DiTV (:203-221, kind 0) and
// DisplacementRegularizer (:223-268) 'gradient-l2' (1), 'gradient-l1' (2) and 'bending' (3); include/modet_hip_reg.h has the formulae.
//
// One forward + backward launch per call (reg_kernel) and a fixed-order fp64 sum of the workgroups' loss partials
// (scalar_finalize_kernel, common.h).  Every kind is a streaming stencil in grad3d_kernel's scheme: a flat index over the ELEMENTS of the flow
// in either layout (planar: CS = 1 over B C volumes; channels-last: CS = 3, a voxel's neighbours are CS elements apart), each thread
// GATHERS the adjoint of the stencils that touch its element, so nothing is scattered, nothing is atomic and no intermediate volume
// exists: the flow is read (neighbours through the caches) and the gradient written once, 8 B per element.  A neighbour outside the
// volume re-reads the element itself; where the term it would enter is not simply an exact 0 a mask drops it.
//
// Loss terms are handed to exactly one element each: the element itself (iTV norm, s_aa), the element one central difference up
// the axis (gradient kinds: the difference centred at q - e_a belongs to q) or the upper corner q = p + e_a + e_b of a mixed
// derivative s_ab(p) -- always inside the volume, and made of loads the gradient needs anyway.
//
// bending: the gradient at q collects s_aa at q and q +- 2 e_a and s_ab at the four q +- e_a +- e_b, 25 distinct loads at the offsets
// 0, +- 2 e_a, +- 4 e_a, +- 2 e_a +- 2 e_b.  Elements at least 4 voxels from every face (all but a shell) run the stencil with every
// term present: no masks, no clamped addresses.  The shell runs the SAME arithmetic with a mask per term, so the two paths differ
// in instructions, not in rounding, and an element's result depends on its position alone, not on the layout or the grid.
#include "common.h"

#include "../../include/modet_hip_reg.h"

namespace {

constexpr int BLK = 256;
constexpr int MAX_PARTS = 2048;

struct Geo {
  int n[3];          // D, H, W
  int64_t s[3];      // element strides of z, y, x
};

struct Term { float loss, grad; };

// ------------------------------------------------------------------------------------------------ iTV
// (d_H^2 + d_D^2) + d_W^2 + 1e-6, the reference's order of the sum under the root
__host__ __device__ __forceinline__ float itv_norm(float dD, float dH, float dW) { return sqrtf(dH * dH + dD * dD + dW * dW + 1e-6f); }

__host__ __device__ __forceinline__ Term itv_element(const float* __restrict__ f, int64_t i, const int (&c)[3], const Geo& g) {
  const float v = f[i];
  const bool lo[3] = {c[0] >= 1, c[1] >= 1, c[2] >= 1};
  float dm[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) dm[a] = v - f[lo[a] ? i - g.s[a] : i];
  const bool own = lo[0] && lo[1] && lo[2];
  const float nq = itv_norm(dm[0], dm[1], dm[2]);
  Term t;
  t.loss = own ? nq : 0.f;
  t.grad = own ? (dm[0] + dm[1] + dm[2]) / nq : 0.f;
  // the three grid points one step up an axis hold a difference against this element: their norms are recomputed from loads
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, e = (a + 2) % 3;
    const bool m = c[a] + 1 < g.n[a] && lo[b] && lo[e];
    const int64_t j = m ? i + g.s[a] : i;
    const float w = f[j];
    float d[3];
    d[a] = w - v;
    d[b] = w - f[m ? j - g.s[b] : j];
    d[e] = w - f[m ? j - g.s[e] : j];
    const float q = d[a] / itv_norm(d[0], d[1], d[2]);
    t.grad -= m ? q : 0.f;
  }
  return t;
}

// ------------------------------------------------------------------------------------------------ gradient-l2 / gradient-l1
// the central difference at p = q - e_a is (f[q] - f[q - 2 e_a]) / 2 and the one at q + e_a is (f[q + 2 e_a] - f[q]) / 2; p has to
// be an interior point.  A dropped term reads f[q] twice: its difference, its penalty and its derivative are exact zeros.
template <bool L1>
__host__ __device__ __forceinline__ Term gradient_element(const float* __restrict__ f, int64_t i, const int (&c)[3], const Geo& g) {
  auto pen = [](float t) { return L1 ? fabsf(t) : t * t; };
  auto dpen = [](float t) { return L1 ? (t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f)) : t; };
  const float v = f[i];
  bool in[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) in[a] = c[a] >= 1 && c[a] <= g.n[a] - 2;
  Term t{0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const bool other = in[(a + 1) % 3] && in[(a + 2) % 3];
    const bool vm = other && c[a] >= 2, vp = other && c[a] <= g.n[a] - 3;
    const float tm = (v - f[vm ? i - 2 * g.s[a] : i]) * 0.5f;
    const float tp = (f[vp ? i + 2 * g.s[a] : i] - v) * 0.5f;
    t.loss += pen(tm);
    t.grad += dpen(tm) - dpen(tp);
  }
  return t;
}

// ------------------------------------------------------------------------------------------------ bending
// r_aa(p) = f[p + 2 e_a] - 2 f[p] + f[p - 2 e_a] = 4 s_aa(p),  r_ab(p) = (f[p+e_a+e_b] - f[p-e_a+e_b]) - (f[p+e_a-e_b] - f[p-e_a-e_b])
// = 4 s_ab(p).  With L = sum r_aa^2 + 2 sum r_ab^2 the loss is L / (16 M) and
//   d loss / d f[q] = G / (8 M),  G = sum_a (r_aa(q - 2 e_a) - 2 r_aa(q) + r_aa(q + 2 e_a)) + 2 sum_{a<b} sum_{s,t = +-1} s t r_ab(q + s e_a + t e_b)
// over the stencil points p that lie at least 2 voxels from every face.
template <bool INTERIOR>
__host__ __device__ __forceinline__ Term bending_element(const float* __restrict__ f, int64_t i, const int (&c)[3], const Geo& g) {
  const float v = f[i];
  bool ok[3], r2m[3], r2p[3], r4m[3], r4p[3];      // c[a] is a stencil point's coordinate; q -+ 2 e_a, q -+ 4 e_a are inside the volume
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r2m[a] = INTERIOR || c[a] >= 2; r2p[a] = INTERIOR || c[a] <= g.n[a] - 3;
    r4m[a] = INTERIOR || c[a] >= 4; r4p[a] = INTERIOR || c[a] <= g.n[a] - 5;
    ok[a] = r2m[a] && r2p[a];
  }
  auto sel = [](bool m, float x) { return (INTERIOR || m) ? x : 0.f; };
  float L = 0.f, G = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const bool other = ok[(a + 1) % 3] && ok[(a + 2) % 3];
    const int64_t s2 = 2 * g.s[a];
    const float um1 = f[r2m[a] ? i - s2 : i], up1 = f[r2p[a] ? i + s2 : i];
    const float um2 = f[r4m[a] ? i - 2 * s2 : i], up2 = f[r4p[a] ? i + 2 * s2 : i];
    // q - 2 e_a is a stencil point when its coordinate is >= 2 (it is <= n - 3 then: q <= n - 1), q + 2 e_a likewise
    const float r0 = sel(other && ok[a], um1 - 2.f * v + up1);
    const float rm = sel(other && r4m[a], um2 - 2.f * um1 + v);
    const float rp = sel(other && r4p[a], v - 2.f * up1 + up2);
    L += r0 * r0;
    G += rm - 2.f * r0 + rp;
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = a + 1; b < 3; ++b) {
      const int e = 3 - a - b;
      // w[j][k] = f[q + 2 (j - 1) e_a + 2 (k - 1) e_b]; outside the volume: f[q] (every term it enters is masked)
      const bool ra[3] = {r2m[a], true, r2p[a]}, rb[3] = {r2m[b], true, r2p[b]};
      float w[3][3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
          w[j][k] = (j == 1 && k == 1) ? v : f[(ra[j] && rb[k]) ? i + 2 * (j - 1) * g.s[a] + 2 * (k - 1) * g.s[b] : i];
      // p = q + s e_a + t e_b is a stencil point when both coordinates are: c + 1 in [2, n - 3] or c - 1 in [2, n - 3]
      const bool pa[2] = {INTERIOR || (c[a] >= 3 && c[a] <= g.n[a] - 2), INTERIOR || (c[a] >= 1 && c[a] <= g.n[a] - 4)};
      const bool pb[2] = {INTERIOR || (c[b] >= 3 && c[b] <= g.n[b] - 2), INTERIOR || (c[b] >= 1 && c[b] <= g.n[b] - 4)};
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          // corners of p: indices j, j + 1 along a and k, k + 1 along b
          const float r = sel(ok[e] && pa[j] && pb[k], (w[j + 1][k + 1] - w[j][k + 1]) - (w[j + 1][k] - w[j][k]));
          acc += (j == k) ? r : -r;                            // s t = +1 for (-,-) and (+,+)
          if (j == 0 && k == 0) L += 2.f * (r * r);            // the loss term of p = q - e_a - e_b
        }
      G += 2.f * acc;
    }
  }
  return Term{L, G};
}

// KIND as in modet_hip_reg.h.  d = {volumes (B C planar, B channels-last), D, H, W}; N elements in all, < 2^31.
// part[blockIdx.x] = this workgroup's sum of loss terms (fp64); df = gcoef * (the element's gathered gradient).
template <int KIND, int CS>
__global__ __launch_bounds__(BLK) void reg_kernel(const float* __restrict__ f, float* __restrict__ df, double* __restrict__ part,
                                                  int D, int H, int W, int64_t N, float gcoef) {
  __shared__ double red[BLK / 64];
  Geo g;
  g.n[0] = D; g.n[1] = H; g.n[2] = W;
  g.s[0] = (int64_t)H * W * CS; g.s[1] = (int64_t)W * CS; g.s[2] = CS;
  double lsum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < N; i += (int64_t)gridDim.x * BLK) {
    // 32-bit divisions (N < 2^31): a 64-bit one by a run-time value is a ~100-instruction routine
    const unsigned vox = (unsigned)i / (unsigned)CS;
    const unsigned t1 = vox / (unsigned)W, t2 = t1 / (unsigned)H;
    const int c[3] = {(int)(t2 % (unsigned)D), (int)(t1 - t2 * (unsigned)H), (int)(vox - t1 * (unsigned)W)};
    Term t;
    if constexpr (KIND == MODET_REG_ITV) t = itv_element(f, i, c, g);
    else if constexpr (KIND == MODET_REG_GRADIENT_L2) t = gradient_element<false>(f, i, c, g);
    else if constexpr (KIND == MODET_REG_GRADIENT_L1) t = gradient_element<true>(f, i, c, g);
    else {
      const bool interior = c[0] >= 4 && c[0] <= D - 5 && c[1] >= 4 && c[1] <= H - 5 && c[2] >= 4 && c[2] <= W - 5;
      t = interior ? bending_element<true>(f, i, c, g) : bending_element<false>(f, i, c, g);
    }
    lsum += (double)t.loss;
    if (df) df[i] = t.grad * gcoef;
  }
  const double r = block_sum_d<BLK>(lsum, red);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

struct Plan { int64_t N; double M; int grid; };
// a function of the kind and the shape alone; false for what the entry point refuses
inline bool make_plan(int kind, int B, int C, int D, int H, int W, int channels_last, Plan& p) {
  if (kind < MODET_REG_ITV || kind > MODET_REG_BENDING) return false;
  const int lo = kind == MODET_REG_ITV ? 2 : (kind == MODET_REG_BENDING ? 5 : 3);       // shortest axis with a stencil point
  const int cut = kind == MODET_REG_ITV ? 1 : (kind == MODET_REG_BENDING ? 4 : 2);      // axis length - points along it
  if (B < 1 || C < 1 || D < lo || H < lo || W < lo) return false;
  if (C != 3 && (kind != MODET_REG_ITV || channels_last)) return false;
  const double n = (double)B * C * D * H * W;
  if (n >= 2147483648.0) return false;
  p.N = (int64_t)n;
  p.M = (double)B * C * (D - cut) * (H - cut) * (W - cut);
  const int g = flat_grid(p.N, BLK);
  p.grid = g > MAX_PARTS ? MAX_PARTS : g;
  return true;
}

}  // namespace

extern "C" {

size_t modet_reg_ws_bytes(int kind, int B, int C, int D, int H, int W) {
  Plan p;
  if (!make_plan(kind, B, C, D, H, W, 0, p)) return 0;
  return (((size_t)p.grid * sizeof(double)) + 15) & ~(size_t)15;
}

int modet_reg_fwd_bwd(const float* f, float* loss, float* d_f, void* ws, size_t ws_bytes, int kind, int B, int C, int D, int H,
                      int W, int channels_last, float grad_scale, modet_stream_t stream) {
  MODET_CHECK_PTR(f); MODET_CHECK_PTR(loss); MODET_CHECK_PTR(ws);
  if (kind < MODET_REG_ITV || kind > MODET_REG_BENDING) return MODET_ERR_UNSUPPORTED;
  Plan p;
  MODET_CHECK_DIM(make_plan(kind, B, C, D, H, W, channels_last, p));
  if (ws_bytes < modet_reg_ws_bytes(kind, B, C, D, H, W) || ((uintptr_t)ws & 7) != 0) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  // the loss over its sum of terms, and the gradient's factor over the gathered sum (header: the derivative of each penalty)
  double lscale, gscale;
  switch (kind) {
    case MODET_REG_ITV: lscale = 1.0 / (3.0 * p.M); gscale = 1.0 / (3.0 * p.M); break;
    case MODET_REG_GRADIENT_L2: lscale = 1.0 / (3.0 * p.M); gscale = 1.0 / (3.0 * p.M); break;     // d (t^2) = 2 t dt, dt = +- 1/2
    case MODET_REG_GRADIENT_L1: lscale = 1.0 / (3.0 * p.M); gscale = 1.0 / (6.0 * p.M); break;     // d |t| = sign(t) dt
    default: lscale = 1.0 / (16.0 * p.M); gscale = 1.0 / (8.0 * p.M); break;
  }
  // one rounding of the product of the two scales: with grad_scale = 1 the factor is the plain derivative's
  const float gcoef = (float)(gscale * (double)grad_scale);
#define REG_GO(KIND_, CS_)                                                                                                  \
  hipLaunchKernelGGL((reg_kernel<KIND_, CS_>), dim3(p.grid), dim3(BLK), 0, s, f, d_f, part, D, H, W, p.N, gcoef)
#define REG_KIND(KIND_) do { if (channels_last) REG_GO(KIND_, 3); else REG_GO(KIND_, 1); } while (0)
  switch (kind) {
    case MODET_REG_ITV: REG_KIND(MODET_REG_ITV); break;
    case MODET_REG_GRADIENT_L2: REG_KIND(MODET_REG_GRADIENT_L2); break;
    case MODET_REG_GRADIENT_L1: REG_KIND(MODET_REG_GRADIENT_L1); break;
    default: REG_KIND(MODET_REG_BENDING); break;
  }
#undef REG_KIND
#undef REG_GO
  hipLaunchKernelGGL(scalar_finalize_kernel<double>, dim3(1), dim3(BLK), 0, s, (const double*)part, p.grid, lscale, loss);
  return modet_launch_status();
}

}  // extern "C"
