// 27-displacement local correlation of the PR++ baseline ("Baseline methods/PR++/models.py":205-232, Correlation3D with
// kernel_size 3, d = 3, sw = 1, sf = 2) -- SURVEY.md 8(f) rank 4, a sibling of the neighbourhood attention:
//   pm = box3(mov), pf = box3(fix)  (3x3x3 all-ones grouped conv, zero padded; pf also on a 1-voxel ring outside the
//   volume, where the box still overlaps it -- the reference pads fix by sf+1 = 3),
//   corr[b][t][p] = (1/27) sum_c pm[b,p,c] * pf[b, p + 2*off(t), c],   t = 9i+3j+k, off = (i-1, j-1, k-1).
// Channels-last features (B,D,H,W,C), C % 4 == 0; corr is written as (B,27,D,H,W) like the reference.
// Backward: d_pm and d_pf by the transposed gathers, then the box sum (self-adjoint under zero padding) once more.
// No atomics; HBM/L2-bound gathers.  The box sums, the dot products and the gathers are in corr3d_internal.h, which prpp.hip
// shares (the same correlation as a slice of a channels-last row).
#include "corr3d_internal.h"

namespace {

// One workgroup per strip of 32 consecutive voxels (corr_strip); the 27 x 32 results go through LDS so that every correlation
// plane receives one contiguous 128 B row.
__global__ __launch_bounds__(BLK) void corr_fwd_kernel(const float* __restrict__ pm, const float* __restrict__ pfx,
                                                       float* __restrict__ corr, int D, int H, int W, int C, int64_t N) {
  __shared__ float res[27 * CS_V];
  const int64_t V = (int64_t)D * H * W;
  const int64_t n0 = (int64_t)blockIdx.x * CS_V;
  corr_strip(pm, pfx, res, D, H, W, C, N, n0);
  __syncthreads();
  for (int i = threadIdx.x; i < 27 * CS_V; i += BLK) {
    const int t = i / CS_V, v = i - t * CS_V;
    const int64_t n = n0 + v;
    if (n < N) {
      const int64_t b = n / V, p = n - b * V;
      corr[(b * 27 + t) * V + p] = res[i] * (1.f / 27.f);
    }
  }
}

}  // namespace

extern "C" {

size_t modet_corr3d_ws_bytes(int B, int D, int H, int W, int C) { return corr_ws_bytes(B, D, H, W, C); }

int modet_corr3d_fwd(const float* mov, const float* fix, float* corr, void* ws, size_t ws_bytes, int B, int D, int H,
                     int W, int C, modet_stream_t stream) {
  MODET_CHECK_PTR(mov); MODET_CHECK_PTR(fix); MODET_CHECK_PTR(corr); MODET_CHECK_PTR(ws);
  if (const int e = corr_check(B, D, H, W, C)) return e;
  if (ws_bytes < modet_corr3d_ws_bytes(B, D, H, W, C)) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * D * H * W;
  float* pm = (float*)ws;
  float* pfx = pm + n * C;
  launch_box_pair(mov, fix, pm, pfx, B, D, H, W, C, s);
  hipLaunchKernelGGL(corr_fwd_kernel, dim3((unsigned)cdiv64(n, CS_V)), dim3(BLK), 0, s, (const float*)pm, (const float*)pfx, corr, D, H,
                     W, C, n);
  return modet_launch_status();
}

int modet_corr3d_bwd(const float* mov, const float* fix, const float* d_corr, float* d_mov, float* d_fix, void* ws,
                     size_t ws_bytes, int B, int D, int H, int W, int C, modet_stream_t stream) {
  MODET_CHECK_PTR(mov); MODET_CHECK_PTR(fix); MODET_CHECK_PTR(d_corr); MODET_CHECK_PTR(d_mov); MODET_CHECK_PTR(d_fix);
  MODET_CHECK_PTR(ws);
  if (const int e = corr_check(B, D, H, W, C)) return e;
  if (ws_bytes < modet_corr3d_ws_bytes(B, D, H, W, C)) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * D * H * W, ne = ext_elems(B, D, H, W, C) / C;
  const unsigned G = C / 4;
  float* pm = (float*)ws;
  float* pfx = pm + n * C;
  float* dpm = pfx + ne * C;
  float* dpfx = dpm + n * C;
  launch_box_pair(mov, fix, pm, pfx, B, D, H, W, C, s);
  hipLaunchKernelGGL(corr_bwd_pm_kernel, dim3(flat_grid(n * G, BLK)), dim3(BLK), 0, s, d_corr, (const float*)pfx, dpm, D, H, W, C,
                     (unsigned)(n * G), 0, 0);
  hipLaunchKernelGGL(corr_bwd_pf_kernel, dim3(flat_grid(ne * G, BLK)), dim3(BLK), 0, s, d_corr, (const float*)pm, dpfx, D, H, W, C,
                     (unsigned)(ne * G), 0, 0);
  // the box sum is self-adjoint: d_mov = box3(d_pm); d_fix = box3 of d_pfx (extended grid) evaluated inside the volume
  hipLaunchKernelGGL(box3_kernel<false>, dim3(flat_grid(n * G, BLK)), dim3(BLK), 0, s, (const float*)dpm, d_mov, D, H, W, C, 0, 0, (unsigned)(n * G),
                     (const float*)nullptr, 0, 0);
  hipLaunchKernelGGL(box3_kernel<false>, dim3(flat_grid(n * G, BLK)), dim3(BLK), 0, s, (const float*)dpfx, d_fix, D, H, W, C, 1, 0, (unsigned)(n * G),
                     (const float*)nullptr, 0, 0);
  return modet_launch_status();
}

}  // extern "C"
