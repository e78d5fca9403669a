/* libmodet_hip.so -- the positional-encoding projection of the Im2Grid baseline (the reference's PositionalEncodingLayer,
 * "Baseline methods/Im2Grid/models.py":238-274: Linear(Cin -> 6) plus alpha times a sinusoidal embedding of the voxel's position),
 * next to the core ABI of modet_hip.h and the families of modet_hip_losses.h, modet_hip_mi.h, modet_hip_ssim.h, modet_hip_reg.h,
 * modet_hip_vecint.h and modet_hip_surface.h (all seven stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no memset node, no float atomics -- a call can be captured into a hipGraph and two runs
 * on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_POSENC_H
#define MODET_HIP_POSENC_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_POSENC_DIM = 6, MODET_POSENC_MAX_TABLE = 1536 };

/* THE LAYER.  x is (B,D,H,W,Cin) fp32, channels-last; y is (B,D,H,W,6):
 *     y[b,d,h,w,j] = sum_c Wt[j,c] * x[b,d,h,w,c] + bias[j] + alpha * emb_j(d,h,w)
 *     emb = [cos t_d, sin t_d, cos t_h, sin t_h, cos t_w, sin t_w],   t_p = p * pi / (n - 1) along the axis of length n
 * (the reference's first / second / third spatial axis).  Wt is (6, Cin) row-major (nn.Linear's weight), bias (6), alpha ONE float
 * in device memory (a parameter: a captured call reads its value at replay time).
 *
 * THE TABLE.  The kernels evaluate no trigonometric function.  tab holds (D + H + W) pairs of fp32, (cos, sin) interleaved:
 *     tab[2 * p]             , tab[2 * p + 1]              = cos, sin of p * pi / (D - 1)     p = 0 .. D-1
 *     tab[2 * (D + p)]       , tab[2 * (D + p) + 1]        = cos, sin of p * pi / (H - 1)     p = 0 .. H-1
 *     tab[2 * (D + H + p)]   , tab[2 * (D + H + p) + 1]    = cos, sin of p * pi / (W - 1)     p = 0 .. W-1
 * The package fills it once per shape in fp64 and rounds to fp32.  The term is fl(fma(alpha, tab, z)) with z the fp32 linear part:
 * with Wt = 0 and bias = 0 the output is fl(alpha * tab) bit for bit.
 *
 * PAIRS.  A level applies the layer to its fixed and to its warped moving features with the same parameters; every entry point
 * takes both uses.  The second use is absent when its pointers are NULL.
 *
 * modet_posenc_fwd_pair: y1 = layer(x1), y2 = layer(x2).  x2 and y2 are NULL together for a single use.
 *
 * modet_posenc_bwd_data_pair: d_x1[n,c] = sum_j d_y1[n,j] * Wt[j,c], the same for use 2.  d_x1 or d_x2 may be NULL (that use is
 *   skipped and its d_y is not read), not both.
 *
 * modet_posenc_bwd_params_pair: d_Wt (6,Cin) = sum over voxels and uses of d_y^T x, d_bias (6) = sum d_y, d_alpha (1) = sum
 *   d_y * emb.  Two stages: per-workgroup fp32 partial rows [d_Wt | d_bias | d_alpha] in ws, then one fixed-order fp64 column sum
 *   over the rows of BOTH uses (the way modet_proj_ln_bwd_pair sums its parameter gradients).  x2 and d_y2 are NULL together
 *   for a single use.  ws: modet_posenc_ws_bytes bytes, 16-byte aligned.
 *
 * LIMITS.  dim == 6 and Cin a multiple of 4 up to 128, else MODET_ERR_UNSUPPORTED; D + H + W <= MODET_POSENC_MAX_TABLE (the table
 * is staged in LDS), else MODET_ERR_UNSUPPORTED.  B < 1, D, H or W < 2 (the reference divides by n - 1 = 0 there and returns
 * NaN), B * D * H * W >= 2^31: MODET_ERR_DIM.  A required pointer that is NULL, or one pointer of a NULL-together pair without
 * the other: MODET_ERR_NULL.  A short or misaligned workspace: MODET_ERR_WORKSPACE.  All are answered before the first launch.
 * modet_posenc_ws_bytes is 0 for every shape an entry point refuses.
 *
 * x, Wt and the d_x outputs are read / written as 16-byte vectors: x, d_x must be 16-byte aligned (Cin % 4 == 0 keeps rows so);
 * Wt, bias, alpha, tab and the d_* parameter outputs need 4-byte alignment only; y and d_y 8-byte alignment. */
size_t modet_posenc_ws_bytes(int B, int D, int H, int W, int Cin, int dim);
int modet_posenc_fwd_pair(const float* x1, const float* x2, const float* Wt, const float* bias, const float* alpha,
                          const float* tab, float* y1, float* y2, int B, int D, int H, int W, int Cin, int dim,
                          modet_stream_t stream);
int modet_posenc_bwd_data_pair(const float* d_y1, const float* d_y2, const float* Wt, float* d_x1, float* d_x2, int B, int D,
                               int H, int W, int Cin, int dim, modet_stream_t stream);
int modet_posenc_bwd_params_pair(const float* x1, const float* d_y1, const float* x2, const float* d_y2, const float* tab,
                                 float* d_Wt, float* d_bias, float* d_alpha, void* ws, size_t ws_bytes, int B, int D, int H,
                                 int W, int Cin, int dim, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
