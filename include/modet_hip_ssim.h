/* libmodet_hip.so -- the SSIM3D similarity loss beside the core ABI of modet_hip.h and the loss families of
 * modet_hip_losses.h and modet_hip_mi.h (all three stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no memset node, no float atomics -- a call can be captured into a hipGraph and two runs
 * on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_SSIM_H
#define MODET_HIP_SSIM_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 - mean structural similarity of two volumes (reference Baseline methods/RCN/losses.py:9-27, 53-74, 103-148, SSIM3D and
 * ssim3D).  a = img1 and b = img2 are (B,1,D,H,W) = (B,D,H,W) fp32 planar, any D, H, W >= 1 (axes shorter than the window
 * included), w = window, p = w / 2.
 *
 *   t_i      = exp(-(i - p)^2 / (2 1.5^2)), i = 0 .. w-1, rounded to fp32 and divided by their sum rounded to fp32 (computed
 *              on the host)
 *   G v      = the zero-padded (p voxels on every side of every axis) filter of v with the window t (x) t (x) t, applied as
 *              three 1-D filters; nothing of the w^3 window is ever formed
 *   m1 = G a,  m2 = G b,  s11 = G a^2,  s22 = G b^2,  s12 = G ab,   C1 = 0.01^2,  C2 = 0.03^2
 *   ssim     = (2 m1 m2 + C1) (2 (s12 - m1 m2) + C2) / ((m1^2 + m2^2 + C1) ((s11 - m1^2) + (s22 - m2^2) + C2))
 *   loss     = 1 - mean of ssim over all voxels of all batch elements      (no clamp, no epsilon beyond C1 and C2)
 *
 * The filter is its own adjoint, so with c_f = d loss / d f per voxel for the five fields f
 *   d loss / d b = G c_m2 + 2 b G c_s22 + a G c_s12      and      d loss / d a = G c_m1 + 2 a G c_s11 + b G c_s12.
 * d_a and d_b (same shape as a and b) may each be NULL; they receive grad_scale * d loss / d a and grad_scale * d loss / d b.
 * loss[0] is unscaled, and its bits do not depend on which gradients are asked for.
 *
 * The workspace holds one double per workgroup of the forward pass and four coefficient volumes (c_s11 = c_s22): a function
 * of the shape and the window alone.  modet_ssim_ws_bytes is 0 for bad arguments (a size < 1, a window that is not odd or
 * not in 1..11, more than 2^31 - 1 voxels in all).  A window that is even or outside 1..11 is MODET_ERR_UNSUPPORTED.  The
 * workspace begins with doubles: ws must be 8-byte aligned, a misaligned one is MODET_ERR_WORKSPACE like a short one.  Every
 * check happens before the first launch. */
size_t modet_ssim_ws_bytes(int B, int D, int H, int W, int window);
int modet_ssim_fwd_bwd(const float* a, const float* b, float* loss, float* d_a, float* d_b, void* ws, size_t ws_bytes, int B,
                       int D, int H, int W, int window, float grad_scale, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
