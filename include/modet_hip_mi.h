/* libmodet_hip.so -- the mutual-information losses beside the core ABI of modet_hip.h and the loss family of
 * modet_hip_losses.h (both stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no memset node, no float atomics -- a call can be captured into a hipGraph and two runs
 * on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_MI_H
#define MODET_HIP_MI_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Mutual information with Parzen windows (reference Baseline methods/RCN/losses.py:401-556, MutualInformation and
 * localMutualInformation).  a = y_true and b = y_pred are (B,1,D,H,W) = (B,D,H,W) fp32 planar, any D, H, W >= 1, N = D H W.
 *
 *   c_j     = the 32 values of an fp32 linspace(minval, maxval, 32) (computed on the host, as torch.linspace computes them)
 *   sigma   = (maxval - minval) / 31 * sigma_ratio,  preterm = 1 / (2 sigma^2)
 *   x'      = min(max(x, 0), maxval)                 (the lower bound is 0, not minval, as in the reference)
 *   w_j(x)  = exp(-preterm (x' - c_j)^2),  I_j(x) = w_j / sum_j w_j
 *   per batch element: pab = I_a^T I_b / N,  pa = mean_k I_a,  pb = mean_k I_b,  papb = pa (x) pb + 1e-6,
 *                      mi = sum_ij pab log(pab / papb + 1e-6);      loss = -mean_b mi
 *   local form: every axis of n voxels is zero-padded AFTER the clamp by r = -n mod p, r / 2 voxels on the low side, and the
 *   padded volume is cut into non-overlapping p^3 patches; the formula runs per patch with N = p^3 (padding voxels count as
 *   value 0); loss = -mean over all patches of all batch elements.
 *
 * Gradient rules are ATen's: the clamp passes gradient where 0 <= x <= maxval (both ends inclusive) and zero elsewhere;
 * padding voxels receive none.  d_a and d_b (same shape as a and b) may each be NULL; they receive grad_scale * d loss / d a
 * and grad_scale * d loss / d b.  loss[0] is unscaled.
 *
 * Nothing per voxel and bin is ever stored: the global form's workspace holds one 32 x 32 histogram partial per 4096 voxels,
 * the local form's one float per patch.  modet_mi_ws_bytes: patch_size 0 = the global form, 1..16 = the local form; 0 bytes
 * for bad arguments.  Only num_bins = 32 exists; it, maxval <= 0, maxval <= minval, sigma_ratio <= 0 and a patch_size
 * outside 1..16 are MODET_ERR_UNSUPPORTED.  The global form's workspace begins with doubles: ws must be 8-byte aligned (4-byte
 * for the local form), a misaligned one is MODET_ERR_WORKSPACE like a short one.  Every check happens before the first launch.
 *
 * sigma_ratio has a practical lower limit: the weights are fp32, so once sigma is small enough that a voxel between two centres
 * is more than about 13 sigma from both (sigma_ratio below about 0.04) all 32 weights underflow, the normaliser is 0 and the
 * result is NaN -- as in the fp32 ATen composition, which this follows; such values are accepted and not special-cased. */
size_t modet_mi_ws_bytes(int B, int D, int H, int W, int patch_size);
int modet_mi_fwd_bwd(const float* a, const float* b, float* loss, float* d_a, float* d_b, void* ws, size_t ws_bytes, int B,
                     int D, int H, int W, int num_bins, float minval, float maxval, float sigma_ratio, float grad_scale,
                     modet_stream_t stream);
int modet_lmi_fwd_bwd(const float* a, const float* b, float* loss, float* d_a, float* d_b, void* ws, size_t ws_bytes, int B,
                      int D, int H, int W, int num_bins, float minval, float maxval, float sigma_ratio, int patch_size,
                      float grad_scale, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
