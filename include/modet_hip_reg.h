/* libmodet_hip.so -- the flow regularisers beside Grad3d: the isotropic total variation and the displacement energies (gradient
 * norms and bending energy), next to the core ABI of modet_hip.h and the loss families of modet_hip_losses.h, modet_hip_mi.h and
 * modet_hip_ssim.h (all four stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no memset node, no float atomics -- a call can be captured into a hipGraph and two runs
 * on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_REG_H
#define MODET_HIP_REG_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_REG_ITV = 0, MODET_REG_GRADIENT_L2 = 1, MODET_REG_GRADIENT_L1 = 2, MODET_REG_BENDING = 3 };

/* Four regularisers of a flow f[b,c,z,y,x] (reference Baseline methods/RCN/losses.py:203-221, Grad3DiTV, and :223-268,
 * DisplacementRegularizer).  e_a is the unit step along axis a of (z, y, x); "mean" is the plain average over the points named.
 *
 * MODET_REG_ITV, any C >= 1 and D, H, W >= 2, on the points p with z, y, x >= 1:
 *     d_a(p) = f[p] - f[p - e_a]
 *     loss   = mean( sqrt(d_z^2 + d_y^2 + d_x^2 + 1e-6) ) / 3              over B C (D-1)(H-1)(W-1) points
 *   The 1e-6 sits under the root: a zero flow has the loss 1e-3 / 3 and the gradient 0.
 *
 * MODET_REG_GRADIENT_L2 and _L1, C = 3 and D, H, W >= 3, on the points p at least 1 from every face:
 *     g_a(p) = (f[p + e_a] - f[p - e_a]) / 2
 *     loss   = mean( g_z^2 + g_y^2 + g_x^2 ) / 3     (L2)                  over B 3 (D-2)(H-2)(W-2) points
 *     loss   = mean( |g_z| + |g_y| + |g_x| ) / 3     (L1);  the derivative of |t| at t = 0 is 0
 *
 * MODET_REG_BENDING, C = 3 and D, H, W >= 5, on the points p at least 2 from every face:
 *     s_aa(p) = (f[p + 2 e_a] - 2 f[p] + f[p - 2 e_a]) / 4
 *     s_ab(p) = (f[p + e_a + e_b] - f[p + e_a - e_b] - f[p - e_a + e_b] + f[p - e_a - e_b]) / 4
 *     loss    = mean( s_zz^2 + s_yy^2 + s_xx^2 + 2 s_zy^2 + 2 s_zx^2 + 2 s_yx^2 )     over B 3 (D-4)(H-4)(W-4) points, no / 3
 *
 * The gradient is the adjoint of these stencils with the terms of points outside their grid absent.  For bending that is a
 * 25-point stencil on f (offsets 0, +-2 e_a, +-4 e_a, +-2 e_a +-2 e_b) whose coefficients are constant for voxels at least 4 from
 * every face and depend on the position nearer to one.
 *
 * f is (B,C,D,H,W) planar, or (B,D,H,W,C) when channels_last != 0, which requires C = 3.  d_f may be NULL; otherwise it has the
 * layout of f and receives grad_scale * d loss / d f, the product of grad_scale and the mean's factor applied once, at the store.
 * loss[0] is unscaled, and its bits do not depend on whether d_f is given.
 *
 * The workspace holds one double per workgroup of the launch and nothing else: at most 2048 of them, 16 KiB, for every kind and
 * shape; no volume is staged.  modet_reg_ws_bytes depends on the kind and the shape alone and is 0 for bad arguments (an unknown
 * kind, a size < 1, an axis shorter than the kind's minimum, C != 3 for a displacement kind, more than 2^31 - 1 elements).
 * An unknown kind is MODET_ERR_UNSUPPORTED; an axis below the minimum, a wrong channel count (C != 3 with channels_last
 * included) or more than 2^31 - 1 elements MODET_ERR_DIM.  The workspace begins with doubles: ws must be 8-byte aligned, a
 * misaligned one is MODET_ERR_WORKSPACE like a short one.  Every check happens before the first launch. */
size_t modet_reg_ws_bytes(int kind, int B, int C, int D, int H, int W);
int modet_reg_fwd_bwd(const float* f, float* loss, float* d_f, void* ws, size_t ws_bytes, int kind, int B, int C, int D, int H,
                      int W, int channels_last, float grad_scale, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
