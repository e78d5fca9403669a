/* libmodet_hip.so -- the similarity-loss family beside the core ABI of modet_hip.h (which stays frozen).
 *
 * Same conventions as modet_hip.h: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit
 * stream, nothing synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.
 * Every entry point only enqueues kernels: no host read-back, no memset node, no float atomics -- a sequence of calls can be
 * captured into a hipGraph and two runs on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_LOSSES_H
#define MODET_HIP_LOSSES_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MIND-SSC (Heinrich et al., MICCAI 2013; reference Baseline methods/RCN/losses.py:333-399, MIND_loss).
 * Images are (B,1,D,H,W) = (B,D,H,W) fp32 planar, any D, H, W >= 1 (every neighbour access is clamped into the volume =
 * replication padding).  Only radius = 2 (the 5^3 box) and dilation = 2 (the six-neighbourhood's reach) exist, as the
 * reference hard-codes them: anything else is MODET_ERR_UNSUPPORTED.
 *
 *   six neighbours n0..n5 = (0,1,1) (1,1,0) (1,0,1) (1,1,2) (2,1,1) (1,2,1) in (z,y,x); twelve channels = the ordered pairs
 *   (i,j), i > j, |n_i - n_j|^2 = 2, row-major: (1,0) (2,0) (2,1) (3,0) (3,2) (4,1) (4,2) (4,3) (5,0) (5,1) (5,3) (5,4)
 *   d_c(p)   = I(clamp(p + 2 (n_i - 1))) - I(clamp(p + 2 (n_j - 1)))
 *   ssd_c(p) = 1/125 sum_{o in {-2..2}^3} d_c^2(clamp(p + o))
 *   m_c = ssd_c - min_c ssd_c,  v = mean_c m_c,  g = mean of v over all B D H W voxels of the tensor,
 *   mind_c = exp(-m_c / min(max(v, 0.001 g), 1000 g))
 *
 * modet_mind_ws_bytes(..., images): images = 1 for modet_mind_descriptor, 2 for modet_mind_fwd_bwd; 0 for bad arguments.
 * modet_mind_descriptor: mind (B,12,D,H,W) in the reference's output channel order (its final permutation
 *   [6,8,1,11,2,10,0,7,9,4,5,3] of the twelve channels above).
 * modet_mind_fwd_bwd: loss[0] = mean over B 12 D H W of (mind(a) - mind(b))^2;  d_b (same shape as b) = grad_scale *
 *   d loss / d b, or NULL for the value alone.  The loss is symmetric: the gradient for a is the call with a and b swapped.
 *   Gradient rules are ATen's: the two clamp bounds are constants (nothing flows through g), v passes gradient where it lies
 *   within the bounds, the channel minimum routes to the lowest-index argmin channel.  g and the bounds stay in device memory. */
size_t modet_mind_ws_bytes(int B, int D, int H, int W, int images);
int modet_mind_descriptor(const float* img, float* mind, void* ws, size_t ws_bytes, int B, int D, int H, int W, int radius,
                          int dilation, modet_stream_t stream);
int modet_mind_fwd_bwd(const float* a, const float* b, float* loss, float* d_b, void* ws, size_t ws_bytes, int B, int D, int H,
                       int W, int radius, int dilation, float grad_scale, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
