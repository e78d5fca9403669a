/* libmodet_hip.so -- trilinear resizing of a channels-last volume between ANY two grids, times a scalar: ATen's
 * upsample_trilinear3d(align_corners=True), which is what nnf.interpolate(mode='trilinear', align_corners=True) runs in either
 * direction, and with it the reference's ResizeTransform and the flow pyramid of a recursive RDN stage ("Baseline methods/RDN/
 * models.py":91-117, :371-377, :480-486) -- next to the core ABI of modet_hip.h and the families of modet_hip_losses.h,
 * modet_hip_mi.h, modet_hip_ssim.h, modet_hip_reg.h, modet_hip_vecint.h, modet_hip_surface.h, modet_hip_posenc.h,
 * modet_hip_convs2.h, modet_hip_deconv.h, modet_hip_pcnet.h and modet_hip_prpp.h (all twelve stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs, an explicit stream, nothing synchronises, return 0 =
 * ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only enqueues ONE kernel: no host
 * read-back, no allocation, no workspace, no memset node, no float atomics -- a call can be captured into a hipGraph, two runs on
 * the same inputs are bit-identical, and a batch of two gives the bits of two batches of one.  Everything is fp32 and
 * channels-last; element offsets are 64-bit.  All argument checks are answered before the launch.
 */
#ifndef MODET_HIP_RESIZE_H
#define MODET_HIP_RESIZE_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_RESIZE_MAX_C = 256 };
enum { MODET_RESIZE_PYRAMID_MIN = 8 };       /* the shortest axis the pyramid takes: its 1/8 output then has one voxel */

/* THE FUNCTION.  x is (B,Di,Hi,Wi,C), y is (B,Do,Ho,Wo,C).  Per axis, with Si the input and So the output size and p the output
 * index, all in fp32:
 *     r  = So > 1 ? (float)(Si - 1) / (float)(So - 1) : 0
 *     c  = r * (float)p                     (one rounding: never contracted with the subtraction below)
 *     i0 = min((int)c, Si - 1),  i1 = min(i0 + 1, Si - 1),  l = c - (float)i0
 *     y[p] = scale * sum over the 8 corners (dz, dy, dx) = (0,0,0), (0,0,1) .. (1,1,1) of w * x[corner],
 *            w = (wz * wy) * wx,  w_axis = dz ? l : 1 - l,  the sum by fused multiply-adds into a zero accumulator in that order.
 * Down, up, identity, So == 1 (the output is x at index 0 of that axis) and Si == 1 are all legal.  With integer ratios every
 * l is 0 and y = scale * x[r p] exactly.  The forward and both backwards take (i0, i1, l) from ONE device function.
 *
 * modet_resize_fwd: one thread per output voxel and group of channels: with C % 4 == 0 and x and y 16-byte aligned a QUAD with
 * 16-byte loads and stores, otherwise (4-byte alignment is then enough) 3, 2 or 1 channels, whichever divides C, float by float.
 * The arithmetic per channel is the same in every form: the same bits.
 *
 * modet_resize_bwd: d_x = (d y / d x)^T d_y as a GATHER, one thread per input voxel and group of channels (as above): per axis
 * it walks a conservative window of output indices around q / r, keeps those whose (i0, i1) name the input index q, with the
 * weight (i0 == q ? 1 - l : 0) + (i1 == q ? l : 0), and sums w * d_y by fused multiply-adds in ascending (pz, py, px) order;
 * d_x = scale * that sum.  Downsampling by 2 or more an input index lies in at most one output's stencil per axis, for an identity
 * resize in two, for 2 -> 9 in nine: the loop is general and short on the network's path.
 *
 * Refused before the launch: a NULL pointer (MODET_ERR_NULL); a size < 1, C outside [1, MODET_RESIZE_MAX_C], B outside
 * [1, 65535], a non-finite scale (MODET_ERR_DIM). */
int modet_resize_fwd(const float* x, float* y, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C, float scale,
                     modet_stream_t stream);
int modet_resize_bwd(const float* d_y, float* d_x, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C, float scale,
                     modet_stream_t stream);

/* THE FLOW PYRAMID of a recursive stage: a 3-channel field x (B,D,H,W,3) is read once and its three rescaled downsamplings are
 * written by ONE launch,
 *     y2 = 0.5   * resize(x -> floor(S / 2)),  y4 = 0.25 * resize(x -> floor(S / 4)),  y8 = 0.125 * resize(x -> floor(S / 8))
 * (floor(S * factor) is the output size of nnf.interpolate(scale_factor=factor)).  Each output holds the bits modet_resize_fwd
 * writes for the same sizes and scale.  Any of the three outputs may be NULL (not wanted, not written); all three NULL is
 * MODET_ERR_NULL.  Every S >= MODET_RESIZE_PYRAMID_MIN and B in [1, 65535], else MODET_ERR_DIM.
 *
 * modet_resize_pyramid_bwd: one gather launch, d_x = [d_x_add +] g2 + g4 + g8 in that fixed order, g_k the gradient
 * modet_resize_bwd computes from d_y_k; NULL cotangents are skipped (all three NULL is MODET_ERR_NULL) and with a single one and
 * no d_x_add the call writes the bits of modet_resize_bwd.  d_x_add (B,D,H,W,3), optional, is another gradient of the same field
 * to fold into this launch; it may alias d_x (every thread reads its element before it writes it). */
int modet_resize_pyramid_fwd(const float* x, float* y2, float* y4, float* y8, int B, int D, int H, int W, modet_stream_t stream);
int modet_resize_pyramid_bwd(const float* d_y2, const float* d_y4, const float* d_y8, const float* d_x_add, float* d_x, int B,
                             int D, int H, int W, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
