/* libmodet_hip.so -- the pieces of the PR++ baseline ("Baseline methods/PR++/models.py", PRNetplusplus) that no other family
 * has: the decoder's input (nearest upsampling by 2 and the concatenation with the skip in one pass), ReLU and the block's
 * x + relu(res), the block's stack [x_warped | correlation | y] as one channels-last row, and the composition of a flow that lives
 * on a COARSER grid with a field on the finer one -- next to the core ABI of modet_hip.h and the families of modet_hip_losses.h,
 * modet_hip_mi.h, modet_hip_ssim.h, modet_hip_reg.h, modet_hip_vecint.h, modet_hip_surface.h, modet_hip_posenc.h,
 * modet_hip_convs2.h, modet_hip_deconv.h and modet_hip_pcnet.h (all eleven stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no allocation, no memset node, no float atomics -- a call can be captured into a hipGraph,
 * two runs on the same inputs are bit-identical, and a batch of two gives the bits of two batches of one.  Everything is fp32 and
 * channels-last; element offsets are 64-bit.  All argument checks are answered before the first launch.
 */
#ifndef MODET_HIP_PRPP_H
#define MODET_HIP_PRPP_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_PRPP_MAX_C = 128 };             /* channels of ONE of the two feature maps of a stack; a row has 2 C + 27 floats */
enum { MODET_PRPP_CORR = 27 };               /* displacements of Correlation3D(kernel_size 3, d 3, sw 1, sf 2) */

/* DECODER INPUT, nn.Upsample(scale_factor=2) (nearest) + torch.cat([up, skip], 1).  x is (B,d,h,w,C1), skip (B,2d,2h,2w,C2), out
 * (B,2d,2h,2w,C1+C2): out[p, :C1] = x[floor(p / 2)], out[p, C1:] = skip[p].  Any C1, C2 >= 1; with C1 and C2 multiples of 4 AND
 * every tensor 16-byte aligned the rows move as 16-byte loads and stores, otherwise (4-byte alignment is then enough) one float
 * at a time inside its row.  Backward: d_x[q] = the sum of the first C1 floats of its eight children's rows, in the fixed order
 * (dz, dy, dx) = (0,0,0), (0,0,1) .. (1,1,1), one thread per (coarse voxel, channel quad): a gather; d_skip = the last C2 floats.
 * d_x or d_skip may be NULL (not wanted, not written); both NULL is MODET_ERR_NULL.  B, d, h, w >= 1 (else MODET_ERR_DIM). */
int modet_prpp_upcat_fwd(const float* x, const float* skip, float* out, int B, int d, int h, int w, int C1, int C2,
                         modet_stream_t stream);
int modet_prpp_upcat_bwd(const float* d_out, float* d_x, float* d_skip, int B, int d, int h, int w, int C1, int C2,
                         modet_stream_t stream);

/* RELU.  y = max(t, 0) over n floats (y may be t); out = x + max(t, 0) (out may be x or t); d_t = d_y where y_or_t > 0, else 0
 * (d_t may be d_y; y > 0 <=> t > 0, so either the output or the input of the forward serves; the gradient at 0 is 0).  A NaN
 * passes through, as in ATen.  Four elements per thread with 16-byte accesses and a scalar tail of n % 4 floats; every tensor
 * 16-byte aligned (else MODET_ERR_UNSUPPORTED), n >= 1 (else MODET_ERR_DIM).  The gradient of relu_add with respect to x is
 * d_out itself: no kernel. */
int modet_prpp_relu_fwd(const float* t, float* y, int64_t n, modet_stream_t stream);
int modet_prpp_relu_add_fwd(const float* x, const float* t, float* out, int64_t n, modet_stream_t stream);
int modet_prpp_relu_bwd(const float* d_y, const float* y_or_t, float* d_t, int64_t n, modet_stream_t stream);

/* THE BLOCK'S STACK, torch.cat([mov, Correlation3D(mov, fix), fix], 1) as rows [mov (C) | corr (27) | fix (C)] of 2 C + 27
 * floats, out (B,D,H,W,2C+27).  corr is modet_corr3d_fwd's function, from the same kernels (box sums with the one-voxel ring of
 * fix, 27 displacements of stride 2, the factor 1/27): the middle slice holds the bits modet_corr3d_fwd writes into its planes.
 * The rows are not 16-byte aligned: the 27 values of a voxel go through LDS and are stored as one contiguous run.
 * Backward: d_mov = d_out[.., :C] + (the correlation's gradient with respect to mov), d_fix = d_out[.., C+27:] + (.. fix); the
 * correlation's cotangent is read from the strided middle slice.  d_mov or d_fix may be NULL; both NULL is MODET_ERR_NULL.
 * LIMITS.  C a multiple of 4 in [4, MODET_PRPP_MAX_C] and fewer than 2^31 elements on the ring-extended grid (else
 * MODET_ERR_UNSUPPORTED), B, D, H, W >= 1 (MODET_ERR_DIM); mov, fix, d_mov, d_fix 16-byte aligned, out and d_out 4-byte
 * (MODET_ERR_UNSUPPORTED); the workspace 16-byte aligned and at least modet_prpp_stack_ws_bytes bytes (MODET_ERR_WORKSPACE),
 * which is the exact size (the forward uses the first half) and 0 for arguments that are refused. */
size_t modet_prpp_stack_ws_bytes(int B, int D, int H, int W, int C);
int modet_prpp_stack_fwd(const float* mov, const float* fix, float* out, void* ws, size_t ws_bytes, int B, int D, int H, int W,
                         int C, modet_stream_t stream);
int modet_prpp_stack_bwd(const float* mov, const float* fix, const float* d_out, float* d_mov, float* d_fix, void* ws,
                         size_t ws_bytes, int B, int D, int H, int W, int C, modet_stream_t stream);

/* CROSS-GRID COMPOSITION, SpatialTransformer(fine size)(src, w) + w with src on another (coarser) grid.  src is (B,Dc,Hc,Wc,3),
 * w and out (B,Df,Hf,Wf,3):
 *     out[p] = w[p] + trilinear(src, c),   c_i = (p_i + w[p,i]) * (Sc_i - 1) / (Sf_i - 1)
 * -- the field is added to the FINE identity grid and normalised by the FINE sizes, grid_sample(align_corners=True, zeros
 * padding) then spans the coarse tensor: corners outside the coarse grid contribute zero.  Channel i displaces axis i.  The
 * coarse flow is not rescaled.  With Sf == Sc the ratio is exactly 1 and the call computes modet_warp_fwd(add_flow = 1), bit for
 * bit.
 * Backward: d_w[p,i] = d_out[p,i] + ratio_i * sum over ch of d_out[p,ch] * d tri(src[..,ch], c) / d c_i, one thread per fine
 * voxel.  d_src is the scatter onto the coarse field (w is unbounded: no gather exists) as modet_warp_bwd_det does it: every
 * contribution becomes a 64-bit fixed-point integer, whose unit is a power of two taken from the SAMPLE's max |d_out| (a first pass)
 * and the voxel count so that no sum can overflow, the sums are integer additions whose order cannot matter, a last pass converts to
 * float.  d_src or d_w may be NULL; both NULL is MODET_ERR_NULL.  The workspace (the int64 sums and a header) is needed for
 * d_src only: 16-byte aligned, at least modet_prpp_compose_ws_bytes(B, Dc, Hc, Wc) = 64 ceil(B / 16) + 24 B Dc Hc Wc bytes
 * (MODET_ERR_WORKSPACE; 0 for arguments that are refused).
 * LIMITS.  B in [1, 65535], every Sc_i >= 1 and every Sf_i >= 2 (else MODET_ERR_DIM); tensors 4-byte aligned. */
size_t modet_prpp_compose_ws_bytes(int B, int Dc, int Hc, int Wc);
int modet_prpp_compose_fwd(const float* src, const float* w, float* out, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf,
                           modet_stream_t stream);
int modet_prpp_compose_bwd(const float* src, const float* w, const float* d_out, float* d_src, float* d_w, void* ws,
                           size_t ws_bytes, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
