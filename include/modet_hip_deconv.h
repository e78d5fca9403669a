/* libmodet_hip.so -- the 4x4x4 transposed convolution with stride 2 and padding 1 that upsamples in the decoders of the RCN / VTN
 * and PCNet baselines (nn.ConvTranspose3d(cin, cout, kernel_size=4, stride=2, padding=1) [+ LeakyReLU]: "Baseline methods/RCN/
 * models.py" writes it as ConvTranspose3d(4, stride=2) followed by the crop [1:-1] of every axis, which is the same function),
 * next to the core ABI of modet_hip.h and the families of modet_hip_losses.h, modet_hip_mi.h, modet_hip_ssim.h, modet_hip_reg.h,
 * modet_hip_vecint.h, modet_hip_surface.h, modet_hip_posenc.h and modet_hip_convs2.h (all nine stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no allocation, no memset node, no atomics -- a call can be captured into a hipGraph and
 * two runs on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_DECONV_H
#define MODET_HIP_DECONV_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_DECONV_MAX_CHANNELS = 1024 };
enum { MODET_DECONV_PASS_FWD = 0, MODET_DECONV_PASS_BWD_DATA = 1, MODET_DECONV_PASS_BWD_WEIGHT = 2 };

/* THE LAYER.  x is (B,D,H,W,Cin) fp32 channels-last, y is (B,2D,2H,2W,Cout); w is nn.ConvTranspose3d's parameter
 * (Cin,Cout,4,4,4), bias (Cout) or NULL.  Per axis, output index o receives tap k of input i = (o + 1 - k) / 2 where o + 1 - k is
 * even and 0 <= i < n: an even o takes taps 1 and 3 of inputs o / 2 and o / 2 - 1, an odd o taps 0 and 2 of inputs (o + 1) / 2 and
 * (o - 1) / 2:
 *     z[b,o,co] = bias[co] + sum over those taps k in {0..3}^3 and ci of  w[ci,co,k] * x[b, (o + 1 - k) / 2, ci]
 *     y = z (act == 0)   or   y = z > 0 ? z : slope * z (act == 1; slope >= 0, 0 gives ReLU)
 * All arithmetic is fp32 fused multiply-add on the values as they are: there is no reduced-precision form (the 3-channel layers
 * carry flows and the last one produces the network's output).  The bias is added last.
 *
 * THE FOLDED DERIVATIVE, as in modet_hip_convs2.h.  The backward entry points take the gradient d_y with respect to y and, when
 * act == 1, y itself: g = d_y * (y > 0 ? 1 : slope) is formed while d_y is loaded.  The kernels keep the two classes apart,
 * P = sum over y > 0 and Q = sum over y <= 0 of d_y * (the other factor), and finish with ONE rounding of P + slope * Q, so where
 * every product and sum is exactly representable (small integers) the results are the exact ones for any slope.  act == 0: y is
 * not read and may be NULL.
 *
 * modet_deconv4s2_fwd: y as above, eight parity classes, each a 2x2x2 stride-1 gather (K = 8 Cin): no scatter.  A workgroup owns
 *   a 3-D tile of input voxels (4x8x8, 4x4x8 or 4x4x4 for up to 4, up to 8 or more output channels per workgroup) and 4, 8 or 16
 *   output channels; it stages the tile plus a one-voxel halo in LDS, 16 input channels at a time, and every thread forms the
 *   2x2x2 output voxels of its input voxel, all eight parity classes from the one window.  ws (pass 0): the weights re-laid as
 *   [tap][ci][co], both channel counts padded with zeros to multiples of 4, by a first launch.
 *
 * modet_deconv4s2_bwd_data: d_x[i,ci] = sum over k in {0..3}^3 and co of g[2 i - 1 + k, co] * w[ci,co,k], a 4x4x4 stride-2 gather
 *   with padding 1.  A workgroup owns a tile of input voxels (4x4x4, or 4x4x8 up to Cin = 8) and stages the d_y (and y) window of
 *   2 T + 2 voxels per axis in LDS, 4 output channels at a time, already split into its P and Q parts; all 64 taps read it.
 *   EVERY element of d_x is written.  ws (pass 1): the weights as [tap][co][ci], padded alike.
 *
 * modet_deconv4s2_bwd_weight: d_w (Cin,Cout,4,4,4) and d_b (Cout; NULL = not wanted) from x, d_y and y.  Stage 1: workgroup
 *   (s, j) sums its 256 (tap, 4 ci, 4 co) items over the input voxels [s V, (s + 1) V), V = max(256, ceil(B D H W / 256)), and
 *   writes a partial row (two with act == 1: P and Q) of 64 Cin' Cout' + Cout' floats into ws (Cin', Cout': the counts rounded up
 *   to multiples of 4).  Stage 2: one fixed-order fp64 column sum over the rows, then P + slope * Q in fp64, rounded once.
 *   ws (pass 2): 2 rows per voxel split.
 *
 * LIMITS.  Cin and Cout are 1 .. MODET_DECONV_MAX_CHANNELS: a count that is a multiple of 4 takes 16-byte loads and stores, any
 * other a scalar tail that stays inside its tensor.  act is 0 or 1, slope >= 0 (act == 1); else MODET_ERR_UNSUPPORTED.  B, D, H or
 * W < 1, Cin or Cout < 1, x or y of 2^31 elements or more: MODET_ERR_DIM.  A required pointer that is NULL: MODET_ERR_NULL.
 * x / d_x must be 16-byte aligned when Cin % 4 == 0, y / d_y when Cout % 4 == 0, every other tensor 4-byte aligned, else
 * MODET_ERR_UNSUPPORTED.  A short workspace or one not 16-byte aligned: MODET_ERR_WORKSPACE.  All are answered before the first
 * launch.  modet_deconv4s2_ws_bytes is the exact size a pass needs and 0 for every shape (or pass number) that is refused. */
size_t modet_deconv4s2_ws_bytes(int B, int D, int H, int W, int Cin, int Cout, int pass);
int modet_deconv4s2_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int D, int H,
                        int W, int Cin, int Cout, int act, float slope, modet_stream_t stream);
int modet_deconv4s2_bwd_data(const float* d_y, const float* y, const float* w, float* d_x, void* ws, size_t ws_bytes, int B, int D,
                             int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream);
int modet_deconv4s2_bwd_weight(const float* x, const float* d_y, const float* y, float* d_w, float* d_b, void* ws, size_t ws_bytes,
                               int B, int D, int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
