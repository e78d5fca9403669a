/* libmodet_hip.so -- the stride-2 3x3x3 convolution that opens the encoders of the RDN, PCNet and PR++ baselines
 * (nn.Conv3d(cin, cout, 3, stride=2, padding=1) + LeakyReLU: "Baseline methods/RDN/models.py":172-192, "PCnet/models.py":189-215,
 * "PR++/models.py":132-148) and the two-tensor channel concatenation of RDN's Estimator, next to the core ABI of modet_hip.h and
 * the families of modet_hip_losses.h, modet_hip_mi.h, modet_hip_ssim.h, modet_hip_reg.h, modet_hip_vecint.h, modet_hip_surface.h
 * and modet_hip_posenc.h (all eight stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no allocation, no memset node, no atomics -- a call can be captured into a hipGraph and
 * two runs on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_CONVS2_H
#define MODET_HIP_CONVS2_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_CONVS2_MAX_CHANNELS = 256 };
enum { MODET_CONVS2_PASS_FWD = 0, MODET_CONVS2_PASS_BWD_DATA = 1, MODET_CONVS2_PASS_BWD_WEIGHT = 2 };

/* THE LAYER.  x is (B,D,H,W,Cin) fp32 channels-last, y is (B,Do,Ho,Wo,Cout) with Do = (D - 1) / 2 + 1 (integer division), Ho and
 * Wo alike; w is nn.Conv3d's parameter (Cout,Cin,3,3,3), bias (Cout) or NULL:
 *     z[b,o,co] = bias[co] + sum over taps k in {0,1,2}^3 and ci of  w[co,ci,k] * x[b, 2 o - 1 + k, ci]
 *     y = z (act == 0)   or   y = z > 0 ? z : slope * z (act == 1; slope >= 0, 0 gives ReLU)
 * Input index -1 is padding, and for an odd dimension n index n is padding too; an even dimension has none at its high end.
 * All arithmetic is fp32 fused multiply-add on the values as they are: no reduced-precision form and no assumption about the
 * range of x (the first encoder layer reads the raw image).  Sums run over 4 interleaved chains per tap, the taps are added in
 * tap order, the bias is added last.
 *
 * THE FOLDED DERIVATIVE.  The backward entry points take the gradient d_y with respect to y and, when act == 1, y itself: the
 * activation's derivative comes from the sign of y while d_y is loaded, g = d_y * (y > 0 ? 1 : slope).  The kernels keep the two
 * classes apart, P = sum over y > 0 and Q = sum over y <= 0 of d_y * (the other factor), and finish with ONE rounding of
 * P + slope * Q.  Where every product and sum is exactly representable (small integers) the results are therefore the exact
 * ones for any slope.  act == 0: y is not read and may be NULL.
 *
 * modet_convs2_fwd: y as above.  ws (pass 0): the weights re-laid as [tap][ci][co] by a first launch.
 *
 * modet_convs2_bwd_data: d_x (B,D,H,W,Cin), a gather with one thread per input voxel and 4 input channels: per axis an even
 *   index receives tap 1 of output i / 2 and an odd index taps 0 and 2 of outputs (i + 1) / 2 and (i - 1) / 2 -- eight parity
 *   classes with 1, 2, 4 or 8 taps, outputs beyond Do / Ho / Wo dropped.  EVERY element of d_x is written (the rows beyond the last
 *   output of an odd dimension included).  No atomics, no zero-dilated copy of d_y.  ws (pass 1): the weights as [tap][co][ci].
 *
 * modet_convs2_bwd_weight: d_w (Cout,Cin,3,3,3) and d_b (Cout; NULL = not wanted) from x, d_y and y.  Stage 1: workgroup (i, s)
 *   sums its 256 (tap, 4 ci, 4 co) items over the output voxels [s * V, (s + 1) * V) -- V = 256 up to Cout = 64, 512 up to 128,
 *   1024 beyond -- and writes a partial row (two with act == 1: P and Q) of 27 Cin Cout + Cout floats into ws.  Stage 2: one
 *   fixed-order fp64 column sum over the rows, then P + slope * Q in fp64, rounded once.  ws (pass 2): 2 rows per voxel split.
 *
 * modet_cat_channels2_fwd: out (N, C1 + C2) with out[n, :C1] = a[n], out[n, C1:] = b[n];  modet_cat_channels2_bwd: the split of
 *   d_out back into d_a (N, C1) and d_b (N, C2); d_a or d_b may be NULL (not written), not both.  N voxels (rows), any C1, C2 >= 1;
 *   16-byte vectors when both are multiples of 4.
 *
 * LIMITS.  Cin is 1 or a multiple of 4, Cout a multiple of 4, both at most MODET_CONVS2_MAX_CHANNELS, act is 0 or 1, slope >= 0
 * (act == 1), else MODET_ERR_UNSUPPORTED.  B, D, H or W < 1, x or y of 2^31 elements or more (the concatenation: out of 2^31
 * elements or more), C1 or C2 < 1: MODET_ERR_DIM.  A required pointer that is NULL: MODET_ERR_NULL.  x / d_x (Cin > 1), y, d_y,
 * and with C1 % 4 == C2 % 4 == 0 the concatenation's tensors, must be 16-byte aligned, every other tensor 4-byte aligned, else
 * MODET_ERR_UNSUPPORTED.  A short workspace or one not 16-byte aligned: MODET_ERR_WORKSPACE.  All are answered before the first
 * launch.  modet_convs2_ws_bytes is the exact size a pass needs and 0 for every shape (or pass number) that is refused. */
size_t modet_convs2_ws_bytes(int B, int D, int H, int W, int Cin, int Cout, int pass);
int modet_convs2_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, size_t ws_bytes, int B, int D, int H,
                     int W, int Cin, int Cout, int act, float slope, modet_stream_t stream);
int modet_convs2_bwd_data(const float* d_y, const float* y, const float* w, float* d_x, void* ws, size_t ws_bytes, int B, int D,
                          int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream);
int modet_convs2_bwd_weight(const float* x, const float* d_y, const float* y, float* d_w, float* d_b, void* ws, size_t ws_bytes,
                            int B, int D, int H, int W, int Cin, int Cout, int act, float slope, modet_stream_t stream);
int modet_cat_channels2_fwd(const float* a, const float* b, float* out, int64_t N, int C1, int C2, modet_stream_t stream);
int modet_cat_channels2_bwd(const float* d_out, float* d_a, float* d_b, int64_t N, int C1, int C2, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
