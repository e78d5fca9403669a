/* libmodet_hip.so -- the pieces of the PCNet baseline ("Baseline methods/PCnet/models.py") that are pure memory traffic: the
 * trilinear upsampling of a 3-channel field by 2, 4 or 8 into a slice of a wider row (DFIBlock.upsample + torch.cat), DFI's gated
 * sum, the tail of the NFF block (3-way voxel softmax, concatenation, global average / max pooling, the two-layer channel gate and
 * the rescale) and ResBlock's residual sum -- next to the core ABI of modet_hip.h and the families of modet_hip_losses.h,
 * modet_hip_mi.h, modet_hip_ssim.h, modet_hip_reg.h, modet_hip_vecint.h, modet_hip_surface.h, modet_hip_posenc.h,
 * modet_hip_convs2.h and modet_hip_deconv.h (all ten stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no allocation, no memset node, no atomics -- a call can be captured into a hipGraph, two
 * runs on the same inputs are bit-identical, and a batch of two gives the bits of two batches of one (the parameter gradients
 * d_W1 / d_W2, sums over the batch, excepted).  Everything is fp32 and channels-last.
 */
#ifndef MODET_HIP_PCNET_H
#define MODET_HIP_PCNET_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_PCNET_MAX_C = 256 };            /* channels of ONE of the three NFF maps; the concatenation has 3 C */
enum { MODET_PCNET_NFF_PASS_POOL = 0, MODET_PCNET_NFF_PASS_BWD_GATE = 1, MODET_PCNET_NFF_PASS_GATE_PARAMS = 2 };

/* UPSAMPLING BY f in {2, 4, 8}, nn.Upsample(scale_factor=f, mode='trilinear', align_corners=True).  x is (B,d,h,w,3); y has
 * B * fd * fh * fw rows of ld floats (ld = 3, 6 or 9) of which the call owns channels [off, off + 3), off + 3 <= ld: the other
 * channels of a row are neither read nor written, so the upsamplings of a DFI block land in the convolution's input directly.
 * Per axis, output o reads inputs i0 = (o (n - 1)) / (f n - 1) and min(i0 + 1, n - 1) with the weights 1 - t and t,
 * t = ((o (n - 1)) % (f n - 1)) / (f n - 1): quotient and remainder are integers, no float rounding decides a cell, and the
 * corners of y are the corners of x exactly.  The backward is the adjoint as a gather: one wave per coarse voxel sums its support
 * of at most (2 f)^3 rows of d_y (the same strided slice) in a fixed order; every element of d_x is written.
 * d, h, w in [2, 4096] (an axis of 1 has no align_corners scale: MODET_ERR_DIM), B >= 1, fewer than 2^31 floats in y; f not in {2,4,8},
 * ld not in {3,6,9} or off outside [0, ld - 3]: MODET_ERR_UNSUPPORTED.  Tensors need 4-byte alignment only. */
int modet_pcnet_upsample_fwd(const float* x, float* y, int B, int d, int h, int w, int f, int ld, int off, modet_stream_t stream);
int modet_pcnet_upsample_bwd(const float* d_y, float* d_x, int B, int d, int h, int w, int f, int ld, int off, modet_stream_t stream);

/* DFI'S GATED SUM.  x and logits are (N, 3 n), n in {1, 2, 3} (else MODET_ERR_UNSUPPORTED), out is (N, 3):
 *     out[v,c] = sum over i < n of  x[v, 3 i + c] * sigmoid(logits[v, 3 i + c])
 * The backward writes d_x = d_out * s and d_logits = d_out * x * s (1 - s) in one pass, s recomputed.  Four voxels per thread
 * with 16-byte loads and stores (every tensor 16-byte aligned, else MODET_ERR_UNSUPPORTED), a scalar tail.  N >= 1. */
int modet_pcnet_dfi_gate_fwd(const float* x, const float* logits, float* out, int64_t N, int n, modet_stream_t stream);
int modet_pcnet_dfi_gate_bwd(const float* x, const float* logits, const float* d_out, float* d_x, float* d_logits, int64_t N, int n,
                             modet_stream_t stream);

/* THE NFF TAIL.  t0, t1, t2 are (B,V,C) and logits is (B,V,3); with w = softmax(logits[v]) over its 3 entries the concatenation
 * is cat[v, k C + ch] = t_k[v,ch] * w[k], 3 C channels.  It is never written: every kernel forms it again from the inputs, with
 * the same instructions, so all of them see the same bits.  R = (3 C) / 8 is the gate's hidden width.
 *
 * modet_pcnet_nff_pool: per (sample, channel j of 3 C) the mean over the V voxels (an fp64 sum, divided by V, rounded once), the
 *   maximum and the voxel index of the maximum in the sample -- among equal maxima the lowest index, the rule of ATen's
 *   adaptive_max_pool3d.  Two stages: partial rows per chunk of max(1024, ceil(V / 1024)) voxels (a function of V alone), then a
 *   fixed-order pass over the rows.  avg, mx (B, 3 C) floats, arg (B, 3 C) int32.  ws: pass 0.
 * modet_pcnet_nff_gate_fwd: g = sigmoid(W2 relu(W1 avg) + W2 relu(W1 mx)), W1 (R, 3 C), W2 (3 C, R), no bias; g (B, 3 C).  One
 *   workgroup per sample, fp64 accumulation.
 * modet_pcnet_nff_gate_bwd: d_avg, d_mx (B, 3 C) and, summed over the batch in sample order, d_W1, d_W2 from d_g.  d_W1 and d_W2
 *   may be NULL together (not wanted).  ws: pass 2.
 * modet_pcnet_nff_apply_fwd: out[v,j] = cat[v,j] * g[j], (B,V,3 C).
 * modet_pcnet_nff_apply_bwd_gate: d_g[j] = sum over v of d_out[v,j] * cat[v,j], the same two stages.  ws: pass 1.
 * modet_pcnet_nff_apply_bwd: d_cat[v,j] = d_out[v,j] g[j] + d_avg[j] / V + (v == arg[j] ? d_mx[j] : 0), then d_t_k = d_cat * w[k]
 *   and d_logits by the softmax's backward.  Each of d_t0, d_t1, d_t2 and d_logits may be NULL (not wanted, not written); all
 *   four NULL is MODET_ERR_NULL.
 *
 * LIMITS.  C a multiple of 4 in [4, MODET_PCNET_MAX_C] (else MODET_ERR_UNSUPPORTED), B in [1, 65535], 1 <= V < 2^31 (else
 * MODET_ERR_DIM).  t0, t1, t2, out, d_out and d_t* must be 16-byte aligned (MODET_ERR_UNSUPPORTED), the workspace 8-byte aligned
 * and at least modet_pcnet_nff_ws_bytes(B, V, C, pass) bytes (MODET_ERR_WORKSPACE), which is the exact size a pass needs and 0
 * for arguments that are refused.  All are answered before the first launch. */
size_t modet_pcnet_nff_ws_bytes(int B, int64_t V, int C, int pass);
int modet_pcnet_nff_pool(const float* t0, const float* t1, const float* t2, const float* logits, float* avg, float* mx, int* arg,
                         void* ws, size_t ws_bytes, int B, int64_t V, int C, modet_stream_t stream);
int modet_pcnet_nff_gate_fwd(const float* avg, const float* mx, const float* W1, const float* W2, float* g, int B, int C,
                             modet_stream_t stream);
int modet_pcnet_nff_gate_bwd(const float* avg, const float* mx, const float* W1, const float* W2, const float* g, const float* d_g,
                             float* d_avg, float* d_mx, float* d_W1, float* d_W2, void* ws, size_t ws_bytes, int B, int C,
                             modet_stream_t stream);
int modet_pcnet_nff_apply_fwd(const float* t0, const float* t1, const float* t2, const float* logits, const float* g, float* out,
                              int B, int64_t V, int C, modet_stream_t stream);
int modet_pcnet_nff_apply_bwd_gate(const float* t0, const float* t1, const float* t2, const float* logits, const float* d_out,
                                   float* d_g, void* ws, size_t ws_bytes, int B, int64_t V, int C, modet_stream_t stream);
int modet_pcnet_nff_apply_bwd(const float* t0, const float* t1, const float* t2, const float* logits, const float* d_out,
                              const float* g, const float* d_avg, const float* d_mx, const int* arg, float* d_t0, float* d_t1,
                              float* d_t2, float* d_logits, int B, int64_t V, int C, modet_stream_t stream);

/* s = a + b over n floats (ResBlock's residual); 16-byte loads and stores with a scalar tail of n % 4 floats.  a, b and s 16-byte
 * aligned (MODET_ERR_UNSUPPORTED); s may be a or b.  n >= 1. */
int modet_pcnet_add(const float* a, const float* b, float* s, int64_t n, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
