/* libmodet_hip.so -- the label-overlap (soft Dice) training term: the moving labels warped by the flow against the fixed
 * labels, value and flow gradient, without a one-hot volume; next to the core ABI of modet_hip.h and the other loss families (all
 * stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no memset node, no float atomics -- a call can be captured into a hipGraph and two runs
 * on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_SEGDICE_H
#define MODET_HIP_SEGDICE_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_SEGDICE_MAX_LABELS = 256 };

/* mov_lab, fix_lab (B,1,D,H,W) int16; flow (B,3,D,H,W) planar, or (B,D,H,W,3) when channels_last != 0, component a = displacement
 * along axis a of (z, y, x); nlabels = L in 1..256.  The geometry is modet_warp_fwd's: direct coordinates p = v + flow(v), base
 * corner floor(p), trilinear weights t_c, a corner outside the volume contributes nothing.  Per batch item b and label l in 1..L:
 *     w_l(v) = sum over the 8 corners c of t_c [mov_lab(c) == l]
 *     I_l = sum_v [fix_lab(v) == l] w_l(v)      P_l = sum_v w_l(v)      T_l = sum_v [fix_lab(v) == l]
 *     dsc_l = 2 I_l / (P_l + T_l + 1e-5)        loss = 1 - mean over b and l of dsc_l
 * A label value of 0, below 0 or above L counts in no sum on either side; it is compared against the range and never used as an
 * index.  A label absent on both sides has dsc_l = 0.  On an integer-valued flow I, P and T are the counts [2], [0] and [1] of
 * modet_label_warp_counts for the labels 1..L.
 *
 * table (B,3,L+1) float64 receives [I, P, T] per batch item; column 0 of every row is 0.  The sums are carried in 64-bit fixed
 * point with 32 fraction bits: a corner's fp32 weight is rounded to the nearest multiple of 2^-32 (at most 2^-33 per corner; a
 * weight that is a multiple of 2^-32, every product of fractions on the 1/16 .. 1/1024 grids, is exact), integer additions in any
 * order give the same sum, and B D H W < 2^31 unit weights stay below 2^63.  The conversion to float64 rounds a sum of more than
 * 53 significant bits (a label with more than 2^21 voxels of weight off the 2^-32 .. 2^-11 grid) once.
 *
 * loss[0] is the fp32 rounding of the fp64 expression above over the table.  d_flow, when given, has the layout of flow and
 * receives grad_scale * d loss / d flow:
 *     d loss / d flow_a(v) = sum_c (d t_c / d p_a) g(mov_lab(c), fix_lab(v)),   g(m, f) = -(2 / (B L)) ([m == f] / S_m - I_m / S_m^2)
 * for m in 1..L and 0 otherwise, S_m = P_m + T_m + 1e-5; the two per-label coefficients are rounded to fp32 once, the eight terms
 * summed in fp32 and multiplied by grad_scale at the store.  With add_into != 0 that product is added to what d_flow holds (one
 * fp32 addition per element) instead of replacing it.  There is no gradient for the labels.
 *
 * FLOW VALUES: the rule of modet_hip.h for every warp entry point.  The base corner is bounded while it is a float: a displacement
 * of any magnitude is simply "outside the volume" (no weight in I and P, zero gradient; the voxel's fixed label still counts in
 * T, which does not depend on the flow), and so is a voxel with a NON-FINITE flow component (NaN, +-inf): it adds nothing to I and
 * P, its d_flow is 0 in all three components (add_into: unchanged), and no address outside the tensors is formed.
 *
 * The workspace holds one row of 3 (L+1) 64-bit sums per workgroup of the sums launch (at most 1024 of them) and the 2 (L+1) fp32
 * coefficients per batch item; no volume is staged.  modet_segdice_ws_bytes depends on the shape and L alone and is 0 for what the
 * entry points refuse: a size < 1, B > 65535, L outside 1..256, B D H W >= 2^31.  Those are MODET_ERR_DIM (L: MODET_ERR_UNSUPPORTED); ws
 * must be 8-byte aligned, a misaligned one is MODET_ERR_WORKSPACE like a short one.  Every check happens before the first launch.
 *
 * modet_segdice_sums writes the table alone (two launches); modet_segdice_fwd_bwd the table, the loss and, if d_flow != NULL, the
 * gradient (three or four launches). */
size_t modet_segdice_ws_bytes(int B, int D, int H, int W, int nlabels);
int modet_segdice_sums(const int16_t* mov_lab, const float* flow, const int16_t* fix_lab, double* table, void* ws, size_t ws_bytes,
                       int B, int D, int H, int W, int nlabels, int channels_last, modet_stream_t stream);
int modet_segdice_fwd_bwd(const int16_t* mov_lab, const float* flow, const int16_t* fix_lab, float* loss, double* table,
                          float* d_flow, void* ws, size_t ws_bytes, int B, int D, int H, int W, int nlabels, int channels_last,
                          float grad_scale, int add_into, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
