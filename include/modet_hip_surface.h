/* libmodet_hip.so -- surface distances between two label maps: the Hausdorff distance, its percentile form (HD95) and the average
 * symmetric surface distance per label (the reference's hd_val, hd95_val and assd_val, Baseline methods/RDN/utils.py:94-116, which
 * call medpy's metric.hd / hd95 / assd once per label on the CPU), next to the core ABI of modet_hip.h and the families of
 * modet_hip_losses.h, modet_hip_mi.h, modet_hip_ssim.h, modet_hip_reg.h and modet_hip_vecint.h (all six stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  The entry point only enqueues
 * kernels: no host read-back, no memset node, integer atomics only -- a call can be captured into a hipGraph and two runs on the
 * same inputs are bit-identical.
 */
#ifndef MODET_HIP_SURFACE_H
#define MODET_HIP_SURFACE_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_SURFACE_MAX_DIM = 512, MODET_SURFACE_MAX_LABELS = 32767 };

/* lab_a, lab_b: (D,H,W) int16 label maps of ONE sample (as modet_label_warp_counts takes them), unit voxel spacing.
 * For each label l = 1 .. nlabels (values outside that range, negative ones included, belong to no label):
 *   border_l(X) = the voxels with X == l that have at least one of their 6 face neighbours != l or outside the volume
 *                 (mask ^ binary_erosion(mask, connectivity 1, border_value 0): a mask that touches the volume's face has border
 *                 voxels there);
 *   sd(A->B)    = for every voxel of border_l(A) the Euclidean distance to the nearest voxel of border_l(B); sd(B->A) likewise.
 *                 Every squared distance is an integer, and the integers are what the kernels compute and keep.
 *   metrics[l-1] = { hd     = max(max sd(A->B), max sd(B->A)),
 *                    hdq    = numpy.percentile(hstack(sd(A->B), sd(B->A)), percentile), the default linear method: virtual index
 *                             (n - 1) * (percentile / 100) in fp64, the order statistics at its floor and the next, the weight its
 *                             fractional part,
 *                    assd   = (asd_ab + asd_ba) / 2,
 *                    asd_ab = mean sd(A->B),  asd_ba = mean sd(B->A) }            (fp64; sums in a fixed order)
 *   counts[l-1]  = { n_a, n_b (voxels of l), nborder_a, nborder_b, hd2, q_lo2, q_hi2 }: the last three are the integer SQUARES of
 *                  hd and of the two order statistics hdq interpolates between.
 * A label that is EMPTY in either map: its five metrics are NaN, hd2 = q_lo2 = q_hi2 = -1, and the four counts say which side is
 * empty.  That is no error.
 *
 * ws: modet_surface_ws_bytes(D, H, W, nlabels) bytes, 16-byte aligned: 12 bytes per voxel (two int16 border-label volumes, one
 * int32 distance volume per direction; the labels are processed in sequence over them), two histograms of
 * (D-1)^2 + (H-1)^2 + (W-1)^2 + 1 bins and 48 bytes per label.  lab_a, lab_b, metrics, counts and ws must not overlap; the maps are
 * only read.
 *
 * Refused before the first launch: a NULL pointer (MODET_ERR_NULL); D, H or W outside 1 .. MODET_SURFACE_MAX_DIM, nlabels outside
 * 1 .. MODET_SURFACE_MAX_LABELS, a percentile outside [0, 100] or NaN (MODET_ERR_DIM); a workspace that is too short or
 * misaligned (MODET_ERR_WORKSPACE).  modet_surface_ws_bytes is 0 for dimensions and label counts out of range. */
size_t modet_surface_ws_bytes(int D, int H, int W, int nlabels);
int modet_surface_distances(const int16_t* lab_a, const int16_t* lab_b, double* metrics, int64_t* counts, void* ws, size_t ws_bytes,
                            int D, int H, int W, int nlabels, float percentile, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
