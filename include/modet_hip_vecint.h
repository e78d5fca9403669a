/* libmodet_hip.so -- integration of a stationary velocity field by scaling and squaring (the reference's VecInt, ModeT/models.py:
 * 70-87, run by its diffeomorphic models at every pyramid level), next to the core ABI of modet_hip.h and the loss families of
 * modet_hip_losses.h, modet_hip_mi.h, modet_hip_ssim.h and modet_hip_reg.h (all five stay frozen).
 *
 * Same conventions: plain C, raw DEVICE pointers, caller-allocated outputs, scratch and workspace, an explicit stream, nothing
 * synchronises, return 0 = ok, < 0 = argument error (the enum of modet_hip.h), > 0 = hipError_t.  Every entry point only
 * enqueues kernels: no host read-back, no memset node, no float atomics -- a call can be captured into a hipGraph and two runs
 * on the same inputs are bit-identical.
 */
#ifndef MODET_HIP_VECINT_H
#define MODET_HIP_VECINT_H

#include "modet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MODET_VECINT_MAX_STEPS = 12 };

/* A FIELD is (B,D,H,W,3) fp32, channels-last, component a = displacement along axis a of (z, y, x), in voxels -- the layout and
 * the meaning of modet_warp_fwd's flow.  With v_0 = 2^-nsteps * vec, step k = 0 .. nsteps-1 is
 *     v_{k+1}[p] = v_k[p] + sample(v_k, p + v_k[p])          trilinear, zeros padding, direct voxel coordinates
 * (modet_warp_fwd with src = flow = v_k and add_flow = 1: the same footprint, clamped loads, value masked afterwards, the same
 * order of the eight corner terms -- the results are equal bit for bit) and out = v_nsteps.  nsteps = 0 copies vec.
 *
 * modet_vecint_fwd: one launch per step; step 0 applies the scale 2^-nsteps while it loads (a power of two: exact).
 *   steps != NULL: (nsteps - 1) fields, steps[k-1] = v_k for k = 1 .. nsteps-1, the inputs the backward needs (v_0 is recomputed
 *                  from vec); scratch is not used and may be NULL.
 *   steps == NULL: inference; the steps alternate between out and scratch (one field; required for nsteps >= 2, else may be NULL).
 *   Both forms run the same kernels on the same values: out is the same bit for bit.
 *   vec, out, steps and scratch must not overlap.
 *
 * modet_vecint_bwd: d_vec = (d out / d vec)^T d_out, one backward step per forward step, last step first.  With g the gradient
 * of v_{k+1} and a_0 = 2^-nsteps, a_k = 1 otherwise, a step writes
 *     d_v[y] = a_k * ( g[y] + sum_c g_c[y] * d sample_c / d x (y + v_k[y]) + sum_x wgt(x -> y) * g[x] )
 * (the identity term, the flow term and the transposed sample).
 *   bound >= 0 is the CALLER'S PROMISE max |vec| <= bound (voxels, every component); 0 = no promise.  Step k then runs on a field of
 *   magnitude <= bound * 2^(k - nsteps) (trilinear sampling with zeros padding is a convex combination of values and zeros, so
 *   max |v_{k+1}| <= 2 max |v_k|).
 *   BOUNDED steps (bound > 0 and bound * 2^(k - nsteps) <= 1): the last sum runs over the 27 neighbours x of y only -- one kernel,
 *     a gather from an LDS tile with a one-voxel halo, no atomics, a fixed order of summation.
 *   GENERAL steps: the last sum is scattered first by the deterministic machinery of the warp backward (modet_warp_bwd_dsrc_tiles
 *     where modet_warp_bwd_dsrc_tiles_ws_bytes reports a workspace, else the 64-bit fixed-point modet_warp_bwd_det; never the
 *     float-atomic kernel) into the workspace, then one kernel adds the three terms.  What those two entry points state about
 *     non-finite d_out (a NaN poisons d_src of every non-empty tile) and about headroom holds here per step.
 *   A BROKEN PROMISE (|vec| > bound somewhere) may give a WRONG GRADIENT: contributions from beyond the 27 neighbours are lost.  It
 *   never gives an out-of-range access: the bounded kernel reads its LDS tile at fixed offsets and global memory at clamped
 *   addresses whatever the values are.
 *   steps: what modet_vecint_fwd wrote (required for nsteps >= 2).  scratch: one field, required for nsteps >= 2 (the gradient
 *   alternates between it and d_vec).  ws: modet_vecint_ws_bytes, 0 where every step is bounded (ws may then be NULL); otherwise
 *   one field for the scattered sum, one more when step 0 is general (v_0 is materialised for the scatter), and the workspace of
 *   the scatter.  ws must be 8-byte aligned.  vec, steps, d_out, d_vec, scratch and ws must not overlap; d_out is only read.
 *
 * NON-FINITE INPUT (vec or d_out holding NaN, +-inf, or magnitudes like 1e30): memory-safe in every entry point -- a coordinate is
 * bounded while it is still a float (clamped to [-2, 1e9] before the conversion to int, as every warp kernel does) and no address
 * outside the tensors is formed.  The VALUES of out and d_vec are then unspecified beyond what modet_warp_fwd, modet_warp_bwd
 * (flow_bound = 1), modet_warp_bwd_dsrc_tiles and modet_warp_bwd_det state for one step.
 *
 * Refused before the first launch: a required pointer that is NULL (MODET_ERR_NULL); B, D, H or W < 1, B > 65535, nsteps outside
 * 0 .. MODET_VECINT_MAX_STEPS, a negative or non-finite bound, B*D*H*W*3 >= 2^31 (MODET_ERR_DIM); a workspace that is too short or
 * misaligned (MODET_ERR_WORKSPACE).  modet_vecint_ws_bytes is 0 for those arguments too. */
int modet_vecint_fwd(const float* vec, float* out, float* steps, float* scratch, int B, int D, int H, int W, int nsteps,
                     modet_stream_t stream);
size_t modet_vecint_ws_bytes(int B, int D, int H, int W, int nsteps, float bound);
int modet_vecint_bwd(const float* vec, const float* steps, const float* d_out, float* d_vec, float* scratch, void* ws,
                     size_t ws_bytes, int B, int D, int H, int W, int nsteps, float bound, modet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
