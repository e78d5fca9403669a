// The interface between the five conv translation units (conv3d*.hip): every modetx_* function declared ONCE, default
// arguments included (C++ linkage, not part of the ABI).  All five include it -- the defining file too, so a definition that
// drifts from its declaration fails to compile instead of linking by luck.
#pragma once
#include "common.h"
#include "step_ctx.h"

// ---- the kernel families (the values: include/modet_hip.h, modet_conv3d_kernel_family_v / modet_conv3d_bf16_kernel_family) and
// the ONE switch between the z-march and the other families, shared by the fp32 routes (conv3d.hip: route_conv, route_wgrad) and
// the bf16-storage routes (conv3d_bf16.hip: route_conv16, route_wgrad16, which only know SPLIT = tiled and X3)
enum ConvFamily { FAM_EXACT = 0, FAM_SPLIT = 1, FAM_X3 = 2, FAM_DIRECT = 3, FAM_WTR = 4, FAM_Q = 5 };
// MODET_CONV_X3 = 0 (tuning builds only) keeps the z-march kernels out of every route (A/B measurements)
inline bool conv_x3_on() { static const bool on = modet_tuning_env("MODET_CONV_X3") != '0'; return on; }

// ---- conv3d_bf16.hip: tiled bf16x3 on fp32 tensors ("split": six exact bf16 piece products per multiply, error <= 3 * 2^-24 |a b|),
// the reductions of the 16-bit weight-gradient partials, the 16-bit side of modet_conv3d_prepack_* / _wgrad_defer_flush
bool modetx_split_eligible(int Cin, int Cout);
size_t modetx_split_ws_bytes(int Cin, int Cout);
size_t modetx_split_stats_bytes(int B, int D, int H, int W, int Cin, int Cout);
int modetx_split_conv(modet_step_ctx* step, const float* x, const float* w, const float* bias, float* y, void* ws, float* stats,
                      int B, int D, int H, int W, int Cin, int Cout, int mode, hipStream_t s);
int modetx_wgrad_partials_reduce(modet_step_ctx* defer, const float* part, float* red, float* dw, float* db, int gx, int Cin,
                                 int Cout, int cib, int u, int layout, hipStream_t s);
int modetx_wgrad_partials_reduce2(modet_step_ctx* defer, const float* part, float* red, float* dw, float* db, int gx, int gy,
                                  int Cin, int Cout, int nq, int mt, int nt, int n_coblk, hipStream_t s);
size_t modetx_bf16_prepack_bytes(modet_step_ctx* c);
void modetx_bf16_prepack_begin(modet_step_ctx* c, void* arena, hipStream_t stream);
void modetx_bf16_defer_flush(modet_step_ctx* c, hipStream_t stream);

// ---- conv3d_x3.hip: bf16x3 z-marching kernels of the few-channel full-resolution layers
bool modetx_x3_eligible(int B, int D, int H, int W, int Cin, int Cout);
size_t modetx_x3_ws_bytes(int Cin, int Cout);
size_t modetx_x3_stats_bytes(int B, int D, int H, int W, int Cin, int Cout);
int modetx_x3_conv(modet_step_ctx* step, const float* x, const float* w, const float* bias, float* y, void* ws, float* stats,
                   const float* in_mean, const float* in_rstd, int B, int D, int H, int W, int Cin, int Cout, int act, int mode,
                   hipStream_t s, const float* amax = nullptr, bool x_free = false);
size_t modetx_x3_bst_rows_bytes(int B, int D, int H, int W, int Cin, int Cout);
int modetx_x3_dgrad_bst(modet_step_ctx* step, const float* dy, const float* w, float* dx, const float* xraw, const float* mean,
                        const float* rstd, float* rows, void* ws, int B, int D, int H, int W, int Cin, int Cout, hipStream_t s,
                        const float* amax = nullptr);
bool modetx_x3_wgrad_eligible(int B, int D, int H, int W, int Cin, int Cout);
size_t modetx_x3_wgrad_ws_bytes(int B, int D, int H, int W, int Cin, int Cout);
int modetx_x3_wgrad(modet_step_ctx* defer, const float* x, const float* dy, float* dw, float* db, void* ws, int B, int D, int H,
                    int W, int Cin, int Cout, hipStream_t s, const float* amax = nullptr, const float* in_mean = nullptr,
                    const float* in_rstd = nullptr);
// its bf16-storage forms (launched by conv3d_bf16.hip's modet_conv3d_bf16_* entry points; the two *_eligible predicates are for
// route_conv16 / route_wgrad16 there and nobody else)
bool modetx_x3_bf16_eligible(int B, int D, int H, int W, int Cin, int Cout, int x_bf16);
int modetx_x3_bf16_rows_per_sample(int B, int D, int H, int W, int Cin, int Cout);
int modetx_x3_bf16_conv(modet_step_ctx* step, const void* x, int x_bf16, const float* w, const float* bias, void* y, int y_bf16,
                        void* ws, float* stats, int B, int D, int H, int W, int Cin, int Cout, int mode, hipStream_t s);
bool modetx_x3_bf16_wgrad_eligible(int B, int D, int H, int W, int Cin, int Cout);
size_t modetx_x3_bf16_wgrad_ws_bytes(int B, int D, int H, int W, int Cin, int Cout);
int modetx_x3_bf16_wgrad(modet_step_ctx* defer, const void* x, int x_bf16, const void* dy, float* dw, float* db, void* ws, int B,
                         int D, int H, int W, int Cin, int Cout, hipStream_t s);
void modetx_x3_prepack_begin(modet_step_ctx* c, hipStream_t stream);      // the recorded 16-bit packing jobs with layout 2 / 3

// ---- conv3d_q.hip: bf16x3 forward / data gradient with the K index packed in channel quads
bool modetx_q_eligible(int B, int D, int H, int W, int Cin, int Cout);
size_t modetx_q_ws_bytes(int Cin, int Cout);
size_t modetx_q_stats_bytes(int B, int D, int H, int W, int Cin, int Cout);
int modetx_q_conv(modet_step_ctx* step, const float* x, const float* w, const float* bias, float* y, void* ws, float* stats,
                  const float* in_mean, const float* in_rstd, int B, int D, int H, int W, int Cin, int Cout, int mode,
                  hipStream_t s, const float* amax = nullptr, const float* xraw = nullptr, const float* bmean = nullptr,
                  const float* brstd = nullptr, float* bst_rows = nullptr, bool x_free = false);
size_t modetx_q_bst_rows_bytes(int B, int D, int H, int W, int Cin, int Cout);
void modetx_q_prepack_begin(modet_step_ctx* c, hipStream_t stream);       // the recorded packing jobs with layout 4

// ---- conv3d_wtr.hip: bf16x3 weight gradient through LDS transpose reads
bool modetx_wtr_eligible(int B, int D, int H, int W, int Cin, int Cout);
size_t modetx_wtr_ws_bytes(int B, int D, int H, int W, int Cin, int Cout);
bool modetx_wtr_batches(int B, int D, int H, int W);
void modetx_wtr_flush(modet_step_ctx* c, hipStream_t s);
int modetx_wtr_wgrad(modet_step_ctx* defer, const float* x, const float* dy, float* dw, float* db, void* ws, int B, int D, int H,
                     int W, int Cin, int Cout, hipStream_t s, const float* amax = nullptr);
