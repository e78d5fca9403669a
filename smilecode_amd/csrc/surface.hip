// Surface distances between two label maps (HD, HD-percentile, ASSD: medpy's metric.hd / hd95 / assd at unit spacing and
// connectivity 1, which the reference's Baseline methods/RDN/utils.py:94-116 calls once per label on the CPU):
// include/modet_hip_surface.h.
//   1. classify: one pass over both maps -- voxel and border counts per label, the bounding box of each label's border voxels
//      (of both maps together), and one int16 "border label" volume per map (l at a border voxel of label l, else 0).
//   2. per label, both directions at once (blockIdx.y): the exact squared Euclidean distance transform of the other map's border
//      set inside the bounding box, three separable passes in int32.  A pass keeps 16 lines in LDS and takes, per output position,
//      the minimum over the line of f(p') + (p - p')^2: O(n^2) per line, branch-free, no lower-envelope logic.  The last pass does
//      not store: it adds the distance at each border voxel of the source map to an integer histogram.
//   3. per label, one workgroup reduces the two histograms: the maximum, the two order statistics of the percentile from a
//      cumulative count, each direction's mean as a fixed-order fp64 sum -- and clears the bins it read for the next label.
// Integer atomics only (counts, minima, maxima): two runs on the same inputs give the same bits.  Nothing synchronises, nothing is
// read back: the bounding boxes and counts stay in device memory and every kernel exits early from them.
#include <math.h>

#include "common.h"
#include "../../include/modet_hip_surface.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;
constexpr int SD_INF = 1 << 29;            // "no border voxel on this line": SD_INF + 511^2 < 2^31
constexpr int NS = 12;                     // ints per label in the statistics table
enum { S_NA = 0, S_NB, S_BA, S_BB, S_MIN /* z y x */, S_MAX = 7 /* z y x */, S_MAXD2 = 10 };
constexpr int LCAP = 1024;                 // labels 1 .. LCAP are counted in LDS first, the others straight in global memory
constexpr int LANES = 16, LSTR = LANES + 1, MAXN = MODET_SURFACE_MAX_DIM;

__global__ __launch_bounds__(BLK) void surface_init_kernel(int* __restrict__ st, int n_entries) {
  for (int i = blockIdx.x * BLK + threadIdx.x; i < n_entries; i += gridDim.x * BLK) {
    const int k = i % NS;
    st[i] = (k >= S_MIN && k < S_MAX) ? 0x7fffffff : ((k >= S_MAX && k < S_MAXD2) ? -1 : 0);
  }
}

// values only fall (rise): a stale read can cost an atomic that changes nothing, never skip one that would
__device__ __forceinline__ void atomic_lower(int* p, int v) { if (v < *(volatile int*)p) atomicMin(p, v); }
__device__ __forceinline__ void atomic_raise(int* p, int v) { if (v > *(volatile int*)p) atomicMax(p, v); }

__device__ __forceinline__ bool is_border(const int16_t* __restrict__ lab, int idx, int v, int z, int y, int x, int D, int H,
                                          int W) {
  const int HW = H * W;
  bool b = z == 0 || y == 0 || x == 0 || z == D - 1 || y == H - 1 || x == W - 1;
  // clamped addresses, always inside the map; at the volume's face the voxel is a border voxel whatever the load returns
  b |= lab[z > 0 ? idx - HW : idx] != v;
  b |= lab[z < D - 1 ? idx + HW : idx] != v;
  b |= lab[y > 0 ? idx - W : idx] != v;
  b |= lab[y < H - 1 ? idx + W : idx] != v;
  b |= lab[x > 0 ? idx - 1 : idx] != v;
  b |= lab[x < W - 1 ? idx + 1 : idx] != v;
  return b;
}

__global__ __launch_bounds__(BLK) void surface_classify_kernel(const int16_t* __restrict__ la, const int16_t* __restrict__ lb,
                                                               int16_t* __restrict__ ba, int16_t* __restrict__ bb,
                                                               int* __restrict__ st, int D, int H, int W, int nlabels) {
  __shared__ int sm[LCAP * 10];
  const int ncap = nlabels < LCAP ? nlabels : LCAP;
  for (int i = threadIdx.x; i < ncap * 10; i += BLK) {
    const int k = i % 10;
    sm[i] = (k >= S_MIN && k < S_MAX) ? 0x7fffffff : (k >= S_MAX ? -1 : 0);
  }
  __syncthreads();
  const int V = D * H * W;
  for (int idx = blockIdx.x * BLK + threadIdx.x; idx < V; idx += gridDim.x * BLK) {
    const int x = idx % W, t = idx / W, y = t % H, z = t / H;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int16_t* lab = m ? lb : la;
      const int v = lab[idx];
      int16_t out = 0;
      if (v >= 1 && v <= nlabels) {
        int* row = v <= LCAP ? sm + (v - 1) * 10 : st + (size_t)v * NS;
        atomicAdd(row + S_NA + m, 1);
        if (is_border(lab, idx, v, z, y, x, D, H, W)) {
          out = (int16_t)v;
          atomicAdd(row + S_BA + m, 1);
          atomic_lower(row + S_MIN, z); atomic_lower(row + S_MIN + 1, y); atomic_lower(row + S_MIN + 2, x);
          atomic_raise(row + S_MAX, z); atomic_raise(row + S_MAX + 1, y); atomic_raise(row + S_MAX + 2, x);
        }
      }
      (m ? bb : ba)[idx] = out;
    }
  }
  __syncthreads();
  for (int l = threadIdx.x; l < ncap; l += BLK) {
    const int* row = sm + l * 10;
    int* g = st + (size_t)(l + 1) * NS;
    if (row[S_NA]) atomicAdd(g + S_NA, row[S_NA]);
    if (row[S_NB]) atomicAdd(g + S_NB, row[S_NB]);
    if (row[S_BA]) atomicAdd(g + S_BA, row[S_BA]);
    if (row[S_BB]) atomicAdd(g + S_BB, row[S_BB]);
    if (row[S_BA] | row[S_BB]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { atomic_lower(g + S_MIN + k, row[S_MIN + k]); atomic_raise(g + S_MAX + k, row[S_MAX + k]); }
    }
  }
}

// One pass of the squared distance transform along AXIS (0 = z, 1 = y, 2 = x) inside label l's bounding box, for direction
// blockIdx.y (0: distances to the border of B, gathered at the border of A; 1: the other way round).
//   AXIS 2 reads the target's border labels (0 at a border voxel of l, SD_INF elsewhere) and writes g;
//   AXIS 1 runs on g in place (a tile is read whole before it is written; tiles are disjoint);
//   AXIS 0 reads g and adds the result at the source's border voxels to hist, and the largest of them to the table.
// A tile is 16 lines: consecutive x for AXIS 0 and 1, consecutive y for AXIS 2.  Every g element of the box is written by the
// AXIS 2 pass before a later pass reads it, and nothing outside the box is read.
template <int AXIS>
__global__ __launch_bounds__(BLK) void surface_edt_kernel(const int16_t* __restrict__ ba, const int16_t* __restrict__ bb,
                                                          int* __restrict__ g0, size_t g_stride, unsigned* __restrict__ hist0,
                                                          int nbins, int* __restrict__ st, int label, int D, int H, int W) {
  __shared__ int line[MAXN * LSTR];
  __shared__ int blockmax;
  int* row = st + (size_t)label * NS;
  if (row[S_NA] == 0 || row[S_NB] == 0) return;                 // a side is empty: nothing to measure (uniform over the grid)
  const int dir = blockIdx.y;
  const int16_t* target = dir ? ba : bb;
  const int16_t* source = dir ? bb : ba;
  int* g = g0 + (size_t)dir * g_stride;
  unsigned* hist = hist0 + (size_t)dir * nbins;
  const int lo[3] = {row[S_MIN], row[S_MIN + 1], row[S_MIN + 2]}, hi[3] = {row[S_MAX], row[S_MAX + 1], row[S_MAX + 2]};
  // (both sides non-empty, so both have border voxels and the box is a real one inside the volume; the clamps below only keep
  // a damaged table from forming an address outside the buffers)
  const int dims[3] = {D, H, W};
  int l0[3], ext[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    l0[a] = min(max(lo[a], 0), dims[a] - 1);
    ext[a] = min(max(hi[a], l0[a]), dims[a] - 1) - l0[a] + 1;
  }
  constexpr int LANE = AXIS == 2 ? 1 : 2, REST = AXIS == 0 ? 1 : 0;
  const int stride[3] = {H * W, W, 1};
  const int n = ext[AXIS];
  const int lane_tiles = (ext[LANE] + LANES - 1) / LANES, tiles = lane_tiles * ext[REST];
  if (AXIS == 0) {
    if (threadIdx.x == 0) blockmax = -1;
    __syncthreads();
  }
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int lane0 = (tile % lane_tiles) * LANES, nl = min(LANES, ext[LANE] - lane0);
    const int base = (l0[REST] + tile / lane_tiles) * stride[REST] + (l0[LANE] + lane0) * stride[LANE] + l0[AXIS] * stride[AXIS];
    const int work = n * LANES;
    for (int i = threadIdx.x; i < work; i += BLK) {
      const int ln = AXIS == 2 ? i / n : i % LANES, p = AXIS == 2 ? i % n : i / LANES;
      int v = SD_INF;
      if (ln < nl) {
        const int at = base + ln * stride[LANE] + p * stride[AXIS];
        v = AXIS == 2 ? (target[at] == label ? 0 : SD_INF) : g[at];
      }
      line[p * LSTR + ln] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < work; i += BLK) {
      const int ln = AXIS == 2 ? i / n : i % LANES, p = AXIS == 2 ? i % n : i / LANES;
      if (ln >= nl) continue;
      int m = SD_INF;
      for (int q = 0; q < n; ++q) m = min(m, line[q * LSTR + ln] + (p - q) * (p - q));
      const int at = base + ln * stride[LANE] + p * stride[AXIS];
      if (AXIS != 0) {
        g[at] = m;
      } else if (source[at] == label && m < nbins) {
        atomicAdd(hist + m, 1u);
        atomic_raise(&blockmax, m);
      }
    }
    __syncthreads();
  }
  if (AXIS == 0 && threadIdx.x == 0 && blockmax >= 0) atomic_raise(row + S_MAXD2, blockmax);
}

// numpy's _lerp: a + (b - a) * t, taken from the other end where t >= 0.5
__device__ __forceinline__ double np_lerp(double a, double b, double t) {
  const double d = b - a;
  return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// label l: metrics[l-1] = hd, hdq, assd, asd_ab, asd_ba; counts[l-1] = n_a, n_b, nborder_a, nborder_b, hd2, q_lo2, q_hi2.
// One workgroup.  Bins 0 .. hd2 of both histograms are read, then cleared.
__global__ __launch_bounds__(BLK) void surface_reduce_kernel(unsigned* __restrict__ hist0, int nbins, const int* __restrict__ st,
                                                             int label, double q, double* __restrict__ metrics,
                                                             long long* __restrict__ counts) {
  __shared__ double sm[BLK];
  __shared__ long long cum[BLK];
  __shared__ int found[2];
  const int* row = st + (size_t)label * NS;
  double* mo = metrics + (size_t)(label - 1) * 5;
  long long* co = counts + (size_t)(label - 1) * 7;
  const int na = row[S_NA], nb = row[S_NB], sa = row[S_BA], sb = row[S_BB];
  if (na == 0 || nb == 0) {
    if (threadIdx.x == 0) {
      co[0] = na; co[1] = nb; co[2] = sa; co[3] = sb; co[4] = -1; co[5] = -1; co[6] = -1;
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
      for (int k = 0; k < 5; ++k) mo[k] = nan;
    }
    return;
  }
  unsigned* ha = hist0;
  unsigned* hb = hist0 + nbins;
  const int top = min(max(row[S_MAXD2], 0), nbins - 1), nb_used = top + 1;
  // each direction's sum of distances: thread t takes bins t, t + 256, ... in order, then the threads are added in order
  double s_ab = 0.0, s_ba = 0.0;
  for (int b = threadIdx.x; b < nb_used; b += BLK) {
    const unsigned ca = ha[b], cb = hb[b];
    if (ca | cb) {
      const double r = sqrt((double)b);
      s_ab += (double)ca * r;
      s_ba += (double)cb * r;
    }
  }
  sm[threadIdx.x] = s_ab;
  __syncthreads();
  double t_ab = 0.0, t_ba = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < BLK; ++i) t_ab += sm[i];
  __syncthreads();
  sm[threadIdx.x] = s_ba;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 0; i < BLK; ++i) t_ba += sm[i];
  // the two order statistics: the combined histogram in 256 contiguous chunks, counted, then the chunk that holds a rank is walked
  const long long n = (long long)sa + sb;
  const double vi = (double)(n - 1) * (q / 100.0);               // numpy: (n - 1) * true_divide(q, 100)
  long long k_lo = (long long)floor(vi);
  double gamma = vi - floor(vi);
  if (k_lo >= n - 1) { k_lo = n - 1; gamma = 0.0; }               // numpy clips both neighbours to the last element
  if (k_lo < 0) k_lo = 0;
  const long long k_hi = k_lo + 1 < n ? k_lo + 1 : n - 1;
  const int chunk = (nb_used + BLK - 1) / BLK, b0 = min((int)threadIdx.x * chunk, nb_used), b1 = min(b0 + chunk, nb_used);
  long long mine = 0;
  for (int b = b0; b < b1; ++b) mine += (long long)ha[b] + hb[b];
  cum[threadIdx.x] = mine;
  if (threadIdx.x < 2) found[threadIdx.x] = top;                  // (a rank beyond the counted total cannot occur: n = sa + sb)
  __syncthreads();
  long long before = 0;
  for (int i = 0; i < (int)threadIdx.x; ++i) before += cum[i];
  if (mine > 0) {
    const bool has_lo = k_lo >= before && k_lo < before + mine, has_hi = k_hi >= before && k_hi < before + mine;
    if (has_lo || has_hi) {
      long long c = before;
      for (int b = b0; b < b1; ++b) {
        const long long c1 = c + (long long)ha[b] + hb[b];
        if (has_lo && k_lo >= c && k_lo < c1) found[0] = b;
        if (has_hi && k_hi >= c && k_hi < c1) found[1] = b;
        c = c1;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int lo2 = found[0], hi2 = found[1];
    const double asd_ab = t_ab / (double)sa, asd_ba = t_ba / (double)sb;
    mo[0] = sqrt((double)top);
    mo[1] = np_lerp(sqrt((double)lo2), sqrt((double)hi2), gamma);
    mo[2] = (asd_ab + asd_ba) / 2.0;
    mo[3] = asd_ab;
    mo[4] = asd_ba;
    co[0] = na; co[1] = nb; co[2] = sa; co[3] = sb; co[4] = top; co[5] = lo2; co[6] = hi2;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb_used; b += BLK) { ha[b] = 0u; hb[b] = 0u; }
}

// ------------------------------------------------------------------------------------------------ host
inline bool args_ok(int D, int H, int W, int nlabels) {
  return D >= 1 && H >= 1 && W >= 1 && D <= MAXN && H <= MAXN && W <= MAXN && nlabels >= 1 && nlabels <= MODET_SURFACE_MAX_LABELS;
}
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
struct Ws { size_t hist_off, g_off, g_stride, ba_off, bb_off, bytes; int nbins; };
inline Ws layout(int D, int H, int W, int nlabels) {
  Ws w{};
  const size_t V = (size_t)D * H * W;
  w.nbins = (D - 1) * (D - 1) + (H - 1) * (H - 1) + (W - 1) * (W - 1) + 1;
  w.hist_off = up256((size_t)(nlabels + 1) * NS * sizeof(int));                 // [table][2 histograms][2 x g][ba][bb]
  w.g_off = w.hist_off + up256((size_t)2 * w.nbins * sizeof(unsigned));
  w.g_stride = up256(V * sizeof(int)) / sizeof(int);
  w.ba_off = w.g_off + 2 * w.g_stride * sizeof(int);
  w.bb_off = w.ba_off + up256(V * sizeof(int16_t));
  w.bytes = w.bb_off + up256(V * sizeof(int16_t));
  return w;
}
inline int tile_grid(int n_lane, int n_rest) {
  const int64_t t = (int64_t)cdiv(n_lane, LANES) * n_rest;
  return (int)(t < 1024 ? t : 1024);
}

}  // namespace

extern "C" {

size_t modet_surface_ws_bytes(int D, int H, int W, int nlabels) {
  return args_ok(D, H, W, nlabels) ? layout(D, H, W, nlabels).bytes : 0;
}

int modet_surface_distances(const int16_t* lab_a, const int16_t* lab_b, double* metrics, int64_t* counts, void* ws,
                            size_t ws_bytes, int D, int H, int W, int nlabels, float percentile, modet_stream_t stream) {
  MODET_CHECK_PTR(lab_a); MODET_CHECK_PTR(lab_b); MODET_CHECK_PTR(metrics); MODET_CHECK_PTR(counts); MODET_CHECK_PTR(ws);
  MODET_CHECK_DIM(args_ok(D, H, W, nlabels) && percentile >= 0.f && percentile <= 100.f);      // (NaN fails both)
  const Ws w = layout(D, H, W, nlabels);
  if (ws_bytes < w.bytes || ((uintptr_t)ws & 15) != 0) return MODET_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  int* st = (int*)base;
  unsigned* hist = (unsigned*)(base + w.hist_off);
  int* g = (int*)(base + w.g_off);
  int16_t* ba = (int16_t*)(base + w.ba_off);
  int16_t* bb = (int16_t*)(base + w.bb_off);
  const int n_entries = (nlabels + 1) * NS;
  hipLaunchKernelGGL(surface_init_kernel, dim3(flat_grid(n_entries, BLK)), dim3(BLK), 0, s, st, n_entries);
  modet_zero_async(hist, (size_t)2 * w.nbins * sizeof(unsigned), s);
  hipLaunchKernelGGL(surface_classify_kernel, dim3(flat_grid((int64_t)D * H * W, BLK)), dim3(BLK), 0, s, lab_a, lab_b, ba, bb, st,
                     D, H, W, nlabels);
  const dim3 gx(tile_grid(H, D), 2), gy(tile_grid(W, D), 2), gz(tile_grid(W, H), 2);
  for (int l = 1; l <= nlabels; ++l) {
    hipLaunchKernelGGL(surface_edt_kernel<2>, gx, dim3(BLK), 0, s, (const int16_t*)ba, (const int16_t*)bb, g, w.g_stride, hist,
                       w.nbins, st, l, D, H, W);
    hipLaunchKernelGGL(surface_edt_kernel<1>, gy, dim3(BLK), 0, s, (const int16_t*)ba, (const int16_t*)bb, g, w.g_stride, hist,
                       w.nbins, st, l, D, H, W);
    hipLaunchKernelGGL(surface_edt_kernel<0>, gz, dim3(BLK), 0, s, (const int16_t*)ba, (const int16_t*)bb, g, w.g_stride, hist,
                       w.nbins, st, l, D, H, W);
    hipLaunchKernelGGL(surface_reduce_kernel, dim3(1), dim3(BLK), 0, s, hist, w.nbins, (const int*)st, l, (double)percentile,
                       metrics, (long long*)counts);
  }
  return modet_launch_status();
}

}  // extern "C"
