// Exact k nearest neighbours of a cloud on the GPU (rs_cloud_knn) and two consumers that keep
// the index lists on the device: the plane fit over a point's own k nearest
// (rs_cloud_knn_normals) and the mean distance to them (rs_cloud_knn_mean_dist).  The definitions
// stand in include/rsamd.h; tests/knn_ref.py restates them in numpy.  All fp64, plain HIP.
//
//   k_knn_box*      the box [lo, hi] of the points whose three coordinates are finite and their
//                   number: per-block partials, then one workgroup over the partials
//   k_knn_count     one lane per point: its cell (eval.hip's coordinate, clamped to the grid),
//                   cnt[cell] += 1 (integer atomicAdd); a non-finite point gets its outputs here
//                   and takes no further part
//   k_knn_scan*     exclusive scan of the cell counts, the three-kernel scheme of cloud.hip and
//                   eval.hip, copied once more; the first kernel also takes the largest count
//   k_knn_scatter   one lane per point: the coordinates, 24 contiguous bytes, and the index into
//                   the cell's segment through an integer cursor, in arrival order
//   k_knn_query     one lane per query, one wave per workgroup, eval.hip's walk over Chebyshev
//                   rings.  The lane's sorted list of k pairs is a column of LDS: slot s of lane l
//                   stands at s * 64 + l, so only that lane touches it (no barrier) and a wave's
//                   lanes hit distinct banks whatever slot each is at.  The current worst key
//                   lives in registers; most candidates are rejected there without an LDS access,
//                   an accepted one is inserted from the tail
//   k_knn_normals, k_knn_mean   one lane per point over its own row of the lists
//   (rs_cloud_fpfh keeps the lists in the same way; its two kernels stand in global_reg.hip)
// The list is the k smallest of the pairs (d2 bits, index), a set that does not depend on the
// order of the visits: neither the arrival order inside a cell, nor the cells' layout, nor `cell`
// can change a bit of the result, and no per-cell sort is needed.
// Every global index is bounded: a cell index is clamped to the grid where a point computes it
// and walked inside the grid where a query does; the scatter writes, and the query reads, only
// below the number of finite points; a list slot is below k, the LDS the launch asks for.  Every
// loop is bounded by the grid's dimensions, a segment's length or k; no lane waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_math.h"
#include "host.h"

namespace rsd {

constexpr int kKnnThreads = 256;
constexpr int kKnnBoxBlocks = 256;
constexpr int kKnnWave = 64;
constexpr int kKnnScanThreads = 1024;
constexpr int kKnnScanItems = 4;
constexpr int kKnnScanChunk = kKnnScanThreads * kKnnScanItems;
constexpr double kKnnShrink = 1.0 - 1.0 / 1048576.0;
constexpr double kKnnFar = 536870912.0;   // 2^29: a query's cell coordinate is clamped to +-this
constexpr int kKnnNone = 0x7fffffff;

// stats words (unsigned long long each)
constexpr int kKnnTested = 0, kKnnLargest = 1;

struct KnnGrid {
  double lo[3], cell;
  int dim[3];
};

__device__ __forceinline__ double knn_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ bool knn_finite3(const double *p) {
  return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// floor((x - lo) / cell) clamped to [-limit, limit]; a NaN gives -limit
__device__ __forceinline__ double knn_coord(double x, double lo, double cell, double limit) {
#pragma clang fp contract(off)
  const double q = floor((x - lo) / cell);
  return !(q >= -limit) ? -limit : (q > limit ? limit : q);
}

// the cell of a finite point: every coordinate clamped to the grid
__device__ __forceinline__ int64_t knn_cell(const KnnGrid &G, const double *p) {
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double q = knn_coord(p[a], G.lo[a], G.cell, static_cast<double>(G.dim[a] - 1));
    c[a] = q < 0.0 ? 0 : static_cast<int>(q);
  }
  return (static_cast<int64_t>(c[2]) * G.dim[1] + c[1]) * G.dim[0] + c[0];
}

// Seven doubles per workgroup: the minimum and the maximum per axis over the points whose three
// coordinates are finite (+inf / -inf where it saw none) and their number.
__global__ __launch_bounds__(kKnnThreads) void k_knn_box(const double *pts, int64_t n,
                                                         double *part) {
  __shared__ double lds[7][kKnnThreads / 64];
  double v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kKnnThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kKnnThreads) {
    const double *p = pts + 3 * i;
    if (knn_finite3(p)) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        v[a] = fmin(v[a], p[a]);
        v[3 + a] = fmax(v[3 + a], p[a]);
      }
      v[6] += 1.0;
    }
  }
#pragma unroll
  for (int a = 0; a < 7; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(v[a], off);
      v[a] = a < 3 ? fmin(v[a], o) : (a < 6 ? fmax(v[a], o) : v[a] + o);
    }
    if ((threadIdx.x & 63) == 0) lds[a][threadIdx.x >> 6] = v[a];
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    const int a = threadIdx.x;
    double r = lds[a][0];
    for (int w = 1; w < kKnnThreads / 64; ++w)
      r = a < 3 ? fmin(r, lds[a][w]) : (a < 6 ? fmax(r, lds[a][w]) : r + lds[a][w]);
    part[7 * static_cast<int64_t>(blockIdx.x) + a] = r;
  }
}

// One wave folds the nb partials (counts are whole numbers below 2^28: their sum is exact).
__global__ __launch_bounds__(kKnnWave) void k_knn_box_fold(const double *part, int nb,
                                                          double *box) {
  double v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0};
  for (int b = threadIdx.x; b < nb; b += kKnnWave) {
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      const double o = part[7 * b + a];
      v[a] = a < 3 ? fmin(v[a], o) : (a < 6 ? fmax(v[a], o) : v[a] + o);
    }
  }
#pragma unroll
  for (int a = 0; a < 7; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(v[a], off);
      v[a] = a < 3 ? fmin(v[a], o) : (a < 6 ? fmax(v[a], o) : v[a] + o);
    }
    if (threadIdx.x == 0) box[a] = v[a];
  }
}

// One lane per point.  cell_of[i] = -1 for a non-finite point; in a self query (`rows` = the
// lists' width, else 0) such a point is a query as well and gets its empty row here.
__global__ __launch_bounds__(kKnnThreads) void k_knn_count(const double *pts, int64_t n,
                                                           KnnGrid G, int32_t *cell_of,
                                                           int32_t *cnt, int rows, int32_t *idx,
                                                           double *d2, int32_t *count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kKnnThreads + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  if (!knn_finite3(p)) {
    cell_of[i] = -1;
    if (rows > 0) {
      count[i] = 0;
      for (int s = 0; s < rows; ++s) {
        idx[i * rows + s] = -1;
        if (d2) d2[i * rows + s] = INFINITY;
      }
    }
    return;
  }
  const int64_t cell = knn_cell(G, p);
  cell_of[i] = static_cast<int32_t>(cell);
  atomicAdd(&cnt[cell], 1);
}

// Exclusive scan in place of the chunk v[at .. at + kKnnScanChunk), clipped to `end`, started at
// `carry`; returns the chunk's sum and leaves the largest element in *largest.  All threads of
// the workgroup call it together.
__device__ __forceinline__ int knn_scan_chunk(int32_t *v, int64_t at, int64_t end, int carry,
                                              int *lds, int *largest) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = at + static_cast<int64_t>(threadIdx.x) * kKnnScanItems;
  int x[kKnnScanItems], sum = 0, big = 0;
#pragma unroll
  for (int k = 0; k < kKnnScanItems; ++k) {
    x[k] = base + k < end ? v[base + k] : 0;
    sum += x[k];
    big = max(big, x[k]);
  }
  int incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  for (int off = 32; off > 0; off >>= 1) big = max(big, __shfl_xor(big, off));
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kKnnScanThreads / 64; ++w) {
    if (w < wave) before += lds[w];
    all += lds[w];
  }
  int run = carry + before + incl - sum;
#pragma unroll
  for (int k = 0; k < kKnnScanItems; ++k) {
    if (base + k < end) v[base + k] = run;
    run += x[k];
  }
  __syncthreads();
  *largest = big;   // of this lane's wave
  return all;
}

__global__ __launch_bounds__(kKnnScanThreads) void k_knn_scan_chunks(int32_t *cnt, int64_t ncell,
                                                                     int32_t *sums,
                                                                     unsigned long long *stats) {
  __shared__ int lds[kKnnScanThreads / 64];
  int big;
  const int total = knn_scan_chunk(cnt, static_cast<int64_t>(blockIdx.x) * kKnnScanChunk, ncell,
                                   0, lds, &big);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
  if ((threadIdx.x & 63) == 0 && big > 0)
    atomicMax(&stats[kKnnLargest], static_cast<unsigned long long>(big));
}

// one workgroup turns v[0 .. m), the chunk sums, into exclusive offsets with the total in v[m]
__global__ __launch_bounds__(kKnnScanThreads) void k_knn_scan(int32_t *v, int64_t m) {
  __shared__ int lds[kKnnScanThreads / 64];
  int carry = 0, big;
  for (int64_t at = 0; at < m; at += kKnnScanChunk)
    carry += knn_scan_chunk(v, at, m, carry, lds, &big);
  if (threadIdx.x == 0) v[m] = carry;
}

// every chunk adds its offset: cnt[0 .. ncell) are the exclusive offsets, cnt[ncell] the total
__global__ __launch_bounds__(kKnnScanThreads) void k_knn_scan_add(int32_t *cnt, int64_t ncell,
                                                                  const int32_t *sums,
                                                                  int nchunks) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kKnnScanChunk +
                       static_cast<int64_t>(threadIdx.x) * kKnnScanItems;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kKnnScanItems; ++k)
    if (base + k < ncell) cnt[base + k] += add;
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[ncell] = sums[nchunks];
}

__global__ __launch_bounds__(kKnnThreads) void k_knn_scatter(const double *pts, int64_t n,
                                                             const int32_t *cell_of,
                                                             const int32_t *cnt, int32_t *fill,
                                                             int64_t nfin, double *packed,
                                                             int32_t *pidx) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kKnnThreads + threadIdx.x;
  if (i >= n) return;
  const int cell = cell_of[i];
  if (cell < 0) return;
  // below the cell's count: the count kernel counted this very point
  const int64_t at = static_cast<int64_t>(cnt[cell]) + atomicAdd(&fill[cell], 1);
  if (at >= nfin) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) packed[3 * at + a] = pts[3 * i + a];
  pidx[at] = static_cast<int32_t>(i);
}

// The walk of one lane over the Chebyshev rings around the cell of its finite position q: the
// lane's sorted list of the k smallest pairs (d2, index) within max_dist ends in its LDS columns
// ld and li (slot s at [s * 64]); returns the list's length and adds the candidates whose d2 was
// computed to *tested.
__device__ __forceinline__ int knn_walk(const double *packed, const int32_t *pidx,
                                        const int32_t *cnt, int64_t nfin, const KnnGrid &G, int k,
                                        double max_dist, const double *q, double *ld, int *li,
                                        unsigned long long *tested_out) {
#pragma clang fp contract(off)
  const double md2 = max_dist * max_dist;
  int have = 0, worst_j = kKnnNone;
  double worst_d = INFINITY;   // the k-th key once the list is full, (+inf, none) before
  unsigned long long tested = 0;
  int c[3], r0 = 0, rmax = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = static_cast<int>(knn_coord(q[a], G.lo[a], G.cell, kKnnFar));
    r0 = max(r0, max(-c[a], c[a] - (G.dim[a] - 1)));   // rings until this axis meets the grid
    rmax = max(rmax, max(c[a], G.dim[a] - 1 - c[a]));  // the last ring that touches it
  }
  // r0 <= rmax, and rmax - r0 is below the grid's largest dimension
  for (int r = r0; r <= rmax; ++r) {
    if (r > 0) {
      const double bound = static_cast<double>(r - 1) * G.cell * kKnnShrink;
      if ((have == k && worst_d <= bound * bound) || bound > max_dist) break;
    }
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, G.dim[2] - 1);
    const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, G.dim[1] - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        // a row on the shell's z or y faces is walked whole, another only at x = c0 -+ r
        const bool whole = z - c[2] == r || c[2] - z == r || y - c[1] == r || c[1] - y == r;
        const long long xs = whole ? max(c[0] - r, 0) : c[0] - r;
        const long long xe = whole ? min(c[0] + r, G.dim[0] - 1) : c[0] + r;
        const long long step = whole ? 1 : 2ll * r;   // r > 0 where a row is not whole
        for (long long x = xs; x <= xe; x += step) {
          if (x < 0 || x >= G.dim[0]) continue;
          const int64_t cell = (static_cast<int64_t>(z) * G.dim[1] + y) * G.dim[0] + x;
          const int64_t b = cnt[cell], e = min(static_cast<int64_t>(cnt[cell + 1]), nfin);
          for (int64_t at = b; at < e; ++at) {
            const double *p = packed + 3 * at;
            const double d0 = q[0] - p[0], d1 = q[1] - p[1], dz = q[2] - p[2];
            const double d = d0 * d0 + d1 * d1 + dz * dz;
            ++tested;
            if (!(d <= md2 && d <= worst_d)) continue;   // most candidates leave here
            const int j = pidx[at];
            if (!(d < worst_d || j < worst_j)) continue;
            // insertion from the tail; a full list loses its last entry
            int pos = have < k ? have : k - 1;
            while (pos > 0) {
              const double pd = ld[(pos - 1) * kKnnWave];
              const int pj = li[(pos - 1) * kKnnWave];
              if (pd < d || (pd == d && pj < j)) break;
              ld[pos * kKnnWave] = pd;
              li[pos * kKnnWave] = pj;
              --pos;
            }
            ld[pos * kKnnWave] = d;
            li[pos * kKnnWave] = j;
            if (have < k) ++have;
            if (have == k) {
              worst_d = ld[(k - 1) * kKnnWave];
              worst_j = li[(k - 1) * kKnnWave];
            }
          }
        }
      }
  }
  *tested_out += tested;
  return have;
}

// One lane per query.  queries == null: lane t takes entry t of the scattered list (cell order,
// so a wave walks the same cells) and writes to that point's own row; otherwise query t of m.
// Dynamic LDS: k * 64 doubles, then k * 64 ints.  d2 == null (the plane fit): only idx and count
// are written.
__global__ __launch_bounds__(kKnnWave) void k_knn_query(
    const double *packed, const int32_t *pidx, const int32_t *cnt, int64_t nfin,
    const double *queries, int64_t m, KnnGrid G, int k, double max_dist, int32_t *idx, double *d2,
    int32_t *count, unsigned long long *stats) {
#pragma clang fp contract(off)
  extern __shared__ double s_knn[];
  const int lane = threadIdx.x;
  double *ld = s_knn + lane;                                          // slot s at ld[s * 64]
  int *li = reinterpret_cast<int *>(s_knn + static_cast<size_t>(k) * kKnnWave) + lane;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kKnnWave + lane;
  const bool active = queries ? t < m : t < nfin;
  int64_t row = t;
  double q[3] = {0.0, 0.0, 0.0};
  if (active) {
    const double *src = queries ? queries + 3 * t : packed + 3 * t;
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = src[a];
    if (!queries) row = pidx[t];
  }
  const bool finite = knn_finite3(q);
  int have = 0;
  unsigned long long tested = 0;
  if (active && finite)
    have = knn_walk(packed, pidx, cnt, nfin, G, k, max_dist, q, ld, li, &tested);
  for (int off = 32; off > 0; off >>= 1) tested += __shfl_xor(tested, off);
  if (lane == 0 && tested > 0) atomicAdd(&stats[kKnnTested], tested);
  if (!active) return;
  count[row] = have;
  for (int s = 0; s < k; ++s) {
    idx[row * k + s] = s < have ? li[s * kKnnWave] : -1;
    if (d2) d2[row * k + s] = s < have ? ld[s * kKnnWave] : INFINITY;
  }
}

// One lane per point over its own row of the lists (`rows` wide).  M about the point itself, the
// sums in list order; the eigen-solve and the sign are those of k_cloud_normals.
__global__ __launch_bounds__(kKnnThreads) void k_knn_normals(const double *pts, int64_t n,
                                                             const double *orient, int rows,
                                                             const int32_t *idx,
                                                             const int32_t *count,
                                                             double *normals, double *evals) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kKnnThreads + threadIdx.x;
  if (i >= n) return;
  const int k = min(count[i], rows);
  double nrm[3] = {knn_nan(), knn_nan(), knn_nan()};
  double ev[3] = {knn_nan(), knn_nan(), knn_nan()};
  if (k >= 3) {
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    double s[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = 0; e < k; ++e) {
      const int64_t j = idx[i * rows + e];
      if (j < 0 || j >= n) continue;   // never: the list holds point indices
      const double d0 = pts[3 * j] - p[0], d1 = pts[3 * j + 1] - p[1], d2 = pts[3 * j + 2] - p[2];
      s[0] += d0;
      s[1] += d1;
      s[2] += d2;
      S[0] += d0 * d0;
      S[1] += d0 * d1;
      S[2] += d0 * d2;
      S[3] += d1 * d1;
      S[4] += d1 * d2;
      S[5] += d2 * d2;
    }
    const double c = static_cast<double>(k);
    const double m0 = s[0] / c, m1 = s[1] / c, m2 = s[2] / c;
    double A[9], V[9];
    A[0] = S[0] / c - m0 * m0;
    A[1] = A[3] = S[1] / c - m0 * m1;
    A[2] = A[6] = S[2] / c - m0 * m2;
    A[4] = S[3] / c - m1 * m1;
    A[5] = A[7] = S[4] / c - m1 * m2;
    A[8] = S[5] / c - m2 * m2;
    jacobi3(A, V);
    // ascending eigenvalues; equal ones keep their column order
    int o0 = 0, o1 = 1, o2 = 2;
    if (A[4 * o1] < A[4 * o0]) { const int w = o0; o0 = o1; o1 = w; }
    if (A[4 * o2] < A[4 * o1]) { const int w = o1; o1 = o2; o2 = w; }
    if (A[4 * o1] < A[4 * o0]) { const int w = o0; o0 = o1; o1 = w; }
    ev[0] = A[4 * o0];
    ev[1] = A[4 * o1];
    ev[2] = A[4 * o2];
    double v[3] = {V[o0], V[3 + o0], V[6 + o0]};
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] /= len;
    bool flip;
    const double *o = orient ? orient + 3 * i : nullptr;
    if (o && knn_finite3(o) && (o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0)) {
      flip = v[0] * o[0] + v[1] * o[1] + v[2] * o[2] < 0.0;
    } else {
      int big = 0;
      if (fabs(v[1]) > fabs(v[big])) big = 1;
      if (fabs(v[2]) > fabs(v[big])) big = 2;
      flip = v[big] < 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) nrm[a] = flip ? -v[a] : v[a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    normals[3 * i + a] = nrm[a];
    evals[3 * i + a] = ev[a];
  }
}

// One lane per point over its own row of k + 1 entries: the entry that names the point itself
// is dropped, the last one where there is none.
__global__ __launch_bounds__(kKnnThreads) void k_knn_mean(int64_t n, int rows, const int32_t *idx,
                                                          const double *d2, const int32_t *count,
                                                          double *mean) {
#pragma clang fp contract(off)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kKnnThreads + threadIdx.x;
  if (i >= n) return;
  const int c = min(count[i], rows);
  int drop = c - 1;
  for (int e = 0; e < c; ++e)
    if (idx[i * rows + e] == i) {
      drop = e;
      break;
    }
  double sum = 0.0;
  for (int e = 0; e < c; ++e)
    if (e != drop) sum += sqrt(d2[i * rows + e]);
  mean[i] = c > 1 ? sum / static_cast<double>(c - 1) : knn_nan();
}

// ---- surface from oriented points (rs_surface_points_volume, rs_surface_points_eval) ----

// How the lanes of a wave map to the nodes of a volume: 1, a brick of 4 x 4 x 4 nodes, so that a
// wave's lanes walk the same cells; 0, a run of 64 nodes along x.  Measured: DESIGN.md section 21.
#ifndef RS_POINTS_BRICK
#define RS_POINTS_BRICK 1
#endif
constexpr int kPtsBrickX = RS_POINTS_BRICK ? 4 : 64, kPtsBrickYZ = RS_POINTS_BRICK ? 4 : 1;

// further stats words
constexpr int kPtsDefined = 2, kPtsSaturated = 3;

struct PtsVolume {
  double o[3], voxel;
  int n[3];   // nx, ny, nz
  int b[2];   // bricks along x and y
};

// A point whose normal is not finite is out: its coordinates become NaN in the copy the grid is
// built from, where the k-NN kernels drop it like any non-finite point.
__global__ __launch_bounds__(kKnnThreads) void k_points_mask(const double *pts,
                                                             const double *normals, int64_t n,
                                                             double *out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kKnnThreads + threadIdx.x;
  if (i >= n) return;
  const bool in = knn_finite3(normals + 3 * i);
#pragma unroll
  for (int a = 0; a < 3; ++a) out[3 * i + a] = in ? pts[3 * i + a] : knn_nan();
}

// One lane per node (kVolume: workgroup w is brick w of the volume) or per query (lane t of m),
// one wave per workgroup.  k_knn_query's walk with max_dist = radius leaves the sorted list in
// the lane's LDS columns (dynamic LDS: k * 64 doubles, then k * 64 ints); the slot loop of the
// contract consumes it where it stands and 8 bytes per node leave the chip.  `pts` is the masked
// copy, so a listed index names a point with six finite numbers; it is below n because k_knn_
// scatter wrote it from a lane index below n.
template <bool kVolume>
__global__ __launch_bounds__(kKnnWave) void k_points_field(
    const double *packed, const int32_t *pidx, const int32_t *cnt, int64_t nfin, const double *pts,
    const double *normals, const double *colors, int64_t n, const double *queries, int64_t m,
    PtsVolume V, KnnGrid G, int k, double radius, double trunc, float *tsdf, float *weight,
    double *value, int32_t *count, double *color, unsigned long long *stats) {
#pragma clang fp contract(off)
  extern __shared__ double s_knn[];
  const int lane = threadIdx.x;
  double *ld = s_knn + lane;                                          // slot s at ld[s * 64]
  int *li = reinterpret_cast<int *>(s_knn + static_cast<size_t>(k) * kKnnWave) + lane;
  int64_t out = -1;   // the lane's output element, -1: none
  double q[3] = {0.0, 0.0, 0.0};
  if (kVolume) {
    const int64_t w = blockIdx.x, rest = w / V.b[0];
    const int bx = static_cast<int>(w - rest * V.b[0]), bz = static_cast<int>(rest / V.b[1]);
    const int by = static_cast<int>(rest - static_cast<int64_t>(bz) * V.b[1]);
    const int lx = lane % kPtsBrickX, ly = lane / kPtsBrickX % kPtsBrickYZ,
              lz = lane / kPtsBrickX / kPtsBrickYZ;
    const int i[3] = {bx * kPtsBrickX + lx, by * kPtsBrickYZ + ly, bz * kPtsBrickYZ + lz};
    if (i[0] < V.n[0] && i[1] < V.n[1] && i[2] < V.n[2]) {
      out = (static_cast<int64_t>(i[2]) * V.n[1] + i[1]) * V.n[0] + i[0];
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = V.o[a] + V.voxel * static_cast<double>(i[a]);
    }
  } else {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kKnnWave + lane;
    if (t < m) {
      out = t;
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = queries[3 * t + a];
    }
  }
  int have = 0;
  unsigned long long tested = 0;
  if (out >= 0 && knn_finite3(q))
    have = knn_walk(packed, pidx, cnt, nfin, G, k, radius, q, ld, li, &tested);
  double acc = 0.0, sw = 0.0, cacc[3] = {0.0, 0.0, 0.0};
  for (int s = 0; s < have; ++s) {
    const int64_t j = li[s * kKnnWave];
    if (j < 0 || j >= n) continue;   // never: the list holds point indices
    const double *p = pts + 3 * j, *nj = normals + 3 * j;
    const double d0 = q[0] - p[0], d1 = q[1] - p[1], dz = q[2] - p[2];
    const double u = fmin(sqrt(ld[s * kKnnWave]) / radius, 1.0);
    const double a = 1.0 - u, a2 = a * a;
    const double wt = (a2 * a2) * (4.0 * u + 1.0);
    const double dot = d0 * nj[0] + d1 * nj[1] + dz * nj[2];
    acc += wt * dot;
    sw += wt;
    if (!kVolume && colors) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) cacc[ch] += wt * colors[3 * j + ch];
    }
  }
  const bool some = sw > 0.0;
  const double f = some ? acc / sw : knn_nan();
  const unsigned long long defined = __popcll(__ballot(out >= 0 && isfinite(f)));
  const unsigned long long full = __popcll(__ballot(out >= 0 && have == k));
  for (int off = 32; off > 0; off >>= 1) tested += __shfl_xor(tested, off);
  if (lane == 0) {
    if (tested > 0) atomicAdd(&stats[kKnnTested], tested);
    if (defined > 0) atomicAdd(&stats[kPtsDefined], defined);
    if (full > 0) atomicAdd(&stats[kPtsSaturated], full);
  }
  if (out < 0) return;
  if (kVolume) {
    double t = f / trunc;   // a NaN passes both comparisons
    t = t > 1.0 ? 1.0 : t;
    t = t < -1.0 ? -1.0 : t;
    tsdf[out] = some ? static_cast<float>(t) : __int_as_float(0x7fc00000);
    weight[out] = static_cast<float>(have);
  } else {
    value[out] = f;
    count[out] = have;
    if (color) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) color[3 * out + ch] = some ? cacc[ch] / sw : knn_nan();
    }
  }
}

}  // namespace rsd

static_assert(RS_CLOUD_KNN_TIMING_SLOTS == 7, "box, grid, scan, scatter, query, normals, mean_dist");
static_assert(sizeof(rs_knn_info) == 40, "rs_knn_info");

namespace {

enum KnnUse { kKnnLists = 0, kKnnNormals = 1, kKnnMean = 2, kKnnFpfh = 3 };

struct KnnOut {
  int32_t *idx = nullptr;      // lists
  double *d2 = nullptr;        // lists
  int32_t *count = nullptr;    // all
  double *normals = nullptr;   // normals
  double *evals = nullptr;     // normals
  double *mean = nullptr;      // mean
  double *fpfh = nullptr;      // fpfh: (n, 33)
  int32_t *pairs = nullptr;    // fpfh: the counted pairs per point
};

// what a call without a finite point returns: empty lists, NaN rows
void knn_fill_empty(KnnUse use, int64_t n, int64_t m, int K, const KnnOut &o) {
  for (int64_t i = 0; i < m; ++i) o.count[i] = 0;
  if (use == kKnnLists)
    for (int64_t i = 0; i < m * K; ++i) {
      o.idx[i] = -1;
      o.d2[i] = INFINITY;
    }
  if (use == kKnnNormals)
    for (int64_t i = 0; i < 3 * n; ++i) o.normals[i] = o.evals[i] = NAN;
  if (use == kKnnMean)
    for (int64_t i = 0; i < n; ++i) o.mean[i] = NAN;
  if (use == kKnnFpfh) {
    for (int64_t i = 0; i < n; ++i) o.pairs[i] = 0;
    for (int64_t i = 0; i < RS_FPFH_BINS * n; ++i) o.fpfh[i] = NAN;
  }
}

// The grid over the box [lo, hi] of nfin > 0 finite points (box: what k_knn_box_fold leaves).
// cell == 0 picks the default: rs_cloud_knn's with radius == 0, that of the surface from points
// with its support radius.  RS_EINVAL with the message of the rule that failed.
int knn_size_grid(const double *box, int64_t nfin, double cell, double radius, rsd::KnnGrid *G) {
  double ext_max = 0.0, mag = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double ext = box[3 + a] - box[a];
    if (!std::isfinite(ext)) return fail(RS_EINVAL, "the extent of the cloud's box is not finite");
    ext_max = std::fmax(ext_max, ext);
    mag = std::fmax(mag, std::fmax(std::fabs(box[a]), std::fabs(box[3 + a])));
    G->lo[a] = box[a];
  }
  if (cell == 0.0 && radius > 0.0) {
    // surface from points: a hair above the support radius, so that B = cell (1 - 2^-20) exceeds
    // it and the walk ends after ring 1, 27 cells (at cell == radius exactly it takes ring 2 as
    // well, 125 cells: measured); raised to the floor and until the grid fits
    cell = std::fmax(radius * (1.0 + 1.0 / 524288.0), mag / 16777216.0);
    for (;;) {
      double cells = 1.0, side = 0.0;
      for (int a = 0; a < 3; ++a) {
        const double nd = std::floor((box[3 + a] - box[a]) / cell) + 1.0;
        side = std::fmax(side, nd);
        cells *= nd;
      }
      if (side <= static_cast<double>(RS_CLOUD_KNN_MAX_CELLS) &&
          cells <= static_cast<double>(RS_CLOUD_KNN_MAX_CELLS))
        break;
      cell *= 1.125;
    }
  } else if (cell == 0.0) {
    const double g = std::fmin(std::fmax(std::round(std::cbrt(static_cast<double>(nfin))), 1.0),
                               256.0);
    cell = std::fmax(ext_max / g, mag / 16777216.0);
    if (!(ext_max > 0.0) || !(cell > 0.0)) cell = mag > 0.0 ? mag : 1.0;   // one cell
  }
  double ncell_d = 1.0;
  for (int a = 0; a < 3; ++a) {
    const double nd = std::floor((box[3 + a] - box[a]) / cell) + 1.0;
    if (!(nd <= static_cast<double>(RS_CLOUD_KNN_MAX_CELLS)))
      return fail(RS_EINVAL,
                  "the grid has more than RS_CLOUD_KNN_MAX_CELLS = 2^24 cells: choose a larger "
                  "cell");
    G->dim[a] = static_cast<int>(nd);
    ncell_d *= nd;
  }
  if (ncell_d > static_cast<double>(RS_CLOUD_KNN_MAX_CELLS))
    return fail(RS_EINVAL,
                "the grid has more than RS_CLOUD_KNN_MAX_CELLS = 2^24 cells: choose a larger cell");
  if (cell < mag / 16777216.0)
    return fail(RS_EINVAL,
                "cell is below 2^-24 of the box's largest coordinate magnitude: choose a larger "
                "cell");
  G->cell = cell;
  return RS_OK;
}

// The grid, the query with lists K wide and, for the consumers, their kernel.  The arguments have
// been checked: 1 <= K <= RS_CLOUD_KNN_MAX_K, 0 < n, m <= RS_CLOUD_MAX_POINTS, queries null only
// with m == n, max_dist >= 0, cell >= 0 and finite.  For the descriptors (kKnnFpfh) `orient`
// carries the normals and the kernels of global_reg.hip follow the query.
int knn_run(rs_ctx *c, KnnUse use, const double *pts, int64_t n, const double *queries, int64_t m,
            int K, double max_dist, double cell, const double *orient, const KnnOut &o,
            rs_knn_info *info) {
  using U64 = unsigned long long;
  const int nb = static_cast<int>(std::min<int64_t>(rsd::kKnnBoxBlocks,
                                                    rs::blocks(n, rsd::kKnnThreads)));
  const size_t sn = static_cast<size_t>(n), sm = static_cast<size_t>(m), sK = static_cast<size_t>(K);
  // [pts | queries | orient] go up and the box comes down before the grid can be sized ...
  rs::Layout L;
  const auto b_pts = L.add<double>(3 * sn);
  const auto b_q = L.add<double>(queries ? 3 * sm : 0);
  const auto b_orient = L.add<double>(orient ? 3 * sn : 0);
  const auto b_part = L.add<double>(7 * static_cast<size_t>(nb)), b_box = L.add<double>(8);
  // ... the lists, the results and the scattered points do not depend on it ...
  const auto b_idx = L.add<int32_t>(sm * sK);
  const auto b_d2 = L.add<double>(use == kKnnNormals ? 0 : sm * sK);   // the plane fit reads none
  const auto b_count = L.add<int32_t>(sm);
  const auto b_res = L.add<double>(use == kKnnNormals ? 6 * sn
                                   : use == kKnnMean  ? sn
                                   : use == kKnnFpfh  ? RS_FPFH_BINS * sn
                                                      : 0);
  const auto b_spfh = L.add<int32_t>(use == kKnnFpfh ? RS_FPFH_BINS * sn : 0);
  const auto b_pairs = L.add<int32_t>(use == kKnnFpfh ? sn : 0);
  const auto b_stats = L.add<U64>(8);
  const auto b_packed = L.add<double>(3 * sn);
  const auto b_pidx = L.add<int32_t>(sn), b_cell_of = L.add<int32_t>(sn);
  HIP_TRY(hipSetDevice(c->device));
  // ... and the default grid has at most (G + 1)^3 cells: one allocation in the usual case
  const double g0 = std::fmin(std::fmax(std::round(std::cbrt(static_cast<double>(n))), 1.0), 256.0);
  const size_t guess = cell == 0.0 ? static_cast<size_t>((g0 + 1) * (g0 + 1) * (g0 + 1)) * 8 + 65536
                                   : 0;
  int st = L.bind(c, 256 + guess);
  if (st) return st;

  hipStream_t s = c->stream;
  const dim3 blk(rsd::kKnnThreads), sblk(rsd::kKnnScanThreads);
  auto upload = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(b_pts.dev(), pts, b_pts.bytes, hipMemcpyHostToDevice, s));
    if (queries) HIP_TRY(hipMemcpyAsync(b_q.dev(), queries, b_q.bytes, hipMemcpyHostToDevice, s));
    if (orient)
      HIP_TRY(hipMemcpyAsync(b_orient.dev(), orient, b_orient.bytes, hipMemcpyHostToDevice, s));
    return RS_OK;
  };
  if ((st = upload())) return st;
  if ((st = c->knn.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_knn_box, dim3(nb), blk, 0, s, b_pts.dev(), n, b_part.dev());
  hipLaunchKernelGGL(rsd::k_knn_box_fold, dim3(1), dim3(rsd::kKnnWave), 0, s, b_part.dev(), nb,
                     b_box.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->knn.mark(1, s))) return st;
  double box[7];
  HIP_TRY(hipMemcpyAsync(box, b_box.dev(), sizeof(box), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->knn.read(0, 0, 1))) return st;

  const int64_t nfin = static_cast<int64_t>(box[6]);
  if (nfin <= 0) {
    knn_fill_empty(use, n, m, K, o);
    info->rows_short = m;
    return RS_OK;
  }
  rsd::KnnGrid G;
  if ((st = knn_size_grid(box, nfin, cell, 0.0, &G))) return st;
  const int64_t ncell = static_cast<int64_t>(G.dim[0]) * G.dim[1] * G.dim[2];
  const int nchunks = static_cast<int>((ncell + rsd::kKnnScanChunk - 1) / rsd::kKnnScanChunk);
  const auto b_cnt = L.add<int32_t>(static_cast<size_t>(ncell) + 1);
  const auto b_fill = L.add<int32_t>(static_cast<size_t>(ncell));
  const auto b_sums = L.add<int32_t>(static_cast<size_t>(nchunks) + 1);
  // a scratch that has to grow is freed and allocated anew, without a copy (and perhaps at the
  // same address): decide by its capacity whether the inputs go up again
  const bool kept = c->scratch_bytes >= L.total() + 256;
  if ((st = L.bind(c))) return st;
  if (!kept && (st = upload())) return st;
  double *const d_d2 = use == kKnnNormals ? nullptr : b_d2.dev();   // null: no d2 is written

  const bool self = queries == nullptr;
  HIP_TRY(hipMemsetAsync(b_stats.dev(), 0, b_stats.bytes, s));
  HIP_TRY(hipMemsetAsync(b_cnt.dev(), 0, L.span(b_cnt, b_sums), s));   // cnt and fill
  if ((st = c->knn.mark(2, s))) return st;
  hipLaunchKernelGGL(rsd::k_knn_count, dim3(rs::blocks(n, rsd::kKnnThreads)), blk, 0, s,
                     b_pts.dev(), n, G, b_cell_of.dev(), b_cnt.dev(), self ? K : 0, b_idx.dev(),
                     d_d2, b_count.dev());
  if ((st = c->knn.mark(3, s))) return st;
  hipLaunchKernelGGL(rsd::k_knn_scan_chunks, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), b_stats.dev());
  hipLaunchKernelGGL(rsd::k_knn_scan, dim3(1), sblk, 0, s, b_sums.dev(),
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_knn_scan_add, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), nchunks);
  if ((st = c->knn.mark(4, s))) return st;
  hipLaunchKernelGGL(rsd::k_knn_scatter, dim3(rs::blocks(n, rsd::kKnnThreads)), blk, 0, s,
                     b_pts.dev(), n, b_cell_of.dev(), b_cnt.dev(), b_fill.dev(), nfin,
                     b_packed.dev(), b_pidx.dev());
  if ((st = c->knn.mark(5, s))) return st;
  const int64_t lanes = self ? nfin : m;
  hipLaunchKernelGGL(rsd::k_knn_query, dim3(rs::blocks(lanes, rsd::kKnnWave)),
                     dim3(rsd::kKnnWave), 768 * sK, s, b_packed.dev(), b_pidx.dev(), b_cnt.dev(),
                     nfin, self ? nullptr : b_q.dev(), m, G, K, max_dist, b_idx.dev(), d_d2,
                     b_count.dev(), b_stats.dev());
  if ((st = c->knn.mark(6, s))) return st;
  if (use == kKnnNormals)
    hipLaunchKernelGGL(rsd::k_knn_normals, dim3(rs::blocks(n, rsd::kKnnThreads)), blk, 0, s,
                       b_pts.dev(), n, orient ? b_orient.dev() : nullptr, K, b_idx.dev(),
                       b_count.dev(), b_res.dev(), b_res.dev() + 3 * n);
  if (use == kKnnMean)
    hipLaunchKernelGGL(rsd::k_knn_mean, dim3(rs::blocks(n, rsd::kKnnThreads)), blk, 0, s, n, K,
                       b_idx.dev(), b_d2.dev(), b_count.dev(), b_res.dev());
  if (use == kKnnFpfh)
    rs::fpfh_launch(c, b_pts.dev(), b_orient.dev(), n, K, b_idx.dev(), b_d2.dev(), b_count.dev(),
                    b_spfh.dev(), b_pairs.dev(), b_res.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->knn.mark(7, s))) return st;
  U64 stats[8];
  if (use == kKnnLists) {
    HIP_TRY(hipMemcpyAsync(o.idx, b_idx.dev(), b_idx.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(o.d2, b_d2.dev(), b_d2.bytes, hipMemcpyDeviceToHost, s));
  } else if (use == kKnnNormals) {
    HIP_TRY(hipMemcpyAsync(o.normals, b_res.dev(), 3 * sn * sizeof(double), hipMemcpyDeviceToHost,
                           s));
    HIP_TRY(hipMemcpyAsync(o.evals, b_res.dev() + 3 * n, 3 * sn * sizeof(double),
                           hipMemcpyDeviceToHost, s));
  } else if (use == kKnnFpfh) {
    HIP_TRY(hipMemcpyAsync(o.fpfh, b_res.dev(), b_res.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(o.pairs, b_pairs.dev(), b_pairs.bytes, hipMemcpyDeviceToHost, s));
  } else {
    HIP_TRY(hipMemcpyAsync(o.mean, b_res.dev(), b_res.bytes, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipMemcpyAsync(o.count, b_count.dev(), b_count.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(stats, b_stats.dev(), b_stats.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 1; k < 5; ++k)
    if ((st = c->knn.read(k, k + 1, k + 2))) return st;
  if ((use == kKnnNormals || use == kKnnMean) &&
      (st = c->knn.read(use == kKnnNormals ? 5 : 6, 6, 7)))
    return st;
  if (use == kKnnFpfh && (st = rs::fpfh_read_timing(c))) return st;

  info->cells = ncell;
  info->largest_cell = static_cast<int64_t>(stats[rsd::kKnnLargest]);
  info->tested = static_cast<int64_t>(stats[rsd::kKnnTested]);
  for (int64_t i = 0; i < m; ++i) {
    info->found += o.count[i];
    info->rows_short += o.count[i] < K ? 1 : 0;
  }
  return RS_OK;
}

int knn_check(const rs_ctx *c, const rs_knn_info *info, int64_t n, int64_t m, int32_t k,
              int32_t kmax, double max_dist, double cell) {
  if (!c || !info) return fail(RS_EINVAL, "null pointer");
  if (k < 1 || k > kmax)
    return fail(RS_EINVAL, kmax == RS_CLOUD_KNN_MAX_K
                               ? "k must be in 1..RS_CLOUD_KNN_MAX_K = 64"
                               : "k must be in 1..RS_CLOUD_KNN_MAX_K - 1 = 63");
  if (n < 0 || m < 0) return fail(RS_EINVAL, "negative size");
  if (n > RS_CLOUD_MAX_POINTS || m > RS_CLOUD_MAX_POINTS)
    return fail(RS_EINVAL, "more points or queries than RS_CLOUD_MAX_POINTS = 2^28");
  if (!(max_dist >= 0.0)) return fail(RS_EINVAL, "max_dist must be >= 0 (+inf is allowed)");
  if (!std::isfinite(cell) || cell < 0.0)
    return fail(RS_EINVAL, "cell must be finite and >= 0 (0: the default)");
  return RS_OK;
}

}  // namespace

extern "C" int rs_cloud_knn(rs_ctx *c, const double *pts, int64_t n, const double *queries,
                            int64_t m, int32_t k, double max_dist, double cell, int32_t *idx,
                            double *d2, int32_t *count, rs_knn_info *info) {
  int st = knn_check(c, info, n, m, k, RS_CLOUD_KNN_MAX_K, max_dist, cell);
  if (st) return st;
  if (n > 0 && !pts) return fail(RS_EINVAL, "null pointer: pts");
  if (!queries && m != n)
    return fail(RS_EINVAL, "without queries the points are the queries: m must equal n");
  const rs_knn_info zero = {0, 0, 0, 0, 0};
  *info = zero;
  if (m == 0) return RS_OK;
  if (!idx || !d2 || !count) return fail(RS_EINVAL, "null pointer");
  KnnOut o;
  o.idx = idx;
  o.d2 = d2;
  o.count = count;
  if (n == 0) {
    knn_fill_empty(kKnnLists, n, m, k, o);
    info->rows_short = m;
    return RS_OK;
  }
  return knn_run(c, kKnnLists, pts, n, queries, m, k, max_dist, cell, nullptr, o, info);
}

extern "C" int rs_cloud_knn_normals(rs_ctx *c, const double *pts, int64_t n, int32_t k,
                                    double cell, const double *orient, double *normals,
                                    double *evals, int32_t *count, rs_knn_info *info) {
  int st = knn_check(c, info, n, n, k, RS_CLOUD_KNN_MAX_K, INFINITY, cell);
  if (st) return st;
  const rs_knn_info zero = {0, 0, 0, 0, 0};
  *info = zero;
  if (n == 0) return RS_OK;
  if (!pts || !normals || !evals || !count) return fail(RS_EINVAL, "null pointer");
  KnnOut o;
  o.normals = normals;
  o.evals = evals;
  o.count = count;
  return knn_run(c, kKnnNormals, pts, n, nullptr, n, k, INFINITY, cell, orient, o, info);
}

extern "C" int rs_cloud_knn_mean_dist(rs_ctx *c, const double *pts, int64_t n, int32_t k,
                                      double cell, double *mean_dist, int32_t *count,
                                      rs_knn_info *info) {
  int st = knn_check(c, info, n, n, k, RS_CLOUD_KNN_MAX_K - 1, INFINITY, cell);
  if (st) return st;
  const rs_knn_info zero = {0, 0, 0, 0, 0};
  *info = zero;
  if (n == 0) return RS_OK;
  if (!pts || !mean_dist || !count) return fail(RS_EINVAL, "null pointer");
  KnnOut o;
  o.mean = mean_dist;
  o.count = count;
  return knn_run(c, kKnnMean, pts, n, nullptr, n, k + 1, INFINITY, cell, nullptr, o, info);
}

extern "C" int rs_cloud_fpfh(rs_ctx *c, const double *pts, const double *normals, int64_t n,
                             int32_t k, double cell, double *fpfh, int32_t *count,
                             rs_knn_info *info) {
  int st = knn_check(c, info, n, n, k, RS_CLOUD_KNN_MAX_K - 1, INFINITY, cell);
  if (st) return st;
  const rs_knn_info zero = {0, 0, 0, 0, 0};
  *info = zero;
  if (n == 0) return RS_OK;
  if (!pts || !normals || !fpfh || !count) return fail(RS_EINVAL, "null pointer");
  std::vector<int32_t> listed(static_cast<size_t>(n));   // the lists' lengths, for info
  KnnOut o;
  o.fpfh = fpfh;
  o.pairs = count;
  o.count = listed.data();
  return knn_run(c, kKnnFpfh, pts, n, nullptr, n, k + 1, INFINITY, cell, normals, o, info);
}

extern "C" int rs_cloud_knn_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->knn.enable(enable != 0);
  if (st) return st;
  c->knn.copy_out(ms);
  return RS_OK;
}

// ---- surface from oriented points ----

static_assert(RS_SURFACE_POINTS_TIMING_SLOTS == 5, "box, grid, scan, scatter, field");
static_assert(sizeof(rs_points_info) == 40, "rs_points_info");

namespace {

struct PtsOut {
  float *tsdf = nullptr, *weight = nullptr;                      // volume
  double *value = nullptr, *color = nullptr;                     // eval
  int32_t *count = nullptr;                                      // eval
};

// what a call without a point that is not out returns: NaN everywhere, no neighbour
void points_fill_empty(bool volume, int64_t m, const PtsOut &o) {
  for (int64_t i = 0; i < m; ++i) {
    if (volume) {
      o.tsdf[i] = NAN;
      o.weight[i] = 0.0f;
    } else {
      o.value[i] = NAN;
      o.count[i] = 0;
      if (o.color) o.color[3 * i] = o.color[3 * i + 1] = o.color[3 * i + 2] = NAN;
    }
  }
}

// The grid of knn_run over the points that are not out, then the field on the m nodes of the
// volume V (queries == null) or at the m queries.  The arguments have been checked.
int points_run(rs_ctx *c, const double *pts, const double *normals, const double *colors,
               int64_t n, const double *queries, int64_t m, const rsd::PtsVolume &V, int K,
               double radius, double trunc, double cell, const PtsOut &o, rs_points_info *info) {
  using U64 = unsigned long long;
  const bool volume = queries == nullptr;
  const int nb = static_cast<int>(std::min<int64_t>(rsd::kKnnBoxBlocks,
                                                    rs::blocks(n, rsd::kKnnThreads)));
  const size_t sn = static_cast<size_t>(n), sm = static_cast<size_t>(m);
  // the inputs go up and the box comes down before the grid can be sized ...
  rs::Layout L;
  const auto b_pts = L.add<double>(3 * sn), b_nrm = L.add<double>(3 * sn);
  const auto b_col = L.add<double>(colors ? 3 * sn : 0);
  const auto b_q = L.add<double>(volume ? 0 : 3 * sm);
  const auto b_in = L.add<double>(3 * sn);   // the points that are not out, NaN rows for the rest
  const auto b_part = L.add<double>(7 * static_cast<size_t>(nb)), b_box = L.add<double>(8);
  // ... the results and the scattered points do not depend on it
  const auto b_tsdf = L.add<float>(volume ? sm : 0), b_weight = L.add<float>(volume ? sm : 0);
  const auto b_value = L.add<double>(volume ? 0 : sm);
  const auto b_count = L.add<int32_t>(volume ? 0 : sm);
  const auto b_color = L.add<double>(colors ? 3 * sm : 0);
  const auto b_stats = L.add<U64>(8);
  const auto b_packed = L.add<double>(3 * sn);
  const auto b_pidx = L.add<int32_t>(sn), b_cell_of = L.add<int32_t>(sn);
  HIP_TRY(hipSetDevice(c->device));
  int st = L.bind(c);
  if (st) return st;

  hipStream_t s = c->stream;
  const dim3 blk(rsd::kKnnThreads), sblk(rsd::kKnnScanThreads);
  auto upload = [&]() -> int {
    HIP_TRY(hipMemcpyAsync(b_pts.dev(), pts, b_pts.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b_nrm.dev(), normals, b_nrm.bytes, hipMemcpyHostToDevice, s));
    if (colors)
      HIP_TRY(hipMemcpyAsync(b_col.dev(), colors, b_col.bytes, hipMemcpyHostToDevice, s));
    if (!volume) HIP_TRY(hipMemcpyAsync(b_q.dev(), queries, b_q.bytes, hipMemcpyHostToDevice, s));
    return RS_OK;
  };
  auto mask = [&]() {
    hipLaunchKernelGGL(rsd::k_points_mask, dim3(rs::blocks(n, rsd::kKnnThreads)), blk, 0, s,
                       b_pts.dev(), b_nrm.dev(), n, b_in.dev());
  };
  if ((st = upload())) return st;
  if ((st = c->points.mark(0, s))) return st;
  mask();
  hipLaunchKernelGGL(rsd::k_knn_box, dim3(nb), blk, 0, s, b_in.dev(), n, b_part.dev());
  hipLaunchKernelGGL(rsd::k_knn_box_fold, dim3(1), dim3(rsd::kKnnWave), 0, s, b_part.dev(), nb,
                     b_box.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->points.mark(1, s))) return st;
  double box[7];
  HIP_TRY(hipMemcpyAsync(box, b_box.dev(), sizeof(box), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->points.read(0, 0, 1))) return st;

  const int64_t nfin = static_cast<int64_t>(box[6]);
  if (nfin <= 0) {
    points_fill_empty(volume, m, o);
    return RS_OK;
  }
  rsd::KnnGrid G;
  if ((st = knn_size_grid(box, nfin, cell, radius, &G))) return st;
  const int64_t ncell = static_cast<int64_t>(G.dim[0]) * G.dim[1] * G.dim[2];
  const int nchunks = static_cast<int>((ncell + rsd::kKnnScanChunk - 1) / rsd::kKnnScanChunk);
  const auto b_cnt = L.add<int32_t>(static_cast<size_t>(ncell) + 1);
  const auto b_fill = L.add<int32_t>(static_cast<size_t>(ncell));
  const auto b_sums = L.add<int32_t>(static_cast<size_t>(nchunks) + 1);
  // a scratch that has to grow is allocated anew without a copy: the inputs go up again
  const bool kept = c->scratch_bytes >= L.total() + 256;
  if ((st = L.bind(c))) return st;
  if (!kept) {
    if ((st = upload())) return st;
    mask();
  }

  HIP_TRY(hipMemsetAsync(b_stats.dev(), 0, b_stats.bytes, s));
  HIP_TRY(hipMemsetAsync(b_cnt.dev(), 0, L.span(b_cnt, b_sums), s));   // cnt and fill
  if ((st = c->points.mark(2, s))) return st;
  hipLaunchKernelGGL(rsd::k_knn_count, dim3(rs::blocks(n, rsd::kKnnThreads)), blk, 0, s,
                     b_in.dev(), n, G, b_cell_of.dev(), b_cnt.dev(), 0, nullptr, nullptr, nullptr);
  if ((st = c->points.mark(3, s))) return st;
  hipLaunchKernelGGL(rsd::k_knn_scan_chunks, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), b_stats.dev());
  hipLaunchKernelGGL(rsd::k_knn_scan, dim3(1), sblk, 0, s, b_sums.dev(),
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_knn_scan_add, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), nchunks);
  if ((st = c->points.mark(4, s))) return st;
  hipLaunchKernelGGL(rsd::k_knn_scatter, dim3(rs::blocks(n, rsd::kKnnThreads)), blk, 0, s,
                     b_in.dev(), n, b_cell_of.dev(), b_cnt.dev(), b_fill.dev(), nfin,
                     b_packed.dev(), b_pidx.dev());
  if ((st = c->points.mark(5, s))) return st;
  const size_t lds = 768 * static_cast<size_t>(K);
  if (volume) {
    const unsigned bricks = static_cast<unsigned>(
        static_cast<int64_t>(V.b[0]) * V.b[1] * rs::blocks(V.n[2], rsd::kPtsBrickYZ));
    hipLaunchKernelGGL(rsd::k_points_field<true>, dim3(bricks), dim3(rsd::kKnnWave), lds, s,
                       b_packed.dev(), b_pidx.dev(), b_cnt.dev(), nfin, b_in.dev(), b_nrm.dev(),
                       nullptr, n, nullptr, m, V, G, K, radius, trunc, b_tsdf.dev(),
                       b_weight.dev(), nullptr, nullptr, nullptr, b_stats.dev());
  } else {
    hipLaunchKernelGGL(rsd::k_points_field<false>, dim3(rs::blocks(m, rsd::kKnnWave)),
                       dim3(rsd::kKnnWave), lds, s, b_packed.dev(), b_pidx.dev(), b_cnt.dev(),
                       nfin, b_in.dev(), b_nrm.dev(), colors ? b_col.dev() : nullptr, n,
                       b_q.dev(), m, V, G, K, radius, trunc, nullptr, nullptr, b_value.dev(),
                       b_count.dev(), colors ? b_color.dev() : nullptr, b_stats.dev());
  }
  HIP_TRY(hipGetLastError());
  if ((st = c->points.mark(6, s))) return st;
  U64 stats[8];
  if (volume) {
    HIP_TRY(hipMemcpyAsync(o.tsdf, b_tsdf.dev(), b_tsdf.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(o.weight, b_weight.dev(), b_weight.bytes, hipMemcpyDeviceToHost, s));
  } else {
    HIP_TRY(hipMemcpyAsync(o.value, b_value.dev(), b_value.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(o.count, b_count.dev(), b_count.bytes, hipMemcpyDeviceToHost, s));
    if (colors)
      HIP_TRY(hipMemcpyAsync(o.color, b_color.dev(), b_color.bytes, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipMemcpyAsync(stats, b_stats.dev(), b_stats.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 1; k < 5; ++k)
    if ((st = c->points.read(k, k + 1, k + 2))) return st;

  info->cells = ncell;
  info->largest_cell = static_cast<int64_t>(stats[rsd::kKnnLargest]);
  info->tested = static_cast<int64_t>(stats[rsd::kKnnTested]);
  info->defined = static_cast<int64_t>(stats[rsd::kPtsDefined]);
  info->saturated = static_cast<int64_t>(stats[rsd::kPtsSaturated]);
  return RS_OK;
}

int points_check(const rs_ctx *c, const rs_points_info *info, const double *pts,
                 const double *normals, int64_t n, int32_t k, double radius, double cell) {
  if (!c || !info) return fail(RS_EINVAL, "null pointer");
  if (k < 1 || k > RS_CLOUD_KNN_MAX_K)
    return fail(RS_EINVAL, "k must be in 1..RS_CLOUD_KNN_MAX_K = 64");
  if (n < 0) return fail(RS_EINVAL, "negative size");
  if (n > RS_CLOUD_MAX_POINTS)
    return fail(RS_EINVAL, "more points or queries than RS_CLOUD_MAX_POINTS = 2^28");
  if (n > 0 && (!pts || !normals)) return fail(RS_EINVAL, "null pointer: pts or normals");
  if (!std::isfinite(radius) || !(radius > 0.0))
    return fail(RS_EINVAL, "radius must be finite and > 0");
  if (!std::isfinite(cell) || cell < 0.0)
    return fail(RS_EINVAL, "cell must be finite and >= 0 (0: the default)");
  return RS_OK;
}

}  // namespace

extern "C" int rs_surface_points_volume(rs_ctx *c, const double *pts, const double *normals,
                                        int64_t n, int32_t k, double radius, double trunc,
                                        double cell, const double *origin, double voxel,
                                        int64_t nz, int64_t ny, int64_t nx, float *tsdf,
                                        float *weight, rs_points_info *info) {
  int st = points_check(c, info, pts, normals, n, k, radius, cell);
  if (st) return st;
  if (!origin || !tsdf || !weight) return fail(RS_EINVAL, "null pointer");
  if (!std::isfinite(trunc) || !(trunc > 0.0))
    return fail(RS_EINVAL, "trunc must be finite and > 0");
  if (nx < 1 || ny < 1 || nz < 1 || nx > RS_SURFACE_MAX_SIDE || ny > RS_SURFACE_MAX_SIDE ||
      nz > RS_SURFACE_MAX_SIDE)
    return fail(RS_EINVAL, "each side of the volume must be in 1..RS_SURFACE_MAX_SIDE = 2048");
  if (nx * ny * nz > RS_SURFACE_MAX_NODES)
    return fail(RS_EINVAL, "a volume of more than RS_SURFACE_MAX_NODES = 2^27 nodes");
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]) ||
      !std::isfinite(voxel) || !(voxel > 0.0))
    return fail(RS_EINVAL, "origin and voxel must be finite, voxel > 0");
  const rs_points_info zero = {0, 0, 0, 0, 0};
  *info = zero;
  PtsOut o;
  o.tsdf = tsdf;
  o.weight = weight;
  const int64_t m = nx * ny * nz;
  if (n == 0) {
    points_fill_empty(true, m, o);
    return RS_OK;
  }
  rsd::PtsVolume V;
  for (int a = 0; a < 3; ++a) V.o[a] = origin[a];
  V.voxel = voxel;
  V.n[0] = static_cast<int>(nx);
  V.n[1] = static_cast<int>(ny);
  V.n[2] = static_cast<int>(nz);
  V.b[0] = static_cast<int>(rs::blocks(nx, rsd::kPtsBrickX));
  V.b[1] = static_cast<int>(rs::blocks(ny, rsd::kPtsBrickYZ));
  return points_run(c, pts, normals, nullptr, n, nullptr, m, V, k, radius, trunc, cell, o, info);
}

extern "C" int rs_surface_points_eval(rs_ctx *c, const double *pts, const double *normals,
                                      const double *colors, int64_t n, const double *queries,
                                      int64_t m, int32_t k, double radius, double cell,
                                      double *value, int32_t *count, double *color,
                                      rs_points_info *info) {
  int st = points_check(c, info, pts, normals, n, k, radius, cell);
  if (st) return st;
  if (m < 0) return fail(RS_EINVAL, "negative size");
  if (m > RS_CLOUD_MAX_POINTS)
    return fail(RS_EINVAL, "more points or queries than RS_CLOUD_MAX_POINTS = 2^28");
  if ((colors == nullptr) != (color == nullptr))
    return fail(RS_EINVAL, "colors and color are given together or not at all");
  const rs_points_info zero = {0, 0, 0, 0, 0};
  *info = zero;
  if (m == 0) return RS_OK;
  if (!queries || !value || !count) return fail(RS_EINVAL, "null pointer");
  PtsOut o;
  o.value = value;
  o.count = count;
  o.color = color;
  if (n == 0) {
    points_fill_empty(false, m, o);
    return RS_OK;
  }
  rsd::PtsVolume V = {};
  return points_run(c, pts, normals, colors, n, queries, m, V, k, radius, 1.0, cell, o, info);
}

extern "C" int rs_surface_points_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->points.enable(enable != 0);
  if (st) return st;
  c->points.copy_out(ms);
  return RS_OK;
}
