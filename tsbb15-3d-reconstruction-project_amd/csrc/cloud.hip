// The point-cloud stage on the GPU: what main.py does last (main.py:175-176,
// Tables.get3DPointsColorsAndNormals: a colour and an averaged direction to the cameras per
// point) and the surface normals 3Dvisualization.py attempts on the cloud itself (a fixed-radius
// neighbourhood per point, a plane fit, a sign).  All fp64, plain HIP, one lane per point.
//
// rs_cloud_attributes is one kernel: a lane walks its point's entries in list order.
//
// rs_cloud_normals is a hash grid of cells of side h = radius (1 + 2^-20):
//   k_cloud_min      the minimum corner `lo` of the finite points: per-block minima, then the
//                    same kernel once more over the partial minima
//   k_cloud_key      cell = floor(((p - lo) / radius) (1 - 2^-20)) per axis, 21 bits each in a
//                    63-bit key; the key goes into an open-addressed table (integer atomicCAS)
//                    and the slot's count goes up (integer atomicAdd).  The cells are a shade
//                    larger than radius so that the rounding of (p - lo) / radius -- up to 2^-32
//                    at the far end of the range -- can never put two points that are within
//                    radius of each other two cells apart.  Non-finite points get their outputs
//                    here and take no further part
//   k_cloud_scan*    exclusive scan of the slot counts: every workgroup scans its chunk, one
//                    workgroup scans the chunk sums, every chunk adds its offset
//   k_cloud_scatter  point indices into their cell's segment, in arrival order
//   k_cloud_sort     one lane per slot sorts its segment by point index: from here on nothing
//                    depends on the arrival order or on the slot layout
//   k_cloud_normals  one lane per query, the queries in cell order (the scattered list itself),
//                    so a wave's lanes read the same segments.  The lane looks its 27 cells up,
//                    keeps a cursor per non-empty one in LDS and merges them: every step takes
//                    the smallest point index at any cursor, so the candidates arrive in
//                    ascending j, as the contract in rsamd.h demands.  k, s, S live in
//                    registers; then M, a cyclic Jacobi (the scheme of pnp_minimal.h's sym_jacobi,
//                    which needs the PnP point types around it) and the sign
// Every loop is bounded by construction: a hash probe stops after `capacity` steps (and raises
// a flag), the merge advances one cursor per step, and no lane waits for another workgroup.
// The cost is O(n * 27 * points per cell); a cloud inside one cell is O(n^2) by nature and its
// cell is sorted by a single lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "device_math.h"
#include "host.h"

namespace rsd {

constexpr int kCloudThreads = 256;
constexpr int kCloudMinBlocks = 256;
constexpr int kCloudScanThreads = 1024;
constexpr int kCloudScanItems = 4;
constexpr int kCloudScanChunk = kCloudScanThreads * kCloudScanItems;
constexpr int kCloudWave = 64;
constexpr int kCloudBits = 21;
constexpr unsigned long long kCloudEmpty = ~0ULL;
constexpr double kCloudShrink = 1.0 - 1.0 / 1048576.0;
constexpr int kCloudNone = 0x7fffffff;

// stats words (unsigned long long each)
constexpr int kStatFlags = 0, kStatOccupied = 1, kStatLargest = 2, kStatPairs = 3;
constexpr unsigned long long kFlagRange = 1, kFlagProbe = 2;

__device__ __forceinline__ double cloud_nan() {
  return __longlong_as_double(0x7ff8000000000000LL);
}

__device__ __forceinline__ bool cloud_finite3(const double *p) {
  return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

__device__ __forceinline__ unsigned long long cloud_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

// Per-axis minimum over the points whose three coordinates are finite; +inf where a workgroup
// saw none.  A second launch with one workgroup over the first launch's output finishes it (a
// workgroup's output is a finite point or three +inf, which the filter drops).
__global__ __launch_bounds__(kCloudThreads) void k_cloud_min(const double *pts, int64_t n,
                                                             double *out) {
  __shared__ double lds[3][kCloudThreads / 64];
  double m[3] = {INFINITY, INFINITY, INFINITY};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCloudThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kCloudThreads) {
    const double *p = pts + 3 * i;
    if (cloud_finite3(p)) {
#pragma unroll
      for (int a = 0; a < 3; ++a) m[a] = fmin(m[a], p[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int off = 32; off > 0; off >>= 1) m[a] = fmin(m[a], __shfl_xor(m[a], off));
    if ((threadIdx.x & 63) == 0) lds[a][threadIdx.x >> 6] = m[a];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = lds[threadIdx.x][0];
    for (int w = 1; w < kCloudThreads / 64; ++w) v = fmin(v, lds[threadIdx.x][w]);
    out[3 * static_cast<int64_t>(blockIdx.x) + threadIdx.x] = v;
  }
}

struct CloudGrid {
  unsigned long long *keys;   // cap slots, kCloudEmpty where free
  int32_t *cnt;               // cap + 1: counts, after the scan the offsets and the total
  int32_t *fill;              // cap
  unsigned long long *pkey;   // n: the point's key, kCloudEmpty for a point outside the grid
  int32_t *slot_of;           // n: its slot, -1 outside the grid
  int32_t *cell_pts;          // n: the point indices by cell, ascending within a cell
  unsigned long long *stats;
  unsigned mask;              // cap - 1
};

__global__ __launch_bounds__(kCloudThreads) void k_cloud_key(const double *pts, int64_t n,
                                                             const double *lo, double radius,
                                                             CloudGrid G, double *normals,
                                                             double *evals, int32_t *count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCloudThreads + threadIdx.x;
  if (i >= n) return;
  const double *p = pts + 3 * i;
  G.pkey[i] = kCloudEmpty;
  G.slot_of[i] = -1;
  if (!cloud_finite3(p)) {
    count[i] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = evals[3 * i + a] = cloud_nan();
    return;
  }
  unsigned long long key = 0;
  bool in_range = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double q = (p[a] - lo[a]) / radius;   // >= 0: lo is the minimum of these very points
    if (!(q < static_cast<double>(1 << kCloudBits))) {
      in_range = false;
    } else {
      key |= static_cast<unsigned long long>(q * kCloudShrink) << (kCloudBits * a);
    }
  }
  if (!in_range) {
    atomicOr(&G.stats[kStatFlags], kFlagRange);
    return;
  }
  unsigned h = static_cast<unsigned>(cloud_hash(key)) & G.mask;
  int slot = -1;
  for (unsigned step = 0; step <= G.mask; ++step) {
    const unsigned long long prev = atomicCAS(&G.keys[h], kCloudEmpty, key);
    if (prev == kCloudEmpty || prev == key) {
      slot = static_cast<int>(h);
      break;
    }
    h = (h + 1) & G.mask;
  }
  if (slot < 0) {
    atomicOr(&G.stats[kStatFlags], kFlagProbe);
    return;
  }
  atomicAdd(&G.cnt[slot], 1);
  G.pkey[i] = key;
  G.slot_of[i] = slot;
}

// Exclusive scan in place of the chunk v[at .. at + kCloudScanChunk), clipped to `end`, started
// at `carry`; returns the chunk's sum.  All threads of the workgroup call it together.
__device__ __forceinline__ int cloud_scan_chunk(int32_t *v, int64_t at, int64_t end, int carry,
                                                int *lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = at + static_cast<int64_t>(threadIdx.x) * kCloudScanItems;
  int x[kCloudScanItems], sum = 0;
#pragma unroll
  for (int k = 0; k < kCloudScanItems; ++k) {
    x[k] = base + k < end ? v[base + k] : 0;
    sum += x[k];
  }
  int incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kCloudScanThreads / 64; ++w) {
    if (w < wave) before += lds[w];
    all += lds[w];
  }
  int run = carry + before + incl - sum;
#pragma unroll
  for (int k = 0; k < kCloudScanItems; ++k) {
    if (base + k < end) v[base + k] = run;
    run += x[k];
  }
  __syncthreads();
  return all;
}

// The scan of the slot counts in three launches.  First every workgroup scans its own chunk
// of cnt in place and leaves the chunk's sum ...
__global__ __launch_bounds__(kCloudScanThreads) void k_cloud_scan_chunks(int32_t *cnt, int64_t cap,
                                                                         int32_t *sums) {
  __shared__ int lds[kCloudScanThreads / 64];
  const int total = cloud_scan_chunk(cnt, static_cast<int64_t>(blockIdx.x) * kCloudScanChunk, cap,
                                     0, lds);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ... then one workgroup turns v[0 .. m), the chunk sums, into exclusive offsets in place with
// the total in v[m] ...
__global__ __launch_bounds__(kCloudScanThreads) void k_cloud_scan(int32_t *v, int64_t m) {
  __shared__ int lds[kCloudScanThreads / 64];
  int carry = 0;
  for (int64_t at = 0; at < m; at += kCloudScanChunk)
    carry += cloud_scan_chunk(v, at, m, carry, lds);
  if (threadIdx.x == 0) v[m] = carry;
}

// ... and every chunk adds its offset: cnt[0 .. cap) are the exclusive offsets, cnt[cap] the total.
__global__ __launch_bounds__(kCloudScanThreads) void k_cloud_scan_add(int32_t *cnt, int64_t cap,
                                                                      const int32_t *sums,
                                                                      int nchunks) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kCloudScanChunk +
                       static_cast<int64_t>(threadIdx.x) * kCloudScanItems;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kCloudScanItems; ++k)
    if (base + k < cap) cnt[base + k] += add;
  if (blockIdx.x == 0 && threadIdx.x == 0) cnt[cap] = sums[nchunks];
}

__global__ __launch_bounds__(kCloudThreads) void k_cloud_scatter(int64_t n, CloudGrid G) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kCloudThreads + threadIdx.x;
  if (i >= n) return;
  const int s = G.slot_of[i];
  if (s < 0) return;
  const int at = atomicAdd(&G.fill[s], 1);   // < the slot's count: every point counted once
  G.cell_pts[G.cnt[s] + at] = static_cast<int32_t>(i);
}

// One lane per slot: insertion sort of the slot's segment by point index (the arrival order
// is close to sorted already).  The grid is cap / kCloudThreads workgroups, all lanes live.
__global__ __launch_bounds__(kCloudThreads) void k_cloud_sort(CloudGrid G) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kCloudThreads + threadIdx.x;
  const int lo = G.cnt[s], hi = G.cnt[s + 1];
  int32_t *a = G.cell_pts;
  for (int i = lo + 1; i < hi; ++i) {
    const int32_t v = a[i];
    int j = i;
    while (j > lo && a[j - 1] > v) {
      a[j] = a[j - 1];
      --j;
    }
    a[j] = v;
  }
  int m = hi - lo;
  const int occupied = __popcll(__ballot(m > 0));
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0 && occupied > 0) {
    atomicAdd(&G.stats[kStatOccupied], static_cast<unsigned long long>(occupied));
    atomicMax(&G.stats[kStatLargest], static_cast<unsigned long long>(m));
  }
}

__global__ __launch_bounds__(kCloudWave) void k_cloud_normals(const double *pts,
                                                              const double *orient, int64_t cap,
                                                              CloudGrid G, double r2,
                                                              double *normals, double *evals,
                                                              int32_t *count) {
  // a lane's cursors: column `lane` of each array, touched by that lane only
  __shared__ int s_cur[27][kCloudWave], s_end[27][kCloudWave], s_head[27][kCloudWave];
  const int lane = threadIdx.x;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kCloudWave + lane;
  const bool active = t < G.cnt[cap];
  int64_t i = 0;
  double p[3] = {0.0, 0.0, 0.0};
  int nseg = 0;
  if (active) {
    i = G.cell_pts[t];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = pts[3 * i + a];
    const unsigned long long key = G.pkey[i];
    const int cmask = (1 << kCloudBits) - 1;
    const int c0 = static_cast<int>(key) & cmask;
    const int c1 = static_cast<int>(key >> kCloudBits) & cmask;
    const int c2 = static_cast<int>(key >> (2 * kCloudBits)) & cmask;
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int x = c0 + dx, y = c1 + dy, z = c2 + dz;
          if ((x | y | z) < 0 || x > cmask || y > cmask || z > cmask) continue;
          const unsigned long long nk = static_cast<unsigned long long>(x) |
                                        static_cast<unsigned long long>(y) << kCloudBits |
                                        static_cast<unsigned long long>(z) << (2 * kCloudBits);
          unsigned h = static_cast<unsigned>(cloud_hash(nk)) & G.mask;
          for (unsigned step = 0; step <= G.mask; ++step) {
            const unsigned long long k = G.keys[h];
            if (k == nk) {
              const int b = G.cnt[h], e = G.cnt[h + 1];
              if (e > b) {
                s_cur[nseg][lane] = b;
                s_end[nseg][lane] = e;
                s_head[nseg][lane] = G.cell_pts[b];
                ++nseg;
              }
              break;
            }
            if (k == kCloudEmpty) break;
            h = (h + 1) & G.mask;
          }
        }
  }

  int k = 0;
  unsigned long long tested = 0;
  double s[3] = {0.0, 0.0, 0.0}, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  while (true) {   // one cursor advances per step: at most the 27 segments' lengths in all
    int best = kCloudNone, bc = -1;
    for (int c = 0; c < nseg; ++c) {
      const int h = s_head[c][lane];
      if (h < best) {
        best = h;
        bc = c;
      }
    }
    if (bc < 0) break;
    const double *q = pts + 3 * static_cast<int64_t>(best);
    const double d0 = q[0] - p[0], d1 = q[1] - p[1], d2 = q[2] - p[2];
    ++tested;
    if (d0 * d0 + d1 * d1 + d2 * d2 <= r2) {
      ++k;
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
    const int cur = s_cur[bc][lane] + 1;
    s_cur[bc][lane] = cur;
    s_head[bc][lane] = cur < s_end[bc][lane] ? G.cell_pts[cur] : kCloudNone;
  }

  for (int off = 32; off > 0; off >>= 1) tested += __shfl_xor(tested, off);
  if (lane == 0 && tested > 0) atomicAdd(&G.stats[kStatPairs], tested);
  if (!active) return;

  count[i] = k;
  double nrm[3] = {cloud_nan(), cloud_nan(), cloud_nan()};
  double ev[3] = {cloud_nan(), cloud_nan(), cloud_nan()};
  if (k >= 3) {
    const double ik = 1.0 / static_cast<double>(k);
    const double m0 = s[0] * ik, m1 = s[1] * ik, m2 = s[2] * ik;
    double A[9], V[9];
    A[0] = S[0] * ik - m0 * m0;
    A[1] = A[3] = S[1] * ik - m0 * m1;
    A[2] = A[6] = S[2] * ik - m0 * m2;
    A[4] = S[3] * ik - m1 * m1;
    A[5] = A[7] = S[4] * ik - m1 * m2;
    A[8] = S[5] * ik - m2 * m2;
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
    if (o && cloud_finite3(o) && (o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0)) {
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

// One lane per point: its entries [off[j], off[j + 1]) in list order.
__global__ __launch_bounds__(kCloudThreads) void k_cloud_attr(
    const double *cams, const double *pts, const int32_t *off, const int32_t *entry_obs,
    const int32_t *obs_view, const double *obs_color, int64_t nP, double *colors,
    double *normals) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kCloudThreads + threadIdx.x;
  if (j >= nP) return;
  const int lo = off[j], hi = off[j + 1];
  const double X[3] = {pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]};
  double col[3] = {0.0, 0.0, 0.0}, dir[3] = {0.0, 0.0, 0.0};
  for (int e = lo; e < hi; ++e) {
    const int64_t o = entry_obs[e];
    const double *c = cams + 12 * static_cast<int64_t>(obs_view[o]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double centre = -1.0 * (c[a] * c[3] + c[4 + a] * c[7] + c[8 + a] * c[11]);
      dir[a] += centre - X[a];
      col[a] += obs_color[3 * o + a];
    }
  }
  const double m = static_cast<double>(hi - lo);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    colors[3 * j + a] = hi > lo ? col[a] / m / 255.0 : cloud_nan();
    normals[3 * j + a] = hi > lo ? dir[a] / m : cloud_nan();
  }
}

}  // namespace rsd

using rs::blocks;

extern "C" int rs_cloud_attributes(rs_ctx *c, const double *cams, int64_t nC, const double *pts,
                                   int64_t nP, const int32_t *entry_point,
                                   const int32_t *entry_obs, int64_t m, const int32_t *obs_view,
                                   const double *obs_color, int64_t nObs, double *colors,
                                   double *normals) {
  if (!c || nP < 0 || m < 0 || nC < 0 || nObs < 0) return fail(RS_EINVAL, "bad sizes");
  if (nP > RS_CLOUD_MAX_POINTS || m > (1LL << 30) || nObs > (1LL << 30))
    return fail(RS_EINVAL, "the cloud is larger than RS_CLOUD_MAX_POINTS");
  if (nP == 0) {
    if (m > 0) return fail(RS_EINVAL, "an entry names a point of an empty cloud");
    return RS_OK;
  }
  if (!pts || !colors || !normals) return fail(RS_EINVAL, "null pointer");
  if (m > 0 && (!cams || !entry_point || !entry_obs || !obs_view || !obs_color))
    return fail(RS_EINVAL, "null pointer");
  if (m > 0 && nC < 1) return fail(RS_EINVAL, "entries need at least one camera");
  for (int64_t o = 0; o < nObs && m > 0; ++o)
    if (obs_view[o] < 0 || obs_view[o] >= nC) return fail(RS_EINVAL, "obs_view out of range");

  // [cams | pts | obs_color | off | entry_obs | obs_view] go up, [colors | normals] come down
  rs::Layout L;
  const auto b_cams = L.add<double>(12 * nC), b_pts = L.add<double>(3 * nP);
  const auto b_color = L.add<double>(3 * nObs);
  const auto b_off = L.add<int32_t>(nP + 1), b_eobs = L.add<int32_t>(m), b_oview = L.add<int32_t>(nObs);
  const auto b_colors = L.add<double>(3 * nP), b_normals = L.add<double>(3 * nP);
  HIP_TRY(hipSetDevice(c->device));
  int st = L.bind(c, 256, L.total() + 256);
  if (st) return st;
  int32_t *off = b_off.host();
  std::memset(off, 0, b_off.bytes);
  for (int64_t e = 0; e < m; ++e) {
    const int32_t j = entry_point[e];
    if (j < 0 || j >= nP) return fail(RS_EINVAL, "entry_point out of range");
    if (e > 0 && j < entry_point[e - 1])
      return fail(RS_EINVAL, "entry_point must be grouped by point, non-decreasing");
    if (entry_obs[e] < 0 || entry_obs[e] >= nObs) return fail(RS_EINVAL, "entry_obs out of range");
    ++off[j + 1];
  }
  for (int64_t j = 0; j < nP; ++j) off[j + 1] += off[j];
  if (m > 0) {
    std::memcpy(b_cams.host(), cams, b_cams.bytes);
    std::memcpy(b_color.host(), obs_color, b_color.bytes);
    std::memcpy(b_eobs.host(), entry_obs, b_eobs.bytes);
    std::memcpy(b_oview.host(), obs_view, b_oview.bytes);
  }
  std::memcpy(b_pts.host(), pts, b_pts.bytes);

  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(L.dev(), L.host(), L.upto(b_colors), hipMemcpyHostToDevice, s));
  if ((st = c->cloud.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_cloud_attr, dim3(blocks(nP, rsd::kCloudThreads)),
                     dim3(rsd::kCloudThreads), 0, s, b_cams.dev(), b_pts.dev(), b_off.dev(),
                     b_eobs.dev(), b_oview.dev(), b_color.dev(), nP, b_colors.dev(),
                     b_normals.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->cloud.mark(1, s))) return st;
  HIP_TRY(hipMemcpyAsync(b_colors.host(), b_colors.dev(), L.from(b_colors), hipMemcpyDeviceToHost,
                         s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->cloud.read(4, 0, 1))) return st;
  std::memcpy(colors, b_colors.host(), b_colors.bytes);
  std::memcpy(normals, b_normals.host(), b_normals.bytes);
  return RS_OK;
}

extern "C" int rs_cloud_normals(rs_ctx *c, const double *pts, int64_t n, double radius,
                                const double *orient, double *normals, int32_t *count,
                                double *evals, rs_cloud_info *info) {
  if (!c || !info) return fail(RS_EINVAL, "null pointer");
  if (!std::isfinite(radius) || !(radius > 0.0))
    return fail(RS_EINVAL, "radius must be finite and positive");
  if (n < 0 || n > RS_CLOUD_MAX_POINTS)
    return fail(RS_EINVAL, "the cloud is larger than RS_CLOUD_MAX_POINTS");
  const rs_cloud_info zero = {0, 0, 0, 0, 0};
  *info = zero;
  if (n == 0) return RS_OK;
  if (!pts || !normals || !count || !evals) return fail(RS_EINVAL, "null pointer");

  int64_t cap = 1024;
  while (cap < 2 * n) cap *= 2;
  const int nb = static_cast<int>(std::min<int64_t>(rsd::kCloudMinBlocks,
                                                    (n + rsd::kCloudThreads - 1) /
                                                        rsd::kCloudThreads));
  const int nchunks = static_cast<int>((cap + rsd::kCloudScanChunk - 1) / rsd::kCloudScanChunk);
  using U64 = unsigned long long;
  // [pts | orient] go up, [normals | evals | count | stats] come down, the rest is the grid
  rs::Layout L;
  const auto b_pts = L.add<double>(3 * n), b_orient = L.add<double>(orient ? 3 * n : 0);
  const auto b_normals = L.add<double>(3 * n), b_evals = L.add<double>(3 * n);
  const auto b_count = L.add<int32_t>(n);
  const auto b_stats = L.add<U64>(8);
  const auto b_pkey = L.add<U64>(n);
  const auto b_slot_of = L.add<int32_t>(n), b_cell_pts = L.add<int32_t>(n);
  const auto b_keys = L.add<U64>(cap);
  const auto b_cnt = L.add<int32_t>(cap + 1), b_fill = L.add<int32_t>(cap);
  const auto b_part = L.add<double>(3 * nb), b_lo = L.add<double>(3);
  const auto b_sums = L.add<int32_t>(nchunks + 1);
  HIP_TRY(hipSetDevice(c->device));
  int st = L.bind(c, 256, L.upto(b_pkey) + 256);  // the pinned mirror ends with stats
  if (st) return st;
  std::memcpy(b_pts.host(), pts, b_pts.bytes);
  if (orient) std::memcpy(b_orient.host(), orient, b_orient.bytes);

  const double *d_pts = b_pts.dev();
  const double *d_orient = orient ? b_orient.dev() : nullptr;
  double *d_normals = b_normals.dev(), *d_evals = b_evals.dev();
  int32_t *d_count = b_count.dev();
  double *d_part = b_part.dev(), *d_lo = b_lo.dev();
  int32_t *d_sums = b_sums.dev();
  rsd::CloudGrid G;
  G.stats = b_stats.dev();
  G.pkey = b_pkey.dev();
  G.slot_of = b_slot_of.dev();
  G.cell_pts = b_cell_pts.dev();
  G.keys = b_keys.dev();
  G.cnt = b_cnt.dev();
  G.fill = b_fill.dev();
  G.mask = static_cast<unsigned>(cap - 1);

  hipStream_t s = c->stream;
  const dim3 blk(rsd::kCloudThreads);
  HIP_TRY(hipMemcpyAsync(L.dev(), L.host(), L.upto(b_normals), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(b_stats.dev(), 0, b_stats.bytes, s));
  HIP_TRY(hipMemsetAsync(b_keys.dev(), 0xff, b_keys.bytes, s));
  HIP_TRY(hipMemsetAsync(b_cnt.dev(), 0, L.span(b_cnt, b_part), s));  // cnt and fill
  if ((st = c->cloud.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_cloud_min, dim3(nb), blk, 0, s, d_pts, n, d_part);
  hipLaunchKernelGGL(rsd::k_cloud_min, dim3(1), blk, 0, s, d_part, static_cast<int64_t>(nb),
                     d_lo);
  hipLaunchKernelGGL(rsd::k_cloud_key, dim3(blocks(n, rsd::kCloudThreads)), blk, 0, s, d_pts, n,
                     d_lo, radius, G, d_normals, d_evals, d_count);
  if ((st = c->cloud.mark(1, s))) return st;
  const dim3 sblk(rsd::kCloudScanThreads);
  hipLaunchKernelGGL(rsd::k_cloud_scan_chunks, dim3(nchunks), sblk, 0, s, G.cnt, cap, d_sums);
  hipLaunchKernelGGL(rsd::k_cloud_scan, dim3(1), sblk, 0, s, d_sums,
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_cloud_scan_add, dim3(nchunks), sblk, 0, s, G.cnt, cap, d_sums,
                     nchunks);
  if ((st = c->cloud.mark(2, s))) return st;
  hipLaunchKernelGGL(rsd::k_cloud_scatter, dim3(blocks(n, rsd::kCloudThreads)), blk, 0, s, n, G);
  hipLaunchKernelGGL(rsd::k_cloud_sort, dim3(static_cast<unsigned>(cap / rsd::kCloudThreads)),
                     blk, 0, s, G);
  if ((st = c->cloud.mark(3, s))) return st;
  hipLaunchKernelGGL(rsd::k_cloud_normals, dim3(blocks(n, rsd::kCloudWave)),
                     dim3(rsd::kCloudWave), 0, s, d_pts, d_orient, cap, G, radius * radius,
                     d_normals, d_evals, d_count);
  HIP_TRY(hipGetLastError());
  if ((st = c->cloud.mark(4, s))) return st;
  HIP_TRY(hipMemcpyAsync(b_normals.host(), b_normals.dev(), L.span(b_normals, b_pkey),
                         hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 4; ++k)
    if ((st = c->cloud.read(k, k, k + 1))) return st;

  const U64 *stats = b_stats.host();
  if (stats[rsd::kStatFlags] & rsd::kFlagRange)
    return fail(RS_EINVAL,
                "the cloud is too wide for this radius: (p - lo) / radius must stay below "
                "2^21 = 2097152 on every axis (lo: the minimum corner of the finite points)");
  if (stats[rsd::kStatFlags] & rsd::kFlagProbe)
    return fail(RS_EDEVICE, "the cell table overflowed (a hash probe ran its whole capacity)");
  std::memcpy(normals, b_normals.host(), b_normals.bytes);
  std::memcpy(evals, b_evals.host(), b_evals.bytes);
  std::memcpy(count, b_count.host(), b_count.bytes);
  rs_cloud_info r = zero;
  r.cells_occupied = static_cast<int64_t>(stats[rsd::kStatOccupied]);
  r.largest_cell = static_cast<int64_t>(stats[rsd::kStatLargest]);
  r.pairs_tested = static_cast<int64_t>(stats[rsd::kStatPairs]);
  for (int64_t i = 0; i < n; ++i) {
    r.neighbours_found += count[i];
    r.rows_not_ok += count[i] < 3 ? 1 : 0;
  }
  *info = r;
  return RS_OK;
}

extern "C" int rs_cloud_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->cloud.enable(enable != 0);
  if (st) return st;
  c->cloud.copy_out(ms);
  return RS_OK;
}
