// Global registration on the GPU: descriptors over the k-NN lists of cloud_knn.hip
// (rs_cloud_fpfh's two kernels; the entry point stands beside knn_run in cloud_knn.hip),
// brute-force descriptor matching (rs_feature_match) and a RANSAC over the similarities of three
// correspondences (rs_sim3_ransac).  The definitions stand in include/rsamd.h ("Global
// registration"); tests/global_ref.py restates them in numpy.  All fp64 without contraction, only
// + - * /, sqrt, floor, min, max and comparisons, every sum in the header's order: the outputs are
// compared with the restatement bit for bit.
//
//   k_fpfh_spfh      one lane per point, one wave per workgroup: the 33 counts of the point's
//                    simplified histogram live in the lane's column of LDS (bin b at [b * 64]),
//                    because the bin is a run-time index and 33 counters in registers would go
//                    to scratch; only that lane touches the column, so there is no barrier and
//                    no atomic.  A wave per point was not chosen: a list has at most 63 entries
//                    and a lane's work per entry is 60 flops, so a wave would idle on short
//                    lists and need cross-lane traffic for integer adds a lane does in place
//   k_fpfh_sum       one lane per point walks its list again and adds the neighbours' integer
//                    histograms, weighted, in list order into 33 accumulators in registers
//                    (static indices); it reads integer histograms only and has no atomic
//   k_feature_match  one lane per row of fa, the row in DP registers (D padded with zeros to the
//                    next of 8, 16, 36, 64: a term 0 * 0 adds +0.0 to a sum that is not negative
//                    and changes no bit), fb through LDS in tiles of RS_FEATURE_MATCH_TILE rows
//                    that every lane reads at the same address (broadcast)
//   k_sim3_solve     one lane per hypothesis: sample, gates, closed form; a survivor takes the
//                    next slot of the chunk's compact list through an integer counter (the
//                    order of the list is arbitrary; nothing that is returned depends on it)
//   k_sim3_count     one lane per survivor, its model in registers, a segment of the
//                    correspondences read at wave-uniform addresses; integer atomicAdd of the
//                    segment's count
//   k_sim3_gather    the models of the slots the host picked
// Every global index is bounded: a sample index by M (floyd_sample), a list entry is checked
// against n before it is used, a slot against the capacity of the compact list, a tile row
// against m, a histogram bin is clamped to 0..10.  Every loop is bounded by k, D, m, M or a
// constant; no lane waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "device_math.h"
#include "host.h"

namespace rsd {

constexpr int kGlbThreads = 256;
constexpr int kGlbWave = 64;
constexpr int kFpfhBins = RS_FPFH_BINS;
constexpr int kMatchTile = RS_FEATURE_MATCH_TILE;
constexpr int kSimSegment = 1024;   // correspondences per count workgroup
// stats words (unsigned long long each): passed gate 1..5, then the survivors' counter
constexpr int kSimSurvivors = 5;

__device__ __forceinline__ double glb_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ bool glb_finite3(const double *p) {
  return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

__device__ __forceinline__ double glb_dot(const double *a, const double *b) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ void glb_cross(const double *a, const double *b, double *c) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// 0 unless floor(q) >= 0 (a NaN), 10 above 10
__device__ __forceinline__ int fpfh_bin(double q) {
  const double f = floor(q);
  return !(f >= 0.0) ? 0 : (f > 10.0 ? 10 : static_cast<int>(f));
}

// the entry of the row of point i that is dropped: the one that names i, else the last
__device__ __forceinline__ int fpfh_drop(const int32_t *row, int c, int64_t i) {
  for (int e = 0; e < c; ++e)
    if (row[e] == i) return e;
  return c - 1;
}

__global__ __launch_bounds__(kGlbWave) void k_fpfh_spfh(const double *pts, const double *nrm,
                                                        int64_t n, int rows, const int32_t *idx,
                                                        const double *d2, const int32_t *count,
                                                        int32_t *spfh, int32_t *pairs) {
#pragma clang fp contract(off)
  __shared__ int s_hist[kFpfhBins * kGlbWave];
  const int lane = threadIdx.x;
  int *h = s_hist + lane;   // bin b at h[b * 64]
  for (int b = 0; b < kFpfhBins; ++b) h[b * kGlbWave] = 0;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGlbWave + lane;
  if (i >= n) return;
  int ci = 0;
  const double u[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
  const int c = min(count[i], rows);
  if (c > 0 && glb_finite3(u)) {
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    const int32_t *row = idx + i * rows;
    const int drop = fpfh_drop(row, c, i);
    for (int e = 0; e < c; ++e) {
      if (e == drop) continue;
      const int64_t j = row[e];
      if (j < 0 || j >= n) continue;   // never: the list holds point indices
      const double q = d2[i * rows + e];
      if (!(q > 0.0)) continue;
      const double nj[3] = {nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2]};
      if (!glb_finite3(nj)) continue;
      const double d[3] = {pts[3 * j] - p[0], pts[3 * j + 1] - p[1], pts[3 * j + 2] - p[2]};
      double cr[3], v[3], w[3];
      glb_cross(d, u, cr);
      const double cc = glb_dot(cr, cr);
      if (!(cc > 0.0)) continue;
      const double len = sqrt(cc);
#pragma unroll
      for (int a = 0; a < 3; ++a) v[a] = cr[a] / len;
      glb_cross(u, v, w);
      const double f1 = glb_dot(v, nj);
      const double f2 = glb_dot(u, d) / sqrt(q);
      const double x = glb_dot(u, nj), y = glb_dot(w, nj);
      const double den = fabs(x) + fabs(y);
      double ang = 0.0;
      if (den > 0.0) {
        const double r = y / den;
        ang = x >= 0.0 ? 1.0 + r : (y >= 0.0 ? 3.0 - r : (-1.0 - r) + 4.0);
      }
      h[fpfh_bin((f1 + 1.0) * 5.5) * kGlbWave] += 1;
      h[(11 + fpfh_bin((f2 + 1.0) * 5.5)) * kGlbWave] += 1;
      h[(22 + fpfh_bin(ang * 2.75)) * kGlbWave] += 1;
      ++ci;
    }
  }
  for (int b = 0; b < kFpfhBins; ++b) spfh[i * kFpfhBins + b] = h[b * kGlbWave];
  pairs[i] = ci;
}

__global__ __launch_bounds__(kGlbThreads) void k_fpfh_sum(int64_t n, int rows, const int32_t *idx,
                                                          const double *d2, const int32_t *count,
                                                          const int32_t *spfh,
                                                          const int32_t *pairs, double *out) {
#pragma clang fp contract(off)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGlbThreads + threadIdx.x;
  if (i >= n) return;
  double A[kFpfhBins], W = 0.0;
#pragma unroll
  for (int b = 0; b < kFpfhBins; ++b) A[b] = 0.0;
  bool any = false;
  const int c = min(count[i], rows), ci = pairs[i];
  if (c > 0 && ci > 0) {
    const int32_t *row = idx + i * rows;
    const int drop = fpfh_drop(row, c, i);
    for (int e = 0; e < c; ++e) {
      if (e == drop) continue;
      const int64_t j = row[e];
      if (j < 0 || j >= n) continue;   // never: the list holds point indices
      const double q = d2[i * rows + e];
      if (!(q > 0.0)) continue;
      const int cj = pairs[j];
      if (cj <= 0) continue;
      const double w = 1.0 / sqrt(q), dc = static_cast<double>(cj);
      const int32_t *hj = spfh + j * kFpfhBins;
#pragma unroll
      for (int b = 0; b < kFpfhBins; ++b) A[b] += (w * static_cast<double>(hj[b])) / dc;
      W += w;
      any = true;
    }
  }
  const double di = static_cast<double>(ci);
#pragma unroll
  for (int b = 0; b < kFpfhBins; ++b)
    out[i * kFpfhBins + b] =
        any ? static_cast<double>(spfh[i * kFpfhBins + b]) / di + A[b] / W : glb_nan();
}

template <int DP>
__global__ __launch_bounds__(kGlbThreads) void k_feature_match(const double *fa, int64_t n,
                                                               const double *fb, int64_t m, int D,
                                                               int32_t *idx, double *d2) {
#pragma clang fp contract(off)
  __shared__ double s_tile[kMatchTile * DP];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGlbThreads + threadIdx.x;
  double a[DP];
#pragma unroll
  for (int c = 0; c < DP; ++c) a[c] = (i < n && c < D) ? fa[i * D + c] : 0.0;
  double best = INFINITY;
  int bj = -1;
  for (int64_t j0 = 0; j0 < m; j0 += kMatchTile) {
    const int rows = static_cast<int>(min(static_cast<int64_t>(kMatchTile), m - j0));
    __syncthreads();   // the tile before this one has been read
    for (int t = threadIdx.x; t < rows * DP; t += kGlbThreads) {
      const int r = t / DP, c = t - r * DP;
      s_tile[t] = c < D ? fb[(j0 + r) * D + c] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const double *b = s_tile + r * DP;
      const double e0 = a[0] - b[0];
      double s = e0 * e0;
#pragma unroll
      for (int c = 1; c < DP; ++c) {
        const double e = a[c] - b[c];
        s += e * e;
      }
      if (s < best) {   // a NaN never is; a tie keeps the lower index
        best = s;
        bj = static_cast<int>(j0 + r);
      }
    }
  }
  if (i < n) {
    idx[i] = bj;
    d2[i] = best;
  }
}

struct SimArgs {
  double lo, hi, edge_tol, min_edge;
  int with_scale;
};

// the frame of a triangle, columns x, y, z
__device__ __forceinline__ void sim3_frame(const double *p0, const double *p1, const double *p2,
                                           double *x, double *y, double *z) {
#pragma clang fp contract(off)
  const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const double l1 = sqrt(glb_dot(e1, e1));
  double g[3];
  glb_cross(e1, e2, g);
  const double lg = sqrt(glb_dot(g, g));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    x[a] = e1[a] / l1;
    z[a] = g[a] / lg;
  }
  glb_cross(z, x, y);
}

__device__ __forceinline__ double sim3_dist(const double *p, const double *q) {
#pragma clang fp contract(off)
  const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  return sqrt(glb_dot(d, d));
}

// hypotheses h0 .. h0 + nh - 1; models: 13 rows of `cap` slots; hs: the survivors' hypotheses
__global__ __launch_bounds__(kGlbThreads) void k_sim3_solve(
    const double *__restrict__ src, const double *__restrict__ dst, int M, uint64_t seed,
    uint64_t h0, int64_t nh, SimArgs A, double *__restrict__ models, int64_t *__restrict__ hs,
    int64_t cap, unsigned long long *stats) {
#pragma clang fp contract(off)
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kGlbThreads + threadIdx.x;
  const bool active = k < nh;
  const uint64_t h = h0 + static_cast<uint64_t>(active ? k : 0);
  int id[3];
  floyd_sample<3>(seed, h, M, id);   // indices in [0, M)
  double a[3][3], b[3][3];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      a[q][r] = src[3 * static_cast<int64_t>(id[q]) + r];
      b[q][r] = dst[3 * static_cast<int64_t>(id[q]) + r];
    }
  auto same = [](const double *p, const double *q) {
    return p[0] == q[0] && p[1] == q[1] && p[2] == q[2];
  };
  const bool g1 = active && !same(b[0], b[1]) && !same(b[0], b[2]) && !same(b[1], b[2]);
  const double la[3] = {sim3_dist(a[0], a[1]), sim3_dist(a[0], a[2]), sim3_dist(a[1], a[2])};
  const double lb[3] = {sim3_dist(b[0], b[1]), sim3_dist(b[0], b[2]), sim3_dist(b[1], b[2])};
  const bool g2 = g1 && la[0] > A.min_edge && la[1] > A.min_edge && la[2] > A.min_edge;
  const double r[3] = {lb[0] / la[0], lb[1] / la[1], lb[2] / la[2]};
  const double up = 1.0 + A.edge_tol;
  const double rmax = fmax(fmax(r[0], r[1]), r[2]), rmin = fmin(fmin(r[0], r[1]), r[2]);
  // fmax and fmin drop a NaN: every ratio is compared on its own as well
  bool g3 = g2 && r[0] == r[0] && r[1] == r[1] && r[2] == r[2] && rmax <= up * rmin;
  if (!A.with_scale) {
    const double dn = 1.0 / up;
#pragma unroll
    for (int e = 0; e < 3; ++e) g3 = g3 && r[e] >= dn && r[e] <= up;
  }
  double ca[3], cb[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    ca[q] = ((a[0][q] + a[1][q]) + a[2][q]) / 3.0;
    cb[q] = ((b[0][q] + b[1][q]) + b[2][q]) / 3.0;
  }
  double sa[3], sb[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double da[3] = {a[q][0] - ca[0], a[q][1] - ca[1], a[q][2] - ca[2]};
    const double db[3] = {b[q][0] - cb[0], b[q][1] - cb[1], b[q][2] - cb[2]};
    sa[q] = glb_dot(da, da);
    sb[q] = glb_dot(db, db);
  }
  const double s =
      A.with_scale ? sqrt((sb[0] + sb[1]) + sb[2]) / sqrt((sa[0] + sa[1]) + sa[2]) : 1.0;
  const bool g4 = g3 && s >= A.lo && s <= A.hi;
  double xa[3], ya[3], za[3], xb[3], yb[3], zb[3], m[13];
  sim3_frame(a[0], a[1], a[2], xa, ya, za);
  sim3_frame(b[0], b[1], b[2], xb, yb, zb);
  m[0] = s;
  bool fin = isfinite(s);
#pragma unroll
  for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[1 + 3 * rr + c] = (xb[rr] * xa[c] + yb[rr] * ya[c]) + zb[rr] * za[c];
      fin = fin && isfinite(m[1 + 3 * rr + c]);
    }
  }
#pragma unroll
  for (int rr = 0; rr < 3; ++rr) {
    m[10 + rr] =
        cb[rr] - s * ((m[1 + 3 * rr] * ca[0] + m[2 + 3 * rr] * ca[1]) + m[3 + 3 * rr] * ca[2]);
    fin = fin && isfinite(m[10 + rr]);
  }
  const bool g5 = g4 && fin;
  const bool g[5] = {g1, g2, g3, g4, g5};
#pragma unroll
  for (int e = 0; e < 5; ++e) {
    const unsigned long long mask = __ballot(g[e]);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&stats[e], static_cast<unsigned long long>(__popcll(mask)));
  }
  if (!g5) return;
  const int64_t slot = static_cast<int64_t>(atomicAdd(&stats[kSimSurvivors], 1ull));
  if (slot >= cap) return;   // never: cap is the number of hypotheses of the chunk
#pragma unroll
  for (int q = 0; q < 13; ++q) models[q * cap + slot] = m[q];
  hs[slot] = static_cast<int64_t>(h);
}

// grid (survivors / 256, segments of the correspondences); counts zeroed before
__global__ __launch_bounds__(kGlbThreads) void k_sim3_count(
    const double *__restrict__ src, const double *__restrict__ dst, int M,
    const double *__restrict__ models, int64_t cap, int64_t S, double thr2,
    int32_t *__restrict__ counts) {
#pragma clang fp contract(off)
  const int64_t slot = static_cast<int64_t>(blockIdx.x) * kGlbThreads + threadIdx.x;
  const int64_t sl = slot < S ? slot : S - 1;   // S >= 1
  double m[13];
#pragma unroll
  for (int q = 0; q < 13; ++q) m[q] = models[q * cap + sl];
  const int i0 = blockIdx.y * kSimSegment, i1 = min(M, i0 + kSimSegment);
  int cnt = 0;
  for (int i = i0; i < i1; ++i) {   // wave-uniform addresses
    const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
    double d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      d[r] = (m[0] * ((m[1 + 3 * r] * x + m[2 + 3 * r] * y) + m[3 + 3 * r] * z) + m[10 + r]) -
             dst[3 * i + r];
    cnt += glb_dot(d, d) <= thr2 ? 1 : 0;
  }
  if (slot < S && cnt > 0) atomicAdd(&counts[slot], cnt);
}

__global__ __launch_bounds__(kGlbWave) void k_sim3_gather(const double *models, int64_t cap,
                                                          int64_t S, const int32_t *sel, int nsel,
                                                          double *out) {
  const int t = blockIdx.x * kGlbWave + threadIdx.x;
  if (t >= nsel) return;
  const int64_t slot = sel[t];
  if (slot < 0 || slot >= S) return;   // never: the host picked among the S survivors
  for (int q = 0; q < 13; ++q) out[13 * t + q] = models[q * cap + slot];
}

}  // namespace rsd

static_assert(RS_GLOBAL_TIMING_SLOTS == 6, "spfh, fpfh, match, solve, count, gather");
static_assert(sizeof(rs_sim3_candidate) == 120, "rs_sim3_candidate");
static_assert(sizeof(rs_sim3_info) == 64, "rs_sim3_info");
static_assert(RS_FEATURE_MATCH_TILE * RS_FEATURE_MATCH_MAX_D * sizeof(double) <= 65536,
              "the tile fits the LDS of a workgroup");

namespace rs {

// events of c->global: 0..2 the descriptor kernels, 3..4 the match, 5..8 a chunk of the RANSAC
void fpfh_launch(rs_ctx *c, const double *pts, const double *normals, int64_t n, int rows,
                 const int32_t *idx, const double *d2, const int32_t *count, int32_t *spfh,
                 int32_t *pairs, double *out) {
  hipStream_t s = c->stream;
  (void)c->global.mark(0, s);
  hipLaunchKernelGGL(rsd::k_fpfh_spfh, dim3(blocks(n, rsd::kGlbWave)), dim3(rsd::kGlbWave), 0, s,
                     pts, normals, n, rows, idx, d2, count, spfh, pairs);
  (void)c->global.mark(1, s);
  hipLaunchKernelGGL(rsd::k_fpfh_sum, dim3(blocks(n, rsd::kGlbThreads)), dim3(rsd::kGlbThreads), 0,
                     s, n, rows, idx, d2, count, spfh, pairs, out);
  (void)c->global.mark(2, s);
}

int fpfh_read_timing(rs_ctx *c) {
  int st = c->global.read(0, 0, 1);
  return st ? st : c->global.read(1, 1, 2);
}

}  // namespace rs

namespace {

template <int DP>
void match_launch(hipStream_t s, const double *fa, int64_t n, const double *fb, int64_t m, int D,
                  int32_t *idx, double *d2) {
  hipLaunchKernelGGL(rsd::k_feature_match<DP>, dim3(rs::blocks(n, rsd::kGlbThreads)),
                     dim3(rsd::kGlbThreads), 0, s, fa, n, fb, m, D, idx, d2);
}

struct SimKey {
  int64_t count, h;
  int32_t slot;
  bool operator<(const SimKey &o) const { return count != o.count ? count > o.count : h < o.h; }
};

}  // namespace

extern "C" int rs_feature_match(rs_ctx *c, const double *fa, int64_t n, const double *fb,
                                int64_t m, int32_t D, int32_t *idx, double *d2) {
  if (!c) return fail(RS_EINVAL, "null pointer");
  if (D < 1 || D > RS_FEATURE_MATCH_MAX_D)
    return fail(RS_EINVAL, "D must be in 1..RS_FEATURE_MATCH_MAX_D = 64");
  if (n < 0 || m < 0) return fail(RS_EINVAL, "negative size");
  if (n > RS_CLOUD_MAX_POINTS || m > RS_CLOUD_MAX_POINTS)
    return fail(RS_EINVAL, "more rows than RS_CLOUD_MAX_POINTS = 2^28");
  if (n == 0) return RS_OK;
  if (!fa || !idx || !d2 || (m > 0 && !fb)) return fail(RS_EINVAL, "null pointer");
  if (m == 0) {
    for (int64_t i = 0; i < n; ++i) {
      idx[i] = -1;
      d2[i] = INFINITY;
    }
    return RS_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t sn = static_cast<size_t>(n), sm = static_cast<size_t>(m), sD = static_cast<size_t>(D);
  rs::Layout L;
  const auto b_fa = L.add<double>(sn * sD), b_fb = L.add<double>(sm * sD);
  const auto b_idx = L.add<int32_t>(sn);
  const auto b_d2 = L.add<double>(sn);
  int st = L.bind(c);
  if (st) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_fa.dev(), fa, b_fa.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_fb.dev(), fb, b_fb.bytes, hipMemcpyHostToDevice, s));
  if ((st = c->global.mark(3, s))) return st;
  if (D <= 8)
    match_launch<8>(s, b_fa.dev(), n, b_fb.dev(), m, D, b_idx.dev(), b_d2.dev());
  else if (D <= 16)
    match_launch<16>(s, b_fa.dev(), n, b_fb.dev(), m, D, b_idx.dev(), b_d2.dev());
  else if (D <= 36)
    match_launch<36>(s, b_fa.dev(), n, b_fb.dev(), m, D, b_idx.dev(), b_d2.dev());
  else
    match_launch<64>(s, b_fa.dev(), n, b_fb.dev(), m, D, b_idx.dev(), b_d2.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->global.mark(4, s))) return st;
  HIP_TRY(hipMemcpyAsync(idx, b_idx.dev(), b_idx.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(d2, b_d2.dev(), b_d2.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return c->global.read(2, 3, 4);
}

extern "C" int rs_sim3_ransac(rs_ctx *c, const double *src, const double *dst, int64_t M,
                              int64_t H, double inlier_dist, uint64_t seed, int32_t with_scale,
                              double scale_lo, double scale_hi, double edge_tol, double min_edge,
                              int32_t candidates, rs_sim3_candidate *out, rs_sim3_info *info) {
  using U64 = unsigned long long;
  if (!c || !src || !dst || !out || !info) return fail(RS_EINVAL, "null pointer");
  if (M < 3 || M > (1LL << 24))
    return fail(RS_EINVAL, "a similarity needs 3 <= M <= 2^24 correspondences");
  if (H < 1 || H > (1LL << 32)) return fail(RS_EINVAL, "H must be in 1..2^32");
  if (candidates < 1 || candidates > RS_SIM3_MAX_CANDIDATES)
    return fail(RS_EINVAL, "candidates must be in 1..RS_SIM3_MAX_CANDIDATES = 1024");
  if (!std::isfinite(inlier_dist) || inlier_dist < 0.0 || !std::isfinite(edge_tol) ||
      edge_tol < 0.0 || !std::isfinite(min_edge) || min_edge < 0.0)
    return fail(RS_EINVAL, "inlier_dist, edge_tol and min_edge must be finite and >= 0");
  if (!(scale_lo >= 0.0) || !(scale_hi >= 0.0))
    return fail(RS_EINVAL, "the scale interval must be >= 0 (+inf is allowed)");
  std::memset(out, 0, sizeof(rs_sim3_candidate) * static_cast<size_t>(candidates));
  std::memset(info, 0, sizeof(*info));
  info->hypotheses = H;
  HIP_TRY(hipSetDevice(c->device));
  const int64_t cap = std::min<int64_t>(H, RS_SIM3_CHUNK);
  const size_t sM = static_cast<size_t>(M), scap = static_cast<size_t>(cap);
  const size_t sC = static_cast<size_t>(candidates);
  rs::Layout L;
  const auto b_src = L.add<double>(3 * sM), b_dst = L.add<double>(3 * sM);
  const auto b_models = L.add<double>(13 * scap);
  const auto b_hs = L.add<int64_t>(scap);
  const auto b_counts = L.add<int32_t>(scap);
  const auto b_stats = L.add<U64>(8);
  const auto b_sel = L.add<int32_t>(sC);
  const auto b_got = L.add<double>(13 * sC);
  int st = L.bind(c);
  if (st) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_src.dev(), src, b_src.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_dst.dev(), dst, b_dst.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(b_stats.dev(), 0, b_stats.bytes, s));
  const rsd::SimArgs A = {scale_lo, scale_hi, edge_tol, min_edge, with_scale != 0};
  const double thr2 = inlier_dist * inlier_dist;
  const unsigned segs = rs::blocks(M, rsd::kSimSegment);
  std::vector<rs_sim3_candidate> best;   // sorted, at most `candidates`
  std::vector<int64_t> hs;
  std::vector<int32_t> counts, sel;
  std::vector<SimKey> keys;
  std::vector<double> got;
  U64 stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c->global.on) c->global.ms[3] = c->global.ms[4] = c->global.ms[5] = 0.0;
  for (int64_t h0 = 0; h0 < H; h0 += cap) {
    const int64_t nh = std::min<int64_t>(cap, H - h0);
    HIP_TRY(hipMemsetAsync(b_stats.dev() + rsd::kSimSurvivors, 0, sizeof(U64), s));
    if ((st = c->global.mark(5, s))) return st;
    hipLaunchKernelGGL(rsd::k_sim3_solve, dim3(rs::blocks(nh, rsd::kGlbThreads)),
                       dim3(rsd::kGlbThreads), 0, s, b_src.dev(), b_dst.dev(),
                       static_cast<int>(M), seed, static_cast<uint64_t>(h0), nh, A,
                       b_models.dev(), b_hs.dev(), cap, b_stats.dev());
    HIP_TRY(hipGetLastError());
    if ((st = c->global.mark(6, s))) return st;
    HIP_TRY(hipMemcpyAsync(stats, b_stats.dev(), b_stats.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((st = c->global.add(3, 5, 6))) return st;
    const int64_t S = std::min<int64_t>(static_cast<int64_t>(stats[rsd::kSimSurvivors]), nh);
    if (S == 0) continue;
    const size_t sS = static_cast<size_t>(S);
    HIP_TRY(hipMemsetAsync(b_counts.dev(), 0, sizeof(int32_t) * sS, s));
    if ((st = c->global.mark(6, s))) return st;
    hipLaunchKernelGGL(rsd::k_sim3_count, dim3(rs::blocks(S, rsd::kGlbThreads), segs),
                       dim3(rsd::kGlbThreads), 0, s, b_src.dev(), b_dst.dev(),
                       static_cast<int>(M), b_models.dev(), cap, S, thr2, b_counts.dev());
    HIP_TRY(hipGetLastError());
    if ((st = c->global.mark(7, s))) return st;
    hs.resize(sS);
    counts.resize(sS);
    HIP_TRY(hipMemcpyAsync(hs.data(), b_hs.dev(), sizeof(int64_t) * sS, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(counts.data(), b_counts.dev(), sizeof(int32_t) * sS,
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((st = c->global.add(4, 6, 7))) return st;
    info->tests += S * M;
    // the chunk's best by (count descending, h ascending), then their models
    keys.resize(sS);
    for (size_t k = 0; k < sS; ++k) keys[k] = {counts[k], hs[k], static_cast<int32_t>(k)};
    const size_t take = std::min(sS, sC);
    std::partial_sort(keys.begin(), keys.begin() + take, keys.end());
    sel.resize(take);
    for (size_t k = 0; k < take; ++k) sel[k] = keys[k].slot;
    got.resize(13 * take);
    HIP_TRY(hipMemcpyAsync(b_sel.dev(), sel.data(), sizeof(int32_t) * take, hipMemcpyHostToDevice,
                           s));
    if ((st = c->global.mark(7, s))) return st;
    hipLaunchKernelGGL(rsd::k_sim3_gather, dim3(rs::blocks(static_cast<int64_t>(take), rsd::kGlbWave)),
                       dim3(rsd::kGlbWave), 0, s, b_models.dev(), cap, S, b_sel.dev(),
                       static_cast<int>(take), b_got.dev());
    HIP_TRY(hipGetLastError());
    if ((st = c->global.mark(8, s))) return st;
    HIP_TRY(hipMemcpyAsync(got.data(), b_got.dev(), sizeof(double) * 13 * take,
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((st = c->global.add(5, 7, 8))) return st;
    for (size_t k = 0; k < take; ++k) {
      rs_sim3_candidate cd;
      cd.h = keys[k].h;
      cd.count = keys[k].count;
      std::memcpy(cd.model, got.data() + 13 * k, sizeof(cd.model));
      best.push_back(cd);
    }
    std::sort(best.begin(), best.end(), [](const rs_sim3_candidate &a, const rs_sim3_candidate &b) {
      return a.count != b.count ? a.count > b.count : a.h < b.h;
    });
    if (best.size() > sC) best.resize(sC);
  }
  for (int e = 0; e < 5; ++e) info->passed[e] = static_cast<int64_t>(stats[e]);
  info->found = static_cast<int64_t>(best.size());
  if (!best.empty()) std::memcpy(out, best.data(), sizeof(rs_sim3_candidate) * best.size());
  return RS_OK;
}

extern "C" int rs_global_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->global.enable(enable != 0);
  if (st) return st;
  c->global.copy_out(ms);
  return RS_OK;
}
