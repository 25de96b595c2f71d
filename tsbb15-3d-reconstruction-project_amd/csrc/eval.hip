// The evaluation stage on the GPU: the exact distance from each of many points to a triangle mesh
// (rs_eval_mesh_distance).  The definitions stand in include/rsamd.h; tests/eval_ref.py restates
// them in numpy.  All fp64, plain HIP, one lane per face while the grid is built and one lane per
// query afterwards.
//
//   k_eval_bin      one lane per face: the nine coordinates packed into `tri` (the query reads a
//                   face with one contiguous 72-byte load, not through its three indices), the
//                   validity test, and cnt[cell] += 1 (integer atomicAdd) for every cell the
//                   face's box overlaps
//   k_eval_scan*    exclusive scan of the cell counts, the three-kernel scheme of cloud.hip: every
//                   workgroup scans its chunk, one workgroup scans the chunk sums, every chunk
//                   adds its offset.  The first kernel also takes the largest count
//   k_eval_scatter  one lane per face: the face index into each of its cells' segments through an
//                   integer atomic cursor, in arrival order
//   k_eval_query    one lane per query, the walk over Chebyshev rings of rsamd.h
// The query keeps the minimum of the pair (d2, face index), so neither the arrival order inside a
// cell, nor the cells' layout, nor `cell` itself can change a bit of the result.
// eval_closest is the one point-triangle routine and has one call site; it, the validity test and
// the cell coordinates are compiled without FMA contraction.  The host runs the validity test and
// the cell ranges as well -- the same functions, subtraction and division only besides the
// contraction-free cross product -- to know the number of registrations before it allocates.
// Every global index is bounded: a vertex is read at a face index the host has checked against nv
// before any launch; a cell index is clamped to the grid where a face computes it and tested
// against the grid where a query does; the scatter writes below the allocated number of entries
// and the query reads a segment only below it; no lane waits for another, and every loop is
// bounded by the grid's dimensions or by a segment's length.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "host.h"

namespace rsd {

constexpr int kEvalThreads = 256;
constexpr int kEvalScanThreads = 1024;
constexpr int kEvalScanItems = 4;
constexpr int kEvalScanChunk = kEvalScanThreads * kEvalScanItems;
constexpr double kEvalShrink = 1.0 - 1.0 / 1048576.0;
constexpr double kEvalFar = 536870912.0;   // 2^29: a query's cell coordinate is clamped to +-this

// stats words (unsigned long long each)
constexpr int kEvalTests = 0, kEvalLargest = 1, kEvalSkipped = 2, kEvalEntries = 3;

struct EvalGrid {
  double lo[3], cell;
  int dim[3];
};

__host__ __device__ inline bool eval_finite(double x) { return x - x == 0.0; }

// a, b, c: three coordinates each
__host__ __device__ inline bool eval_face_valid(const double *a, const double *b,
                                                const double *c) {
#pragma clang fp contract(off)
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && eval_finite(a[k]) && eval_finite(b[k]) && eval_finite(c[k]);
  if (!ok) return false;
  const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
  const double ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
  const double n0 = ab1 * ac2 - ab2 * ac1, n1 = ab2 * ac0 - ab0 * ac2, n2 = ab0 * ac1 - ab1 * ac0;
  return !(n0 == 0.0 && n1 == 0.0 && n2 == 0.0);
}

// floor((x - lo) / cell) clamped to [-limit, limit]; a NaN gives -limit
__host__ __device__ inline double eval_coord(double x, double lo, double cell, double limit) {
#pragma clang fp contract(off)
  const double q = floor((x - lo) / cell);
  return !(q >= -limit) ? -limit : (q > limit ? limit : q);
}

// the cells [c0[k], c1[k]] the box of a valid face overlaps, clamped to the grid
__host__ __device__ inline void eval_face_cells(const EvalGrid &G, const double *a,
                                                const double *b, const double *c, int *c0,
                                                int *c1) {
  for (int k = 0; k < 3; ++k) {
    const double mn = fmin(a[k], fmin(b[k], c[k])), mx = fmax(a[k], fmax(b[k], c[k]));
    const double top = static_cast<double>(G.dim[k] - 1);
    const double q0 = eval_coord(mn, G.lo[k], G.cell, top), q1 = eval_coord(mx, G.lo[k], G.cell, top);
    c0[k] = q0 < 0.0 ? 0 : static_cast<int>(q0);
    c1[k] = q1 < 0.0 ? 0 : static_cast<int>(q1);
  }
}

__device__ __forceinline__ double eval_nan() {
  return __longlong_as_double(0x7ff8000000000000LL);
}

// Ericson's ClosestPtPointTriangle in the order of operations rsamd.h writes down: the closest
// point q of the triangle T = (a, b, c) to p; returns |p - q|^2.
__device__ __forceinline__ double eval_closest(const double *p, const double *T, double *q) {
#pragma clang fp contract(off)
  const double *a = T, *b = T + 3, *c = T + 6;
  const double ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
  const double ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
  const double ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
  const double d1 = ab0 * ap0 + ab1 * ap1 + ab2 * ap2;
  const double d2 = ac0 * ap0 + ac1 * ap1 + ac2 * ap2;
  const double bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
  const double d3 = ab0 * bp0 + ab1 * bp1 + ab2 * bp2;
  const double d4 = ac0 * bp0 + ac1 * bp1 + ac2 * bp2;
  const double cp0 = p[0] - c[0], cp1 = p[1] - c[1], cp2 = p[2] - c[2];
  const double d5 = ab0 * cp0 + ab1 * cp1 + ab2 * cp2;
  const double d6 = ac0 * cp0 + ac1 * cp1 + ac2 * cp2;
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  if (d1 <= 0.0 && d2 <= 0.0) {
    q[0] = a[0], q[1] = a[1], q[2] = a[2];
  } else if (d3 >= 0.0 && d4 <= d3) {
    q[0] = b[0], q[1] = b[1], q[2] = b[2];
  } else if (d6 >= 0.0 && d5 <= d6) {
    q[0] = c[0], q[1] = c[1], q[2] = c[2];
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double t = d1 / (d1 - d3);
    q[0] = a[0] + t * ab0, q[1] = a[1] + t * ab1, q[2] = a[2] + t * ab2;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double t = d2 / (d2 - d6);
    q[0] = a[0] + t * ac0, q[1] = a[1] + t * ac1, q[2] = a[2] + t * ac2;
  } else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
    const double t = e43 / (e43 + e56);
    q[0] = b[0] + t * (c[0] - b[0]), q[1] = b[1] + t * (c[1] - b[1]), q[2] = b[2] + t * (c[2] - b[2]);
  } else {
    const double s = (va + vb) + vc, v = vb / s, w = vc / s;
    q[0] = (a[0] + v * ab0) + w * ac0;
    q[1] = (a[1] + v * ab1) + w * ac1;
    q[2] = (a[2] + v * ab2) + w * ac2;
  }
  const double e0 = p[0] - q[0], e1 = p[1] - q[1], e2 = p[2] - q[2];
  return e0 * e0 + e1 * e1 + e2 * e2;
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_bin(const double *vertices,
                                                           const int32_t *faces, int64_t nf,
                                                           EvalGrid G, double *tri, int32_t *cnt,
                                                           unsigned long long *stats) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kEvalThreads + threadIdx.x;
  if (f >= nf) return;
  double T[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int64_t at = 3 * static_cast<int64_t>(faces[3 * f + i]);
#pragma unroll
    for (int k = 0; k < 3; ++k) tri[9 * f + 3 * i + k] = T[3 * i + k] = vertices[at + k];
  }
  if (!eval_face_valid(T, T + 3, T + 6)) {
    atomicAdd(&stats[kEvalSkipped], 1ull);
    return;
  }
  int c0[3], c1[3];
  eval_face_cells(G, T, T + 3, T + 6, c0, c1);
  for (int z = c0[2]; z <= c1[2]; ++z)
    for (int y = c0[1]; y <= c1[1]; ++y)
      for (int x = c0[0]; x <= c1[0]; ++x)
        atomicAdd(&cnt[(static_cast<int64_t>(z) * G.dim[1] + y) * G.dim[0] + x], 1);
}

// Exclusive scan in place of the chunk v[at .. at + kEvalScanChunk), clipped to `end`, started
// at `carry`; returns the chunk's sum and leaves the largest element in *largest.  All threads
// of the workgroup call it together.
__device__ __forceinline__ int eval_scan_chunk(int32_t *v, int64_t at, int64_t end, int carry,
                                               int *lds, int *largest) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = at + static_cast<int64_t>(threadIdx.x) * kEvalScanItems;
  int x[kEvalScanItems], sum = 0, big = 0;
#pragma unroll
  for (int k = 0; k < kEvalScanItems; ++k) {
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
  for (int w = 0; w < kEvalScanThreads / 64; ++w) {
    if (w < wave) before += lds[w];
    all += lds[w];
  }
  int run = carry + before + incl - sum;
#pragma unroll
  for (int k = 0; k < kEvalScanItems; ++k) {
    if (base + k < end) v[base + k] = run;
    run += x[k];
  }
  __syncthreads();
  *largest = big;   // of this lane's wave
  return all;
}

__global__ __launch_bounds__(kEvalScanThreads) void k_eval_scan_chunks(int32_t *cnt, int64_t ncell,
                                                                       int32_t *sums,
                                                                       unsigned long long *stats) {
  __shared__ int lds[kEvalScanThreads / 64];
  int big;
  const int total = eval_scan_chunk(cnt, static_cast<int64_t>(blockIdx.x) * kEvalScanChunk, ncell,
                                    0, lds, &big);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
  if ((threadIdx.x & 63) == 0 && big > 0)
    atomicMax(&stats[kEvalLargest], static_cast<unsigned long long>(big));
}

// one workgroup turns v[0 .. m), the chunk sums, into exclusive offsets with the total in v[m]
__global__ __launch_bounds__(kEvalScanThreads) void k_eval_scan(int32_t *v, int64_t m) {
  __shared__ int lds[kEvalScanThreads / 64];
  int carry = 0, big;
  for (int64_t at = 0; at < m; at += kEvalScanChunk)
    carry += eval_scan_chunk(v, at, m, carry, lds, &big);
  if (threadIdx.x == 0) v[m] = carry;
}

// every chunk adds its offset: cnt[0 .. ncell) are the exclusive offsets, cnt[ncell] the total
__global__ __launch_bounds__(kEvalScanThreads) void k_eval_scan_add(int32_t *cnt, int64_t ncell,
                                                                    const int32_t *sums,
                                                                    int nchunks,
                                                                    unsigned long long *stats) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kEvalScanChunk +
                       static_cast<int64_t>(threadIdx.x) * kEvalScanItems;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kEvalScanItems; ++k)
    if (base + k < ncell) cnt[base + k] += add;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cnt[ncell] = sums[nchunks];
    stats[kEvalEntries] = static_cast<unsigned long long>(sums[nchunks]);
  }
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_scatter(const double *tri, int64_t nf,
                                                               EvalGrid G, const int32_t *cnt,
                                                               int32_t *fill, int32_t *ent,
                                                               int64_t nent) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kEvalThreads + threadIdx.x;
  if (f >= nf) return;
  double T[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) T[k] = tri[9 * f + k];
  if (!eval_face_valid(T, T + 3, T + 6)) return;
  int c0[3], c1[3];
  eval_face_cells(G, T, T + 3, T + 6, c0, c1);
  for (int z = c0[2]; z <= c1[2]; ++z)
    for (int y = c0[1]; y <= c1[1]; ++y)
      for (int x = c0[0]; x <= c1[0]; ++x) {
        const int64_t cell = (static_cast<int64_t>(z) * G.dim[1] + y) * G.dim[0] + x;
        // below the cell's count: the bin kernel counted this very registration
        const int64_t at = static_cast<int64_t>(cnt[cell]) + atomicAdd(&fill[cell], 1);
        if (at < nent) ent[at] = static_cast<int32_t>(f);
      }
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_query(
    const double *pts, int64_t n, EvalGrid G, const int32_t *cnt, const int32_t *ent, int64_t nent,
    const double *tri, double max_dist, double *d2, int32_t *face, double *closest,
    unsigned long long *stats) {
#pragma clang fp contract(off)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kEvalThreads + threadIdx.x;
  const bool active = i < n;
  double p[3] = {0.0, 0.0, 0.0};
  if (active) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = pts[3 * i + k];
  }
  const bool finite = eval_finite(p[0]) && eval_finite(p[1]) && eval_finite(p[2]);
  double best = INFINITY, bq[3] = {eval_nan(), eval_nan(), eval_nan()};
  int bf = -1;
  unsigned long long tested = 0;
  if (active && finite) {
    int c[3], r0 = 0, rmax = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = static_cast<int>(eval_coord(p[k], G.lo[k], G.cell, kEvalFar));
      r0 = max(r0, max(-c[k], c[k] - (G.dim[k] - 1)));   // rings until this axis meets the grid
      rmax = max(rmax, max(c[k], G.dim[k] - 1 - c[k]));  // the last ring that touches it
    }
    // r0 <= rmax, and rmax - r0 is below the grid's largest dimension
    for (int r = r0; r <= rmax; ++r) {
      if (r > 0) {
        const double bound = static_cast<double>(r - 1) * G.cell * kEvalShrink;
        if (best <= bound * bound || bound > max_dist) break;
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
            const int64_t b = cnt[cell], e = min(static_cast<int64_t>(cnt[cell + 1]), nent);
            for (int64_t k = b; k < e; ++k) {
              const int f = ent[k];
              double T[9], q[3];
#pragma unroll
              for (int j = 0; j < 9; ++j) T[j] = tri[9 * static_cast<int64_t>(f) + j];
              const double d = eval_closest(p, T, q);
              ++tested;
              if (d < best || (d == best && f < bf)) {   // false for a NaN
                best = d;
                bf = f;
                bq[0] = q[0], bq[1] = q[1], bq[2] = q[2];
              }
            }
          }
        }
    }
    if (!(best <= max_dist * max_dist)) {
      best = INFINITY;
      bf = -1;
      bq[0] = bq[1] = bq[2] = eval_nan();
    }
  }
  for (int off = 32; off > 0; off >>= 1) tested += __shfl_xor(tested, off);
  if ((threadIdx.x & 63) == 0 && tested > 0) atomicAdd(&stats[kEvalTests], tested);
  if (!active) return;
  d2[i] = finite ? best : eval_nan();
  face[i] = bf;
#pragma unroll
  for (int k = 0; k < 3; ++k) closest[3 * i + k] = bq[k];
}

}  // namespace rsd

static_assert(RS_EVAL_TIMING_SLOTS == 4, "bin, scan, scatter, query");

extern "C" int rs_eval_mesh_distance(rs_ctx *c, const double *pts, int64_t n,
                                     const double *vertices, int64_t nv, const int32_t *faces,
                                     int64_t nf, double max_dist, double cell, double *d2,
                                     int32_t *face, double *closest, rs_eval_info *info) {
  if (!c || !info) return fail(RS_EINVAL, "null pointer");
  if (n < 0 || nv < 0 || nf < 0) return fail(RS_EINVAL, "negative size");
  if (n > RS_EVAL_MAX_POINTS) return fail(RS_EINVAL, "more queries than RS_EVAL_MAX_POINTS");
  if (nv > INT32_MAX || 3 * nf > INT32_MAX)
    return fail(RS_EINVAL, "nv and 3 nf must be in 0..2^31 - 1");
  if (!(max_dist > 0.0)) return fail(RS_EINVAL, "max_dist must be positive (+inf is allowed)");
  if (!std::isfinite(cell) || !(cell > 0.0))
    return fail(RS_EINVAL, "cell must be finite and positive");
  if ((nv > 0 && !vertices) || (nf > 0 && !faces)) return fail(RS_EINVAL, "null pointer");
  for (int64_t k = 0; k < 3 * nf; ++k)
    if (faces[k] < 0 || faces[k] >= nv) return fail(RS_EINVAL, "a face index is out of range");
  const rs_eval_info zero = {{0, 0, 0}, 0, 0, 0, 0, 0};
  *info = zero;
  if (n == 0) return RS_OK;
  if (!pts || !d2 || !face || !closest) return fail(RS_EINVAL, "null pointer");

  // the box of the faces with finite coordinates, then the grid
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t f = 0; f < nf; ++f) {
    const double *a = vertices + 3 * static_cast<int64_t>(faces[3 * f]);
    const double *b = vertices + 3 * static_cast<int64_t>(faces[3 * f + 1]);
    const double *v = vertices + 3 * static_cast<int64_t>(faces[3 * f + 2]);
    bool ok = true;
    for (int k = 0; k < 3; ++k)
      ok = ok && rsd::eval_finite(a[k]) && rsd::eval_finite(b[k]) && rsd::eval_finite(v[k]);
    if (!ok) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::fmin(lo[k], std::fmin(a[k], std::fmin(b[k], v[k])));
      hi[k] = std::fmax(hi[k], std::fmax(a[k], std::fmax(b[k], v[k])));
    }
  }
  rsd::EvalGrid G;
  G.cell = cell;
  double ncell_d = 1.0, mag = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!(lo[k] <= hi[k])) lo[k] = hi[k] = 0.0;   // no finite face
    const double ext = hi[k] - lo[k];
    if (!std::isfinite(ext)) return fail(RS_EINVAL, "the extent of the mesh's box is not finite");
    const double nd = std::floor(ext / cell) + 1.0;
    if (!(nd <= static_cast<double>(RS_EVAL_MAX_CELLS)))
      return fail(RS_EINVAL,
                  "the grid has more than RS_EVAL_MAX_CELLS = 2^24 cells: choose a larger cell");
    G.lo[k] = lo[k];
    G.dim[k] = static_cast<int>(nd);
    ncell_d *= nd;
    mag = std::fmax(mag, std::fmax(std::fabs(lo[k]), std::fabs(hi[k])));
  }
  if (ncell_d > static_cast<double>(RS_EVAL_MAX_CELLS))
    return fail(RS_EINVAL,
                "the grid has more than RS_EVAL_MAX_CELLS = 2^24 cells: choose a larger cell");
  if (cell < mag / 16777216.0)
    return fail(RS_EINVAL,
                "cell is below 2^-24 of the box's largest coordinate magnitude: choose a larger "
                "cell");
  const int64_t ncell = static_cast<int64_t>(G.dim[0]) * G.dim[1] * G.dim[2];
  int64_t entries = 0, skipped = 0;
  for (int64_t f = 0; f < nf; ++f) {
    const double *a = vertices + 3 * static_cast<int64_t>(faces[3 * f]);
    const double *b = vertices + 3 * static_cast<int64_t>(faces[3 * f + 1]);
    const double *v = vertices + 3 * static_cast<int64_t>(faces[3 * f + 2]);
    if (!rsd::eval_face_valid(a, b, v)) {
      ++skipped;
      continue;
    }
    int c0[3], c1[3];
    rsd::eval_face_cells(G, a, b, v, c0, c1);
    entries += static_cast<int64_t>(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
    if (entries > RS_EVAL_MAX_ENTRIES)
      return fail(RS_EINVAL,
                  "more than RS_EVAL_MAX_ENTRIES = 2^27 face-cell registrations: choose a larger "
                  "cell");
  }

  const int nchunks = static_cast<int>((ncell + rsd::kEvalScanChunk - 1) / rsd::kEvalScanChunk);
  using U64 = unsigned long long;
  // [pts | vertices | faces] go up, [d2 | closest | face | stats] come down, the rest is the grid
  rs::Layout L;
  const auto b_pts = L.add<double>(3 * static_cast<size_t>(n));
  const auto b_vert = L.add<double>(3 * static_cast<size_t>(nv));
  const auto b_face = L.add<int32_t>(3 * static_cast<size_t>(nf));
  const auto b_d2 = L.add<double>(static_cast<size_t>(n));
  const auto b_closest = L.add<double>(3 * static_cast<size_t>(n));
  const auto b_best = L.add<int32_t>(static_cast<size_t>(n));
  const auto b_stats = L.add<U64>(8);
  const auto b_tri = L.add<double>(9 * static_cast<size_t>(nf));
  const auto b_cnt = L.add<int32_t>(static_cast<size_t>(ncell) + 1);
  const auto b_fill = L.add<int32_t>(static_cast<size_t>(ncell));
  const auto b_sums = L.add<int32_t>(static_cast<size_t>(nchunks) + 1);
  const auto b_ent = L.add<int32_t>(static_cast<size_t>(entries));
  HIP_TRY(hipSetDevice(c->device));
  int st = L.bind(c);
  if (st) return st;

  hipStream_t s = c->stream;
  const dim3 blk(rsd::kEvalThreads), sblk(rsd::kEvalScanThreads);
  HIP_TRY(hipMemcpyAsync(b_pts.dev(), pts, b_pts.bytes, hipMemcpyHostToDevice, s));
  if (nv) HIP_TRY(hipMemcpyAsync(b_vert.dev(), vertices, b_vert.bytes, hipMemcpyHostToDevice, s));
  if (nf) HIP_TRY(hipMemcpyAsync(b_face.dev(), faces, b_face.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(b_stats.dev(), 0, b_stats.bytes, s));
  HIP_TRY(hipMemsetAsync(b_cnt.dev(), 0, L.span(b_cnt, b_sums), s));   // cnt and fill
  if ((st = c->eval.mark(0, s))) return st;
  if (nf)
    hipLaunchKernelGGL(rsd::k_eval_bin, dim3(rs::blocks(nf, rsd::kEvalThreads)), blk, 0, s,
                       b_vert.dev(), b_face.dev(), nf, G, b_tri.dev(), b_cnt.dev(), b_stats.dev());
  if ((st = c->eval.mark(1, s))) return st;
  hipLaunchKernelGGL(rsd::k_eval_scan_chunks, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), b_stats.dev());
  hipLaunchKernelGGL(rsd::k_eval_scan, dim3(1), sblk, 0, s, b_sums.dev(),
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_eval_scan_add, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), nchunks, b_stats.dev());
  if ((st = c->eval.mark(2, s))) return st;
  if (nf)
    hipLaunchKernelGGL(rsd::k_eval_scatter, dim3(rs::blocks(nf, rsd::kEvalThreads)), blk, 0, s,
                       b_tri.dev(), nf, G, b_cnt.dev(), b_fill.dev(), b_ent.dev(), entries);
  if ((st = c->eval.mark(3, s))) return st;
  hipLaunchKernelGGL(rsd::k_eval_query, dim3(rs::blocks(n, rsd::kEvalThreads)), blk, 0, s,
                     b_pts.dev(), n, G, b_cnt.dev(), b_ent.dev(), entries, b_tri.dev(), max_dist,
                     b_d2.dev(), b_best.dev(), b_closest.dev(), b_stats.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->eval.mark(4, s))) return st;
  U64 stats[8];
  HIP_TRY(hipMemcpyAsync(d2, b_d2.dev(), b_d2.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(closest, b_closest.dev(), b_closest.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(face, b_best.dev(), b_best.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(stats, b_stats.dev(), b_stats.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 4; ++k)
    if ((st = c->eval.read(k, k, k + 1))) return st;
  if (static_cast<int64_t>(stats[rsd::kEvalEntries]) != entries ||
      static_cast<int64_t>(stats[rsd::kEvalSkipped]) != skipped)
    return fail(RS_EDEVICE, "host and device disagree about the faces' validity or cells");

  rs_eval_info r = zero;
  for (int k = 0; k < 3; ++k) r.cells[k] = G.dim[k];
  r.entries = entries;
  r.largest_cell = static_cast<int64_t>(stats[rsd::kEvalLargest]);
  r.tests = static_cast<int64_t>(stats[rsd::kEvalTests]);
  r.faces_skipped = skipped;
  for (int64_t i = 0; i < n; ++i) r.beyond += std::isinf(d2[i]) ? 1 : 0;
  *info = r;
  return RS_OK;
}

extern "C" int rs_eval_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->eval.enable(enable != 0);
  if (st) return st;
  c->eval.copy_out(ms);
  return RS_OK;
}

// ---- registration: a device mesh index and one step of trimmed ICP ------------------------------
// The definitions stand in include/rsamd.h ("Registration"); tests/register_ref.py restates a step.
//   k_reg_transform  one lane per source point: p' = s R p + t
//   k_eval_query     the query above, on p'
//   k_reg_hist       one pass of the radix select: every workgroup counts the bytes of its block's
//                    matched d2 whose higher bytes equal the prefix, in an LDS table of 256 bins,
//                    and merges it into the pass's global table with integer atomics
//   k_reg_pick       one lane: the rank k (first pass), the bin that holds it, the next prefix
//   k_reg_moments    the blocks' partial sums in the header's order, the kept mask and count
//   k_reg_sum        one lane per slot adds the partials in ascending block order; the record
// Every global index is bounded: a point index by n, the allocation of every per-point array; a
// face index by nf before `tri` is read; a bin index is masked to the table; a partial is written
// at block * slots + slot below blocks * RS_EVAL_REG_SLOTS.  Every loop is bounded by the items
// of a block, the number of bins, slots or blocks; no lane waits for another.
namespace rsd {

constexpr int kRegItems = RS_EVAL_REG_BLOCK / kEvalThreads;
constexpr int kRegPasses = 8, kRegBins = 256;
constexpr int kRegPointSlots = 17, kRegPlaneSlots = 37;
constexpr int kRegFold = 8;   // slots folded together through LDS
static_assert(RS_EVAL_REG_BLOCK % kEvalThreads == 0 && kRegBins == kEvalThreads, "lane per bin");
static_assert(kRegPlaneSlots <= RS_EVAL_REG_SLOTS && kRegPointSlots <= RS_EVAL_REG_SLOTS, "slots");

struct RegXform {
  double s, R[9], t[3], o[3];
};

struct RegState {
  unsigned long long prefix, krem, m, k, kept;
  double tau;
};

__global__ __launch_bounds__(kEvalThreads) void k_reg_transform(const double *src, int64_t n,
                                                                RegXform X, double *out) {
#pragma clang fp contract(off)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kEvalThreads + threadIdx.x;
  if (i >= n) return;
  const double x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    out[3 * i + r] = X.s * ((X.R[3 * r] * x + X.R[3 * r + 1] * y) + X.R[3 * r + 2] * z) + X.t[r];
}

__global__ __launch_bounds__(kEvalThreads) void k_reg_hist(const double *d2, const int32_t *face,
                                                           int64_t n, int pass,
                                                           const RegState *st, unsigned *hist) {
  __shared__ unsigned lds[kRegBins];
  lds[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 8 * (kRegPasses - 1 - pass);
  const unsigned long long prefix = st->prefix;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * RS_EVAL_REG_BLOCK + threadIdx.x;
  for (int j = 0; j < kRegItems; ++j) {
    const int64_t i = base + static_cast<int64_t>(j) * kEvalThreads;
    if (i >= n || face[i] < 0) continue;
    const unsigned long long key = static_cast<unsigned long long>(__double_as_longlong(d2[i]));
    // shift + 8 is below 64 wherever pass > 0
    if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8)))
      atomicAdd(&lds[(key >> shift) & (kRegBins - 1)], 1u);
  }
  __syncthreads();
  const unsigned mine = lds[threadIdx.x];
  if (mine) atomicAdd(&hist[pass * kRegBins + (threadIdx.x & (kRegBins - 1))], mine);
}

__global__ void k_reg_pick(int pass, double keep, const unsigned *hist, RegState *st) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned *h = hist + pass * kRegBins;
  if (pass == 0) {
    unsigned long long m = 0;
    for (int b = 0; b < kRegBins; ++b) m += h[b];
    unsigned long long k = 0;
    if (m > 0) {
      const double md = static_cast<double>(m);
      const double prod = keep * md;
      const double kd = ceil(prod - 1e-9);
      k = !(kd >= 1.0) ? 1ull : (kd > md ? m : static_cast<unsigned long long>(kd));
    }
    st->m = m;
    st->k = k;
    st->krem = k;
    st->prefix = 0ull;
  }
  if (st->m == 0) {
    st->tau = eval_nan();
    return;
  }
  const unsigned long long krem = st->krem;
  unsigned long long before = 0;
  int bin = kRegBins - 1;
  for (int b = 0; b < kRegBins; ++b) {
    if (before + h[b] >= krem) {
      bin = b;
      break;
    }
    before += h[b];
  }
  const unsigned long long prefix =
      st->prefix | (static_cast<unsigned long long>(bin) << (8 * (kRegPasses - 1 - pass)));
  st->krem = krem - before;
  st->prefix = prefix;
  if (pass == kRegPasses - 1) st->tau = __longlong_as_double(static_cast<long long>(prefix));
}

// the terms of one kept point, in the header's slots
template <int METRIC>
__device__ __forceinline__ void reg_terms(const double *p, const double *q, double d2,
                                          const double *T, const double *o, double *w) {
#pragma clang fp contract(off)
  const double x0 = p[0] - o[0], x1 = p[1] - o[1], x2 = p[2] - o[2];
  if (METRIC == RS_EVAL_REG_POINT) {
    const double y[3] = {q[0] - o[0], q[1] - o[1], q[2] - o[2]};
    w[0] = x0, w[1] = x1, w[2] = x2;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      w[3 + i] = y[i];
      w[6 + 3 * i] = y[i] * x0, w[7 + 3 * i] = y[i] * x1, w[8 + 3 * i] = y[i] * x2;
    }
    w[15] = (x0 * x0 + x1 * x1) + x2 * x2;
    w[16] = d2;
  } else {
    const double u0 = T[3] - T[0], u1 = T[4] - T[1], u2 = T[5] - T[2];
    const double v0 = T[6] - T[0], v1 = T[7] - T[1], v2 = T[8] - T[2];
    const double N0 = u1 * v2 - u2 * v1, N1 = u2 * v0 - u0 * v2, N2 = u0 * v1 - u1 * v0;
    const double l = sqrt((N0 * N0 + N1 * N1) + N2 * N2);
    const double n0 = N0 / l, n1 = N1 / l, n2 = N2 / l;
    const double e0 = p[0] - q[0], e1 = p[1] - q[1], e2 = p[2] - q[2];
    const double r = (n0 * e0 + n1 * e1) + n2 * e2;
    const double J[7] = {x1 * n2 - x2 * n1, x2 * n0 - x0 * n2, x0 * n1 - x1 * n0, n0, n1, n2,
                         (x0 * n0 + x1 * n1) + x2 * n2};
    int at = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = i; j < 7; ++j) w[at++] = J[i] * J[j];
#pragma unroll
    for (int i = 0; i < 7; ++i) w[28 + i] = J[i] * r;
    w[35] = r * r;
    w[36] = d2;
  }
}

template <int METRIC>
__global__ __launch_bounds__(kEvalThreads) void k_reg_moments(
    const double *moved, const double *closest, const double *d2, const int32_t *face,
    const double *tri, int64_t nf, int64_t n, RegXform X, RegState *st, uint8_t *kept,
    double *part) {
#pragma clang fp contract(off)
  constexpr int NS = METRIC == RS_EVAL_REG_POINT ? kRegPointSlots : kRegPlaneSlots;
  __shared__ double sh[kRegFold][kEvalThreads];
  const double tau = st->tau;   // NaN when nothing matched: nothing is kept
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  unsigned long long count = 0;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * RS_EVAL_REG_BLOCK + threadIdx.x;
  for (int j = 0; j < kRegItems; ++j) {
    const int64_t i = base + static_cast<int64_t>(j) * kEvalThreads;
    double w[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) w[s] = 0.0;
    if (i < n) {
      const int f = face[i];
      const double d = d2[i];
      const bool k = f >= 0 && f < nf && d <= tau;
      kept[i] = k ? 1 : 0;
      if (k) {
        double p[3], q[3], T[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = moved[3 * i + c], q[c] = closest[3 * i + c];
#pragma unroll
        for (int c = 0; c < 9; ++c)
          T[c] = METRIC == RS_EVAL_REG_PLANE ? tri[9 * static_cast<int64_t>(f) + c] : 0.0;
        reg_terms<METRIC>(p, q, d, T, X.o, w);
        ++count;
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = acc[s] + w[s];
  }
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off);
  if ((threadIdx.x & 63) == 0 && count > 0) atomicAdd(&st->kept, count);
  // the 256 lane sums fold by halving, kRegFold slots at a time
#pragma unroll
  for (int g = 0; g < NS; g += kRegFold) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRegFold; ++j)
      if (g + j < NS) sh[j][threadIdx.x] = acc[g + j];
    for (int h = kEvalThreads / 2; h > 0; h >>= 1) {
      __syncthreads();
      if (static_cast<int>(threadIdx.x) < h) {
#pragma unroll
        for (int j = 0; j < kRegFold; ++j)
          if (g + j < NS) sh[j][threadIdx.x] = sh[j][threadIdx.x] + sh[j][threadIdx.x + h];
      }
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < kRegFold; ++j)
        if (g + j < NS) part[static_cast<int64_t>(blockIdx.x) * RS_EVAL_REG_SLOTS + g + j] = sh[j][0];
    }
  }
}

__global__ __launch_bounds__(64) void k_reg_sum(const double *part, int64_t nblocks, int ns,
                                                const RegState *st,
                                                const unsigned long long *stats,
                                                rs_eval_step *rec) {
#pragma clang fp contract(off)
  const int s = threadIdx.x;
  if (blockIdx.x != 0) return;
  if (s < RS_EVAL_REG_SLOTS) {
    double acc = 0.0;
    if (s < ns)
      for (int64_t b = 0; b < nblocks; ++b) acc = acc + part[b * RS_EVAL_REG_SLOTS + s];
    rec->moments[s] = acc;
  }
  if (s == 0) {
    rec->matched = static_cast<int64_t>(st->m);
    rec->kept = static_cast<int64_t>(st->kept);
    rec->k = static_cast<int64_t>(st->k);
    rec->tests = static_cast<int64_t>(stats[kEvalTests]);
    rec->tau = st->tau;
  }
}

}  // namespace rsd

static_assert(RS_EVAL_REG_TIMING_SLOTS == 4, "transform, query, select, moments");
static_assert(sizeof(rs_eval_step) == 360, "rs_eval_step");

struct rs_eval_index {
  rs_ctx *ctx = nullptr;
  rsd::EvalGrid G = {};
  int64_t nf = 0, entries = 0;
  rs_eval_info info = {};
  // the mesh and its grid
  void *mesh = nullptr;
  double *tri = nullptr;
  int32_t *cnt = nullptr, *ent = nullptr;
  // rs_eval_index_query's buffers, grow-only
  void *qbuf = nullptr;
  size_t qbytes = 0;
  // the source cloud and the arrays of a step
  void *sbuf = nullptr;
  int64_t n = 0, nblocks = 0;
  bool stepped = false;
  double *src = nullptr, *moved = nullptr, *d2 = nullptr, *closest = nullptr, *part = nullptr;
  int32_t *face = nullptr;
  uint8_t *kept = nullptr;
  char *state = nullptr;   // [stats | hist | RegState | rs_eval_step], cleared before a step
  size_t state_bytes = 0;
  unsigned long long *stats = nullptr;
  unsigned *hist = nullptr;
  rsd::RegState *st = nullptr;
  rs_eval_step *rec = nullptr;
  rs::StageTimer<5, RS_EVAL_REG_TIMING_SLOTS> reg{-1.0};
};

extern "C" int rs_eval_index_destroy(rs_eval_index *ix) {
  if (!ix) return RS_OK;
  if (ix->ctx) (void)hipSetDevice(ix->ctx->device);
  if (ix->mesh) (void)hipFree(ix->mesh);
  if (ix->qbuf) (void)hipFree(ix->qbuf);
  if (ix->sbuf) (void)hipFree(ix->sbuf);
  ix->reg.destroy();
  delete ix;
  return RS_OK;
}

namespace {

struct EvalIndexGuard {
  rs_eval_index *ix;
  ~EvalIndexGuard() { rs_eval_index_destroy(ix); }
};

// rs_eval_mesh_distance's steps up to the scatter, into memory the index owns
int eval_index_build(rs_eval_index *ix, const double *vertices, int64_t nv, const int32_t *faces,
                     int64_t nf, double cell) {
  rs_ctx *c = ix->ctx;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t f = 0; f < nf; ++f) {
    const double *a = vertices + 3 * static_cast<int64_t>(faces[3 * f]);
    const double *b = vertices + 3 * static_cast<int64_t>(faces[3 * f + 1]);
    const double *v = vertices + 3 * static_cast<int64_t>(faces[3 * f + 2]);
    bool ok = true;
    for (int k = 0; k < 3; ++k)
      ok = ok && rsd::eval_finite(a[k]) && rsd::eval_finite(b[k]) && rsd::eval_finite(v[k]);
    if (!ok) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::fmin(lo[k], std::fmin(a[k], std::fmin(b[k], v[k])));
      hi[k] = std::fmax(hi[k], std::fmax(a[k], std::fmax(b[k], v[k])));
    }
  }
  rsd::EvalGrid G;
  G.cell = cell;
  double ncell_d = 1.0, mag = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!(lo[k] <= hi[k])) lo[k] = hi[k] = 0.0;   // no finite face
    const double ext = hi[k] - lo[k];
    if (!std::isfinite(ext)) return fail(RS_EINVAL, "the extent of the mesh's box is not finite");
    const double nd = std::floor(ext / cell) + 1.0;
    if (!(nd <= static_cast<double>(RS_EVAL_MAX_CELLS)))
      return fail(RS_EINVAL,
                  "the grid has more than RS_EVAL_MAX_CELLS = 2^24 cells: choose a larger cell");
    G.lo[k] = lo[k];
    G.dim[k] = static_cast<int>(nd);
    ncell_d *= nd;
    mag = std::fmax(mag, std::fmax(std::fabs(lo[k]), std::fabs(hi[k])));
  }
  if (ncell_d > static_cast<double>(RS_EVAL_MAX_CELLS))
    return fail(RS_EINVAL,
                "the grid has more than RS_EVAL_MAX_CELLS = 2^24 cells: choose a larger cell");
  if (cell < mag / 16777216.0)
    return fail(RS_EINVAL,
                "cell is below 2^-24 of the box's largest coordinate magnitude: choose a larger "
                "cell");
  const int64_t ncell = static_cast<int64_t>(G.dim[0]) * G.dim[1] * G.dim[2];
  int64_t entries = 0, skipped = 0;
  for (int64_t f = 0; f < nf; ++f) {
    const double *a = vertices + 3 * static_cast<int64_t>(faces[3 * f]);
    const double *b = vertices + 3 * static_cast<int64_t>(faces[3 * f + 1]);
    const double *v = vertices + 3 * static_cast<int64_t>(faces[3 * f + 2]);
    if (!rsd::eval_face_valid(a, b, v)) {
      ++skipped;
      continue;
    }
    int c0[3], c1[3];
    rsd::eval_face_cells(G, a, b, v, c0, c1);
    entries += static_cast<int64_t>(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
    if (entries > RS_EVAL_MAX_ENTRIES)
      return fail(RS_EINVAL,
                  "more than RS_EVAL_MAX_ENTRIES = 2^27 face-cell registrations: choose a larger "
                  "cell");
  }

  const int nchunks = static_cast<int>((ncell + rsd::kEvalScanChunk - 1) / rsd::kEvalScanChunk);
  using U64 = unsigned long long;
  rs::Layout L;
  const auto b_tri = L.add<double>(9 * static_cast<size_t>(nf));
  const auto b_cnt = L.add<int32_t>(static_cast<size_t>(ncell) + 1);
  const auto b_fill = L.add<int32_t>(static_cast<size_t>(ncell));
  const auto b_sums = L.add<int32_t>(static_cast<size_t>(nchunks) + 1);
  const auto b_ent = L.add<int32_t>(static_cast<size_t>(entries));
  const auto b_stats = L.add<U64>(8);
  const auto b_vert = L.add<double>(3 * static_cast<size_t>(nv));
  const auto b_face = L.add<int32_t>(3 * static_cast<size_t>(nf));
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMalloc(&ix->mesh, L.total() + 256));
  L.bind(ix->mesh, nullptr);

  hipStream_t s = c->stream;
  const dim3 blk(rsd::kEvalThreads), sblk(rsd::kEvalScanThreads);
  if (nv) HIP_TRY(hipMemcpyAsync(b_vert.dev(), vertices, b_vert.bytes, hipMemcpyHostToDevice, s));
  if (nf) HIP_TRY(hipMemcpyAsync(b_face.dev(), faces, b_face.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(b_stats.dev(), 0, b_stats.bytes, s));
  HIP_TRY(hipMemsetAsync(b_cnt.dev(), 0, L.span(b_cnt, b_sums), s));   // cnt and fill
  if (nf)
    hipLaunchKernelGGL(rsd::k_eval_bin, dim3(rs::blocks(nf, rsd::kEvalThreads)), blk, 0, s,
                       b_vert.dev(), b_face.dev(), nf, G, b_tri.dev(), b_cnt.dev(), b_stats.dev());
  hipLaunchKernelGGL(rsd::k_eval_scan_chunks, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), b_stats.dev());
  hipLaunchKernelGGL(rsd::k_eval_scan, dim3(1), sblk, 0, s, b_sums.dev(),
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_eval_scan_add, dim3(nchunks), sblk, 0, s, b_cnt.dev(), ncell,
                     b_sums.dev(), nchunks, b_stats.dev());
  if (nf)
    hipLaunchKernelGGL(rsd::k_eval_scatter, dim3(rs::blocks(nf, rsd::kEvalThreads)), blk, 0, s,
                       b_tri.dev(), nf, G, b_cnt.dev(), b_fill.dev(), b_ent.dev(), entries);
  HIP_TRY(hipGetLastError());
  U64 stats[8];
  HIP_TRY(hipMemcpyAsync(stats, b_stats.dev(), b_stats.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (static_cast<int64_t>(stats[rsd::kEvalEntries]) != entries ||
      static_cast<int64_t>(stats[rsd::kEvalSkipped]) != skipped)
    return fail(RS_EDEVICE, "host and device disagree about the faces' validity or cells");

  ix->G = G;
  ix->nf = nf;
  ix->entries = entries;
  ix->tri = b_tri.dev();
  ix->cnt = b_cnt.dev();
  ix->ent = b_ent.dev();
  const rs_eval_info zero = {{0, 0, 0}, 0, 0, 0, 0, 0};
  ix->info = zero;
  for (int k = 0; k < 3; ++k) ix->info.cells[k] = G.dim[k];
  ix->info.entries = entries;
  ix->info.largest_cell = static_cast<int64_t>(stats[rsd::kEvalLargest]);
  ix->info.faces_skipped = skipped;
  return RS_OK;
}

}  // namespace

extern "C" int rs_eval_index_create(rs_ctx *c, const double *vertices, int64_t nv,
                                    const int32_t *faces, int64_t nf, double cell,
                                    rs_eval_index **out, rs_eval_info *info) {
  if (out) *out = nullptr;
  if (!c || !out || !info) return fail(RS_EINVAL, "null pointer");
  if (nv < 0 || nf < 0) return fail(RS_EINVAL, "negative size");
  if (nv > INT32_MAX || 3 * nf > INT32_MAX)
    return fail(RS_EINVAL, "nv and 3 nf must be in 0..2^31 - 1");
  if (!std::isfinite(cell) || !(cell > 0.0))
    return fail(RS_EINVAL, "cell must be finite and positive");
  if ((nv > 0 && !vertices) || (nf > 0 && !faces)) return fail(RS_EINVAL, "null pointer");
  for (int64_t k = 0; k < 3 * nf; ++k)
    if (faces[k] < 0 || faces[k] >= nv) return fail(RS_EINVAL, "a face index is out of range");
  const rs_eval_info zero = {{0, 0, 0}, 0, 0, 0, 0, 0};
  *info = zero;
  EvalIndexGuard guard{new rs_eval_index};
  guard.ix->ctx = c;
  const int st = eval_index_build(guard.ix, vertices, nv, faces, nf, cell);
  if (st) return st;
  *info = guard.ix->info;
  *out = guard.ix;
  guard.ix = nullptr;
  return RS_OK;
}

extern "C" int rs_eval_index_query(rs_eval_index *ix, const double *pts, int64_t n,
                                   double max_dist, double *d2, int32_t *face, double *closest,
                                   rs_eval_info *info) {
  if (!ix || !info) return fail(RS_EINVAL, "null pointer");
  if (n < 0) return fail(RS_EINVAL, "negative size");
  if (n > RS_EVAL_MAX_POINTS) return fail(RS_EINVAL, "more queries than RS_EVAL_MAX_POINTS");
  if (!(max_dist > 0.0)) return fail(RS_EINVAL, "max_dist must be positive (+inf is allowed)");
  *info = ix->info;
  if (n == 0) return RS_OK;
  if (!pts || !d2 || !face || !closest) return fail(RS_EINVAL, "null pointer");
  rs_ctx *c = ix->ctx;
  using U64 = unsigned long long;
  rs::Layout L;
  const auto b_pts = L.add<double>(3 * static_cast<size_t>(n));
  const auto b_d2 = L.add<double>(static_cast<size_t>(n));
  const auto b_closest = L.add<double>(3 * static_cast<size_t>(n));
  const auto b_best = L.add<int32_t>(static_cast<size_t>(n));
  const auto b_stats = L.add<U64>(8);
  HIP_TRY(hipSetDevice(c->device));
  if (L.total() > ix->qbytes) {
    if (ix->qbuf) HIP_TRY(hipFree(ix->qbuf));
    ix->qbuf = nullptr, ix->qbytes = 0;
    HIP_TRY(hipMalloc(&ix->qbuf, L.total()));
    ix->qbytes = L.total();
  }
  L.bind(ix->qbuf, nullptr);
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_pts.dev(), pts, b_pts.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(b_stats.dev(), 0, b_stats.bytes, s));
  hipLaunchKernelGGL(rsd::k_eval_query, dim3(rs::blocks(n, rsd::kEvalThreads)),
                     dim3(rsd::kEvalThreads), 0, s, b_pts.dev(), n, ix->G, ix->cnt, ix->ent,
                     ix->entries, ix->tri, max_dist, b_d2.dev(), b_best.dev(), b_closest.dev(),
                     b_stats.dev());
  HIP_TRY(hipGetLastError());
  U64 stats[8];
  HIP_TRY(hipMemcpyAsync(d2, b_d2.dev(), b_d2.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(closest, b_closest.dev(), b_closest.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(face, b_best.dev(), b_best.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(stats, b_stats.dev(), b_stats.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  info->tests = static_cast<int64_t>(stats[rsd::kEvalTests]);
  for (int64_t i = 0; i < n; ++i) info->beyond += std::isinf(d2[i]) ? 1 : 0;
  return RS_OK;
}

extern "C" int rs_eval_index_set_points(rs_eval_index *ix, const double *pts, int64_t n) {
  if (!ix || !pts) return fail(RS_EINVAL, "null pointer");
  if (n < 1) return fail(RS_EINVAL, "the source cloud needs at least one point");
  if (n > RS_EVAL_MAX_POINTS) return fail(RS_EINVAL, "more points than RS_EVAL_MAX_POINTS");
  rs_ctx *c = ix->ctx;
  const int64_t nblocks = (n + RS_EVAL_REG_BLOCK - 1) / RS_EVAL_REG_BLOCK;
  using U64 = unsigned long long;
  rs::Layout L;
  const auto b_src = L.add<double>(3 * static_cast<size_t>(n));
  const auto b_moved = L.add<double>(3 * static_cast<size_t>(n));
  const auto b_d2 = L.add<double>(static_cast<size_t>(n));
  const auto b_closest = L.add<double>(3 * static_cast<size_t>(n));
  const auto b_part = L.add<double>(static_cast<size_t>(nblocks) * RS_EVAL_REG_SLOTS);
  const auto b_face = L.add<int32_t>(static_cast<size_t>(n));
  const auto b_kept = L.add<uint8_t>(static_cast<size_t>(n));
  const auto b_stats = L.add<U64>(8);
  const auto b_hist = L.add<unsigned>(rsd::kRegPasses * rsd::kRegBins);
  const auto b_st = L.add<rsd::RegState>(1);
  const auto b_rec = L.add<rs_eval_step>(1);
  HIP_TRY(hipSetDevice(c->device));
  ix->stepped = false;
  ix->n = 0;
  if (ix->sbuf) HIP_TRY(hipFree(ix->sbuf));
  ix->sbuf = nullptr;
  HIP_TRY(hipMalloc(&ix->sbuf, L.total()));
  L.bind(ix->sbuf, nullptr);
  HIP_TRY(hipMemcpyAsync(b_src.dev(), pts, b_src.bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  ix->src = b_src.dev(), ix->moved = b_moved.dev(), ix->d2 = b_d2.dev();
  ix->closest = b_closest.dev(), ix->part = b_part.dev(), ix->face = b_face.dev();
  ix->kept = b_kept.dev(), ix->stats = b_stats.dev(), ix->hist = b_hist.dev();
  ix->st = b_st.dev(), ix->rec = b_rec.dev();
  ix->state = reinterpret_cast<char *>(b_stats.dev());
  ix->state_bytes = L.from(b_stats);
  ix->n = n;
  ix->nblocks = nblocks;
  return RS_OK;
}

extern "C" int rs_eval_index_step(rs_eval_index *ix, const double *T, const double *origin,
                                  double keep, double max_dist, int32_t metric,
                                  rs_eval_step *out) {
  if (!ix || !T || !origin || !out) return fail(RS_EINVAL, "null pointer");
  if (ix->n < 1) return fail(RS_EINVAL, "no source cloud: call rs_eval_index_set_points first");
  for (int k = 0; k < 13; ++k)
    if (!std::isfinite(T[k])) return fail(RS_EINVAL, "the similarity is not finite");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(origin[k])) return fail(RS_EINVAL, "origin is not finite");
  if (!(keep > 0.0 && keep <= 1.0)) return fail(RS_EINVAL, "keep must be in (0, 1]");
  if (!(max_dist > 0.0)) return fail(RS_EINVAL, "max_dist must be positive (+inf is allowed)");
  if (metric != RS_EVAL_REG_POINT && metric != RS_EVAL_REG_PLANE)
    return fail(RS_EINVAL, "metric must be RS_EVAL_REG_POINT or RS_EVAL_REG_PLANE");
  rs_ctx *c = ix->ctx;
  rsd::RegXform X;
  X.s = T[0];
  for (int k = 0; k < 9; ++k) X.R[k] = T[1 + k];
  for (int k = 0; k < 3; ++k) X.t[k] = T[10 + k], X.o[k] = origin[k];
  const int64_t n = ix->n;
  const dim3 blk(rsd::kEvalThreads), per_point(rs::blocks(n, rsd::kEvalThreads));
  const dim3 per_block(static_cast<unsigned>(ix->nblocks));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int st;
  HIP_TRY(hipMemsetAsync(ix->state, 0, ix->state_bytes, s));
  if ((st = ix->reg.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_reg_transform, per_point, blk, 0, s, ix->src, n, X, ix->moved);
  if ((st = ix->reg.mark(1, s))) return st;
  hipLaunchKernelGGL(rsd::k_eval_query, per_point, blk, 0, s, ix->moved, n, ix->G, ix->cnt,
                     ix->ent, ix->entries, ix->tri, max_dist, ix->d2, ix->face, ix->closest,
                     ix->stats);
  if ((st = ix->reg.mark(2, s))) return st;
  for (int pass = 0; pass < rsd::kRegPasses; ++pass) {
    hipLaunchKernelGGL(rsd::k_reg_hist, per_block, blk, 0, s, ix->d2, ix->face, n, pass, ix->st,
                       ix->hist);
    hipLaunchKernelGGL(rsd::k_reg_pick, dim3(1), dim3(64), 0, s, pass, keep, ix->hist, ix->st);
  }
  if ((st = ix->reg.mark(3, s))) return st;
  if (metric == RS_EVAL_REG_POINT)
    hipLaunchKernelGGL(rsd::k_reg_moments<RS_EVAL_REG_POINT>, per_block, blk, 0, s, ix->moved,
                       ix->closest, ix->d2, ix->face, ix->tri, ix->nf, n, X, ix->st, ix->kept,
                       ix->part);
  else
    hipLaunchKernelGGL(rsd::k_reg_moments<RS_EVAL_REG_PLANE>, per_block, blk, 0, s, ix->moved,
                       ix->closest, ix->d2, ix->face, ix->tri, ix->nf, n, X, ix->st, ix->kept,
                       ix->part);
  hipLaunchKernelGGL(rsd::k_reg_sum, dim3(1), dim3(64), 0, s, ix->part, ix->nblocks,
                     metric == RS_EVAL_REG_POINT ? rsd::kRegPointSlots : rsd::kRegPlaneSlots,
                     ix->st, ix->stats, ix->rec);
  HIP_TRY(hipGetLastError());
  if ((st = ix->reg.mark(4, s))) return st;
  rs_eval_step rec;
  HIP_TRY(hipMemcpyAsync(&rec, ix->rec, sizeof rec, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < 4; ++k)
    if ((st = ix->reg.read(k, k, k + 1))) return st;
  ix->stepped = true;
  *out = rec;
  return RS_OK;
}

extern "C" int rs_eval_index_read(rs_eval_index *ix, double *d2, int32_t *face, double *closest,
                                  uint8_t *kept) {
  if (!ix) return fail(RS_EINVAL, "null pointer");
  if (!ix->stepped) return fail(RS_EINVAL, "no step has run since rs_eval_index_set_points");
  rs_ctx *c = ix->ctx;
  const size_t n = static_cast<size_t>(ix->n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (d2) HIP_TRY(hipMemcpyAsync(d2, ix->d2, n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (face) HIP_TRY(hipMemcpyAsync(face, ix->face, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (closest)
    HIP_TRY(hipMemcpyAsync(closest, ix->closest, 3 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (kept) HIP_TRY(hipMemcpyAsync(kept, ix->kept, n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RS_OK;
}

extern "C" int rs_eval_index_timing(rs_eval_index *ix, int32_t enable, double *ms) {
  if (!ix || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(ix->ctx->device));
  const int st = ix->reg.enable(enable != 0);
  if (st) return st;
  ix->reg.copy_out(ms);
  return RS_OK;
}
