// Mesh simplification on the GPU (rs_mesh_simplify): vertex clustering on a uniform grid, every
// cluster placed by its accumulated error quadric.  The definition stands in include/rsamd.h;
// tests/simplify_ref.py restates it in numpy, to the bit.
//
// Three times the work is "items grouped by bucket, each bucket's items ascending": vertices by
// cluster (the mean), face corners by cluster (the quadric) and faces by their smallest cluster
// (the duplicates).  That is written once: the items' buckets stand in an int32 array (-1: no
// bucket), and
//
//   k_simplify_count      count[bucket]++, integer atomicAdd
//   rs::mesh_scan         the exclusive scan of mesh.hip (chunks of RS_MESH_SCAN_CHUNK)
//   k_simplify_scatter    item / per into its bucket's row through an atomic cursor
//   simplify_sort         one lane sorts its row in place: insertion up to 24 items, heap sort
//                         above, O(d log d); the sort removes the cursor's arrival order
//
// serve all three; what differs is the order (plain integers, or faces by their other two
// clusters and then their index) and what the lane does with the sorted row:
//
//   k_simplify_keys       per vertex: the cell key, and the cell's occupancy flag
//   k_simplify_vmap       per vertex: the cluster (the scanned flag of its cell), the cluster's key
//   k_simplify_mean       per cluster: the ascending sum of its vertices, divided by their number
//   k_simplify_faces      per face: the plane (n, d), the corners' clusters, degenerate or not,
//                         and for the others the smallest cluster and the other two in order
//   k_simplify_quadric    per cluster: the ten sums over its distinct faces in ascending order,
//                         Jacobi, the position, the test that it stays in the cell
//   k_simplify_dups       per cluster: the faces whose smallest cluster it is, sorted; the first
//                         of every run of equal cluster sets stays
//   k_simplify_emit       per face: the survivors to their scanned offsets, fmap
//
// The host waits twice: for the sizes, which it compares with the capacities, and for the
// results.  The number of clusters is not known to the host while the kernels run: arrays and
// grids per cluster are sized for nv, and a lane reads the count from the scan's total.
//
// Every global index is bounded.  A vertex has passed the host's test that its cell lies in the
// grid, so key < cells; a face index has passed rs::mesh_check; a cluster number is a scanned
// flag below the total, which is at most nv; a row is written at off[b] + cursor < off[b + 1],
// because the cursor counts exactly the items the count kernel counted; the emit kernel writes
// below the scanned total, which is at most nf.  Every loop has a bound: Jacobi 30 sweeps, the
// sorts and the runs the row's length.
#include <hip/hip_runtime.h>

#include <cmath>

#include "device_math.h"
#include "host.h"

namespace rsd {

constexpr int kSimThreads = 256;
constexpr int kSimInsertionMax = 24;   // longer rows are heap-sorted
// info words (int32 each)
constexpr int kSimFallbacks = 0, kSimDegenerate = 1, kSimDuplicates = 2, kSimLongest = 3;
constexpr int kSimInfoWords = 4;

struct SimGrid {
  double origin[3], cell;
  int d0, d1;
};

__device__ __forceinline__ int64_t sim_lane() {
  return static_cast<int64_t>(blockIdx.x) * kSimThreads + threadIdx.x;
}

// the cell index along one axis, as a double
__device__ __forceinline__ double sim_cell(double x, double origin, double cell) {
#pragma clang fp contract(off)
  return floor((x - origin) / cell);
}

__global__ __launch_bounds__(kSimThreads) void k_simplify_keys(const double *vert, int64_t nv,
                                                               SimGrid G, int32_t *key,
                                                               int32_t *flag) {
  const int64_t v = sim_lane();
  if (v >= nv) return;
  // the host has seen every index inside 0..dims - 1, so the casts are exact
  const int i0 = static_cast<int>(sim_cell(vert[3 * v], G.origin[0], G.cell));
  const int i1 = static_cast<int>(sim_cell(vert[3 * v + 1], G.origin[1], G.cell));
  const int i2 = static_cast<int>(sim_cell(vert[3 * v + 2], G.origin[2], G.cell));
  const int k = (i2 * G.d1 + i1) * G.d0 + i0;
  key[v] = k;
  flag[k] = 1;   // every writer writes the same value
}

__global__ __launch_bounds__(kSimThreads) void k_simplify_vmap(const int32_t *key, int64_t nv,
                                                               const int32_t *cbase,
                                                               int32_t *vmap, int32_t *ckey) {
  const int64_t v = sim_lane();
  if (v >= nv) return;
  const int k = key[v], c = cbase[k];
  vmap[v] = c;
  ckey[c] = k;   // every writer writes the same value
}

// ------------------------------------------------------------------------------------------
// items grouped by bucket
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSimThreads) void k_simplify_count(const int32_t *bucket, int64_t n,
                                                                int32_t *count) {
  const int64_t i = sim_lane();
  if (i >= n) return;
  const int b = bucket[i];
  if (b >= 0) atomicAdd(count + b, 1);
}

__global__ __launch_bounds__(kSimThreads) void k_simplify_scatter(const int32_t *bucket,
                                                                  int64_t n, int per,
                                                                  const int32_t *off,
                                                                  int32_t *cursor,
                                                                  int32_t *rows) {
  const int64_t i = sim_lane();
  if (i >= n) return;
  const int b = bucket[i];
  if (b < 0) return;
  rows[static_cast<int64_t>(off[b]) + atomicAdd(cursor + b, 1)] = static_cast<int32_t>(i / per);
}

template <class Less>
__device__ __forceinline__ void simplify_sift(int32_t *row, int start, int end, Less less) {
  int root = start;
  const int x = row[root];
  for (;;) {   // the depth of the heap: at most log2(end) + 1 rounds
    int child = 2 * root + 1;
    if (child >= end) break;
    int cv = row[child];
    if (child + 1 < end) {
      const int c2 = row[child + 1];
      if (less(cv, c2)) {
        cv = c2;
        ++child;
      }
    }
    if (!less(x, cv)) break;
    row[root] = cv;
    root = child;
  }
  row[root] = x;
}

// row[0 .. d) ascending under `less`, in place in global memory
template <class Less>
__device__ __forceinline__ void simplify_sort(int32_t *row, int d, Less less) {
  if (d <= kSimInsertionMax) {
    for (int i = 1; i < d; ++i) {
      const int x = row[i];
      int j = i;
      while (j > 0 && less(x, row[j - 1])) {
        row[j] = row[j - 1];
        --j;
      }
      row[j] = x;
    }
  } else {
    for (int i = d / 2 - 1; i >= 0; --i) simplify_sift(row, i, d, less);
    for (int end = d - 1; end > 0; --end) {
      const int top = row[0];
      row[0] = row[end];
      row[end] = top;
      simplify_sift(row, 0, end, less);
    }
  }
}

// the wave's longest row into the info record; every lane of the wave calls it
__device__ __forceinline__ void simplify_longest(int d, int32_t *info) {
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(d, off);
    d = o > d ? o : d;
  }
  if ((threadIdx.x & 63) == 0 && d > 0) atomicMax(info + kSimLongest, d);
}

struct SimLessInt {
  __device__ __forceinline__ bool operator()(int a, int b) const { return a < b; }
};

// faces by their middle cluster, their largest cluster, their index
struct SimLessFace {
  const int32_t *fkey;
  __device__ __forceinline__ bool operator()(int a, int b) const {
    const int am = fkey[2 * static_cast<int64_t>(a)], bm = fkey[2 * static_cast<int64_t>(b)];
    if (am != bm) return am < bm;
    const int ah = fkey[2 * static_cast<int64_t>(a) + 1];
    const int bh = fkey[2 * static_cast<int64_t>(b) + 1];
    if (ah != bh) return ah < bh;
    return a < b;
  }
};

// ------------------------------------------------------------------------------------------
// the three users
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSimThreads) void k_simplify_mean(const int32_t *off,
                                                               const int32_t *nclusters,
                                                               int32_t *rows, const double *vert,
                                                               double *mean, int32_t *info) {
#pragma clang fp contract(off)
  const int64_t c = sim_lane();
  const bool in = c < *nclusters;
  const int d = in ? off[c + 1] - off[c] : 0;   // >= 1 for a cluster
  simplify_longest(d, info);
  if (!in) return;
  int32_t *row = rows + off[c];
  simplify_sort(row, d, SimLessInt());
  const double *p = vert + 3 * static_cast<int64_t>(row[0]);
  double s0 = p[0], s1 = p[1], s2 = p[2];
  for (int i = 1; i < d; ++i) {
    p = vert + 3 * static_cast<int64_t>(row[i]);
    s0 += p[0];
    s1 += p[1];
    s2 += p[2];
  }
  const double dn = static_cast<double>(d);
  mean[3 * c] = s0 / dn;
  mean[3 * c + 1] = s1 / dn;
  mean[3 * c + 2] = s2 / dn;
}

__global__ __launch_bounds__(kSimThreads) void k_simplify_faces(
    const double *vert, const int32_t *faces, int64_t nf, const int32_t *vmap, double *plane,
    int32_t *cbucket, int32_t *fbucket, int32_t *fkey, int32_t *fmap, int32_t *info) {
#pragma clang fp contract(off)
  const int64_t f = sim_lane();
  if (f >= nf) return;
  const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  const double *xa = vert + 3 * static_cast<int64_t>(ia);
  const double *xb = vert + 3 * static_cast<int64_t>(ib);
  const double *xc = vert + 3 * static_cast<int64_t>(ic);
  const double a0 = xa[0], a1 = xa[1], a2 = xa[2];
  const double u0 = xb[0] - a0, u1 = xb[1] - a1, u2 = xb[2] - a2;
  const double w0 = xc[0] - a0, w1 = xc[1] - a1, w2 = xc[2] - a2;
  const double n0 = u1 * w2 - u2 * w1;
  const double n1 = u2 * w0 - u0 * w2;
  const double n2 = u0 * w1 - u1 * w0;
  plane[4 * f] = n0;
  plane[4 * f + 1] = n1;
  plane[4 * f + 2] = n2;
  plane[4 * f + 3] = -((n0 * a0 + n1 * a1) + n2 * a2);
  const int c0 = vmap[ia], c1 = vmap[ib], c2 = vmap[ic];
  cbucket[3 * f] = c0;
  cbucket[3 * f + 1] = c1;
  cbucket[3 * f + 2] = c2;
  if (c0 == c1 || c1 == c2 || c0 == c2) {
    fbucket[f] = -1;
    fmap[f] = -1;
    atomicAdd(info + kSimDegenerate, 1);
    return;
  }
  const int lo = min(c0, min(c1, c2)), hi = max(c0, max(c1, c2));
  fbucket[f] = lo;
  fkey[2 * f] = c0 + c1 + c2 - lo - hi;   // three values below 2^27
  fkey[2 * f + 1] = hi;
}

__global__ __launch_bounds__(kSimThreads) void k_simplify_quadric(
    const int32_t *off, const int32_t *nclusters, int32_t *rows, const double *plane,
    const double *mean, const int32_t *ckey, SimGrid G, int placement, double rank_tol,
    double *quad, double *pos, int32_t *info) {
#pragma clang fp contract(off)
  const int64_t c = sim_lane();
  const bool in = c < *nclusters;
  const int d = in ? off[c + 1] - off[c] : 0;
  simplify_longest(d, info);
  if (!in) return;
  int32_t *row = rows + off[c];
  simplify_sort(row, d, SimLessInt());
  double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int last = -1;   // a face with two corners here stands twice in the row
  for (int i = 0; i < d; ++i) {
    const int f = row[i];
    if (f == last) continue;
    const double *pl = plane + 4 * static_cast<int64_t>(f);
    const double n0 = pl[0], n1 = pl[1], n2 = pl[2], dd = pl[3];
    const double t[10] = {n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2,
                          n2 * n2, n0 * dd, n1 * dd, n2 * dd, dd * dd};
#pragma unroll
    for (int k = 0; k < 10; ++k) q[k] = last < 0 ? t[k] : q[k] + t[k];
    last = f;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) quad[10 * c + k] = q[k];

  const double m[3] = {mean[3 * c], mean[3 * c + 1], mean[3 * c + 2]};
  double x[3] = {m[0], m[1], m[2]};
  if (placement == RS_SIMPLIFY_QUADRIC) {
    double A[9] = {q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]}, V[9];
    jacobi3_exact(A, V);
    const double l[3] = {A[0], A[4], A[8]};
    double L = l[0];
    if (l[1] > L) L = l[1];
    if (l[2] > L) L = l[2];
    if (L > 0.0) {
      const double r[3] = {(-q[6]) - ((q[0] * m[0] + q[1] * m[1]) + q[2] * m[2]),
                           (-q[7]) - ((q[1] * m[0] + q[3] * m[1]) + q[4] * m[2]),
                           (-q[8]) - ((q[2] * m[0] + q[4] * m[1]) + q[5] * m[2])};
      const double thr = rank_tol * L;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        if (l[i] > thr) {
          const double g = ((V[i] * r[0] + V[3 + i] * r[1]) + V[6 + i] * r[2]) / l[i];
#pragma unroll
          for (int a = 0; a < 3; ++a) x[a] = x[a] + g * V[3 * a + i];
        }
      }
      const int k = ckey[c];
      const double want[3] = {static_cast<double>(k % G.d0),
                              static_cast<double>(k / G.d0 % G.d1),
                              static_cast<double>(k / G.d0 / G.d1)};
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 3; ++a)
        ok = ok && isfinite(x[a]) && sim_cell(x[a], G.origin[a], G.cell) == want[a];
      if (!ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] = m[a];
        atomicAdd(info + kSimFallbacks, 1);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) pos[3 * c + a] = x[a];
}

// fkeep is zero on entry; it becomes the flags the emit offsets are scanned from
__global__ __launch_bounds__(kSimThreads) void k_simplify_dups(const int32_t *off,
                                                               const int32_t *nclusters,
                                                               int32_t *rows,
                                                               const int32_t *fkey,
                                                               int32_t *fkeep, int32_t *fmap,
                                                               int32_t *info) {
  const int64_t c = sim_lane();
  const bool in = c < *nclusters;
  const int d = in ? off[c + 1] - off[c] : 0;
  simplify_longest(d, info);
  if (!in || d == 0) return;
  int32_t *row = rows + off[c];
  simplify_sort(row, d, SimLessFace{fkey});
  int pm = -1, ph = -1, dups = 0;
  for (int i = 0; i < d; ++i) {
    const int f = row[i];
    const int fm = fkey[2 * static_cast<int64_t>(f)], fh = fkey[2 * static_cast<int64_t>(f) + 1];
    if (fm == pm && fh == ph) {
      fmap[f] = -2;
      ++dups;
    } else {
      fkeep[f] = 1;
    }
    pm = fm;
    ph = fh;
  }
  if (dups) atomicAdd(info + kSimDuplicates, dups);
}

__global__ __launch_bounds__(kSimThreads) void k_simplify_emit(const int32_t *faces, int64_t nf,
                                                               const int32_t *fbase,
                                                               const int32_t *vmap,
                                                               int32_t *fout, int32_t *fmap) {
  const int64_t f = sim_lane();
  if (f >= nf) return;
  const int at = fbase[f];
  if (fbase[f + 1] == at) return;
  fmap[f] = at;
#pragma unroll
  for (int k = 0; k < 3; ++k) fout[3 * static_cast<int64_t>(at) + k] = vmap[faces[3 * f + k]];
}

}  // namespace rsd

namespace {

static_assert(RS_SIMPLIFY_TIMING_SLOTS == 4, "cluster, rows, quadric, faces");
static_assert(3 * RS_MESH_MAX_FACES <= INT32_MAX, "the corner rows' offsets are int32");
static_assert(RS_SIMPLIFY_MAX_CELLS <= INT32_MAX, "a cell key is an int32");

// the rows of `n` items (bucket[i] < nb, or -1; the row holds i / per): off[0 .. nb] the
// offsets, rows the items in arrival order.  off and cursor are adjacent: one memset.
int simplify_rows(hipStream_t s, const int32_t *bucket, int64_t n, int per, int64_t nb,
                   int32_t *off, size_t off_and_cursor_bytes, int32_t *cursor, int32_t *sums,
                   int32_t *rows) {
  HIP_TRY(hipMemsetAsync(off, 0, off_and_cursor_bytes, s));
  const dim3 block(rsd::kSimThreads), grid(rs::blocks(n, rsd::kSimThreads));
  if (n) hipLaunchKernelGGL(rsd::k_simplify_count, grid, block, 0, s, bucket, n, off);
  rs::mesh_scan(s, off, nb, sums);
  if (n)
    hipLaunchKernelGGL(rsd::k_simplify_scatter, grid, block, 0, s, bucket, n, per, off, cursor,
                       rows);
  return RS_OK;
}

}  // namespace

extern "C" int rs_mesh_simplify(rs_ctx *c, const double *vertices, int64_t nv,
                                const int32_t *faces, int64_t nf, const double *origin,
                                double cell, const int64_t *dims, int32_t placement,
                                double rank_tol, double *vertices_out, int64_t vcap,
                                int32_t *faces_out, int64_t fcap, int32_t *vmap, int32_t *fmap,
                                double *quadrics_out, int64_t *nv_out, int64_t *nf_out,
                                rs_simplify_info *info) {
  if (nv_out) *nv_out = 0;
  if (nf_out) *nf_out = 0;
  int st = rs::mesh_check(c, faces, nf, nv);
  if (st) return st;
  if (!nv_out || !nf_out || !info || !origin || !dims || (nv > 0 && (!vertices || !vmap)) ||
      (nf > 0 && !fmap))
    return fail(RS_EINVAL, "null pointer");
  if (vcap < 0 || fcap < 0 || (vcap > 0 && !vertices_out) || (fcap > 0 && !faces_out))
    return fail(RS_EINVAL, "a capacity is negative or its array is null");
  if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
    return fail(RS_EINVAL, "origin must be finite");
  if (!std::isfinite(cell) || !(cell > 0.0))
    return fail(RS_EINVAL, "cell must be finite and positive");
  int64_t ncell = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1) return fail(RS_EINVAL, "every dim must be at least 1");
    if (dims[a] > RS_SIMPLIFY_MAX_CELLS || (ncell *= dims[a]) > RS_SIMPLIFY_MAX_CELLS)
      return fail(RS_EINVAL, "a grid of more than 2^27 cells");
  }
  if (placement != RS_SIMPLIFY_MEAN && placement != RS_SIMPLIFY_QUADRIC)
    return fail(RS_EINVAL, "placement must be 0 (mean) or 1 (quadric)");
  if (!(rank_tol >= 0.0 && rank_tol < 1.0)) return fail(RS_EINVAL, "rank_tol must be in [0, 1)");
  for (int64_t k = 0; k < 3 * nv; ++k) {
    if (!std::isfinite(vertices[k])) return fail(RS_EINVAL, "the vertices must be finite");
    const double i = std::floor((vertices[k] - origin[k % 3]) / cell);
    if (!(i >= 0.0 && i <= static_cast<double>(dims[k % 3] - 1)))
      return fail(RS_EINVAL, "a vertex lies outside the grid");
  }
  if (nv == 0) {   // and nf == 0: no index is in range
    *info = rs_simplify_info{0, 0, 0, 0, 0};
    return RS_OK;
  }

  const size_t n = static_cast<size_t>(nv), m = static_cast<size_t>(nf);
  const size_t items = n > 3 * m ? n : 3 * m;
  rs::Layout L;  // [vertices | faces] go up; the rest is the device's
  const auto b_vert = L.add<double>(3 * n);
  const auto b_face = L.add<int32_t>(3 * m);
  const auto b_cell = L.add<int32_t>(static_cast<size_t>(ncell) + 1);
  const auto b_csums = L.add<int32_t>(rs::blocks(ncell, RS_MESH_SCAN_CHUNK) + 1);
  const auto b_key = L.add<int32_t>(n), b_ckey = L.add<int32_t>(n);
  const auto b_vmap = L.add<int32_t>(n);
  const auto b_off = L.add<int32_t>(n + 1), b_cursor = L.add<int32_t>(n);
  const auto b_sums = L.add<int32_t>(rs::blocks(nv, RS_MESH_SCAN_CHUNK) + 1);
  const auto b_cbucket = L.add<int32_t>(3 * m), b_fbucket = L.add<int32_t>(m);
  const auto b_rows = L.add<int32_t>(items);
  const auto b_fkey = L.add<int32_t>(2 * m);
  const auto b_fbase = L.add<int32_t>(m + 1);
  const auto b_fsums = L.add<int32_t>(rs::blocks(nf, RS_MESH_SCAN_CHUNK) + 1);
  const auto b_info = L.add<int32_t>(rsd::kSimInfoWords);
  const auto b_plane = L.add<double>(4 * m);
  const auto b_mean = L.add<double>(3 * n), b_quad = L.add<double>(10 * n);
  const auto b_pos = L.add<double>(3 * n);
  const auto b_fmap = L.add<int32_t>(m), b_fout = L.add<int32_t>(3 * m);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_vert.dev(), vertices, b_vert.bytes, hipMemcpyHostToDevice, s));
  if (nf) HIP_TRY(hipMemcpyAsync(b_face.dev(), faces, b_face.bytes, hipMemcpyHostToDevice, s));

  rsd::SimGrid G;
  for (int a = 0; a < 3; ++a) G.origin[a] = origin[a];
  G.cell = cell;
  G.d0 = static_cast<int>(dims[0]);
  G.d1 = static_cast<int>(dims[1]);
  const dim3 block(rsd::kSimThreads);
  const dim3 vgrid(rs::blocks(nv, rsd::kSimThreads)), fgrid(rs::blocks(nf, rsd::kSimThreads));
  const int32_t *d_ncl = b_cell.dev() + ncell;   // the scan's total: the number of clusters
  const size_t off_and_cursor = L.span(b_off, b_sums);
  auto &T = c->simplify;

  // cluster
  if ((st = T.mark(0, s))) return st;
  HIP_TRY(hipMemsetAsync(b_cell.dev(), 0, b_cell.bytes, s));
  HIP_TRY(hipMemsetAsync(b_info.dev(), 0, b_info.bytes, s));
  hipLaunchKernelGGL(rsd::k_simplify_keys, vgrid, block, 0, s, b_vert.dev(), nv, G, b_key.dev(),
                     b_cell.dev());
  rs::mesh_scan(s, b_cell.dev(), ncell, b_csums.dev());
  hipLaunchKernelGGL(rsd::k_simplify_vmap, vgrid, block, 0, s, b_key.dev(), nv, b_cell.dev(),
                     b_vmap.dev(), b_ckey.dev());
  HIP_TRY(hipGetLastError());
  // rows: the vertices of a cluster and its mean, then the planes and the corners of a cluster
  if ((st = T.mark(1, s))) return st;
  if ((st = simplify_rows(s, b_vmap.dev(), nv, 1, nv, b_off.dev(), off_and_cursor,
                          b_cursor.dev(), b_sums.dev(), b_rows.dev())))
    return st;
  hipLaunchKernelGGL(rsd::k_simplify_mean, vgrid, block, 0, s, b_off.dev(), d_ncl, b_rows.dev(),
                     b_vert.dev(), b_mean.dev(), b_info.dev());
  if (nf)
    hipLaunchKernelGGL(rsd::k_simplify_faces, fgrid, block, 0, s, b_vert.dev(), b_face.dev(), nf,
                       b_vmap.dev(), b_plane.dev(), b_cbucket.dev(), b_fbucket.dev(),
                       b_fkey.dev(), b_fmap.dev(), b_info.dev());
  if ((st = simplify_rows(s, b_cbucket.dev(), 3 * nf, 3, nv, b_off.dev(), off_and_cursor,
                          b_cursor.dev(), b_sums.dev(), b_rows.dev())))
    return st;
  HIP_TRY(hipGetLastError());
  // quadric and solve
  if ((st = T.mark(2, s))) return st;
  hipLaunchKernelGGL(rsd::k_simplify_quadric, vgrid, block, 0, s, b_off.dev(), d_ncl,
                     b_rows.dev(), b_plane.dev(), b_mean.dev(), b_ckey.dev(), G,
                     static_cast<int>(placement), rank_tol, b_quad.dev(), b_pos.dev(),
                     b_info.dev());
  HIP_TRY(hipGetLastError());
  // faces
  if ((st = T.mark(3, s))) return st;
  if (nf) {
    if ((st = simplify_rows(s, b_fbucket.dev(), nf, 1, nv, b_off.dev(), off_and_cursor,
                            b_cursor.dev(), b_sums.dev(), b_rows.dev())))
      return st;
    HIP_TRY(hipMemsetAsync(b_fbase.dev(), 0, b_fbase.bytes, s));
    hipLaunchKernelGGL(rsd::k_simplify_dups, vgrid, block, 0, s, b_off.dev(), d_ncl,
                       b_rows.dev(), b_fkey.dev(), b_fbase.dev(), b_fmap.dev(), b_info.dev());
    rs::mesh_scan(s, b_fbase.dev(), nf, b_fsums.dev());
    hipLaunchKernelGGL(rsd::k_simplify_emit, fgrid, block, 0, s, b_face.dev(), nf,
                       b_fbase.dev(), b_vmap.dev(), b_fout.dev(), b_fmap.dev());
  }
  HIP_TRY(hipGetLastError());
  if ((st = T.mark(4, s))) return st;

  int32_t ncl = 0, nkept = 0, words[rsd::kSimInfoWords] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(&ncl, d_ncl, sizeof(ncl), hipMemcpyDeviceToHost, s));
  if (nf)
    HIP_TRY(hipMemcpyAsync(&nkept, b_fbase.dev() + m, sizeof(nkept), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(words, b_info.dev(), sizeof(words), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < RS_SIMPLIFY_TIMING_SLOTS; ++k)
    if ((st = T.read(k, k, k + 1))) return st;
  *nv_out = ncl;
  *nf_out = nkept;
  if (*nv_out > vcap || *nf_out > fcap)
    return fail(RS_EINVAL,
                "the result does not fit the capacities (nv_out and nf_out state its size)");

  HIP_TRY(hipMemcpyAsync(vertices_out, b_pos.dev(), sizeof(double) * 3 * ncl,
                         hipMemcpyDeviceToHost, s));
  if (quadrics_out)
    HIP_TRY(hipMemcpyAsync(quadrics_out, b_quad.dev(), sizeof(double) * 10 * ncl,
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(vmap, b_vmap.dev(), b_vmap.bytes, hipMemcpyDeviceToHost, s));
  if (nf) HIP_TRY(hipMemcpyAsync(fmap, b_fmap.dev(), b_fmap.bytes, hipMemcpyDeviceToHost, s));
  if (nkept)
    HIP_TRY(hipMemcpyAsync(faces_out, b_fout.dev(), sizeof(int32_t) * 3 * nkept,
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *info = rs_simplify_info{ncl, words[rsd::kSimFallbacks], words[rsd::kSimDegenerate],
                           words[rsd::kSimDuplicates], words[rsd::kSimLongest]};
  return RS_OK;
}

extern "C" int rs_simplify_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->simplify.enable(enable != 0);
  if (st) return st;
  c->simplify.copy_out(ms);
  return RS_OK;
}
