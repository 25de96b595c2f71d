// Mesh clean-up on the GPU: connected components (rs_mesh_components), compaction
// (rs_mesh_compact) and Taubin smoothing (rs_mesh_smooth) of a welded index mesh.  The
// definitions stand in include/rsamd.h; tests/mesh_ref.py restates them in numpy.
//
// Every kernel runs one lane per face or per vertex.
//
//   k_mesh_init           parent[v] = v
//   k_mesh_hook           per face, edges (a, b) and (a, c).  A round begins with every parent a
//                         root.  The lane reads the two ends' parents, no further, and where
//                         they differ puts the larger under the smaller with atomicMin: a root
//                         ends the round under the smallest root any of its edges leads to.
//                         There is no loop and no lane waits for another; a read that sees a
//                         minimum which has landed already sees a vertex further down the same
//                         tree, which is as good.  parent[v] <= v holds before and after every
//                         write.  (A first version walked to the current roots inside this
//                         kernel, to merge more per round; every walk then ended on the same
//                         few addresses and the first round took 4 to 8 ms on the benchmark
//                         mesh)
//   k_mesh_jump           per vertex: parent[v] = parent[parent[v]] until the parent is a root.
//                         Roots do not change in this kernel and every value a lane reads is an
//                         ancestor, so the walk strictly decreases and ends after at most v
//                         steps whatever the other lanes do; it ends sooner where the lanes
//                         ahead have shortened their paths already (pointer doubling when the
//                         waves run side by side).  Afterwards every parent is a root.
//   k_mesh_face_count     faces per root, integer atomicAdd: one per run of waves of a 1024-lane
//                         workgroup that lie in one component, one per lane in a wave that
//                         spans components
//   k_mesh_sizes          size[v] = faces[root of v]; the roots are counted
//   k_mesh_keep_flags     compaction: 0 / 1 per vertex and per face
//   k_mesh_scan_*         exclusive scan of int32 counts in place, the shape of the surface
//                         stage's scans: every workgroup scans its chunk of 2048, one workgroup
//                         scans the chunk sums, every chunk adds its offset
//   k_mesh_compact_*      kept vertices and faces to their scanned offsets, vmap
//   k_mesh_degree         smoothing: 2 row entries per face corner, counted with atomicAdd
//   k_mesh_scatter        the other two corners into the vertex's row through an atomic cursor
//   k_mesh_rows           per vertex: sort the row (insertion, heap sort above 24 entries, both
//                         in place in global memory), read the boundary flag off the runs, drop
//                         duplicates and the vertex itself, write degree and fixed flag
//   k_mesh_smooth_pass    per vertex: the ascending sum over the row, fp64, no contraction
// Every global index is bounded: a face index has passed the host's range check before any
// launch; a walk reads parent only at values parent holds, all in 0..nv - 1; a row is written at
// off[v] + cursor < off[v + 1], because the cursor counts exactly the corners the degree kernel
// counted; the scans touch only [0, n]; the compaction writes below the scanned totals, which
// the host has compared with the capacities before the emit kernels are launched.
#include <hip/hip_runtime.h>

#include <cmath>

#include "host.h"

namespace rsd {

constexpr int kMeshThreads = 256;
constexpr int kMeshCountThreads = 1024;   // k_mesh_face_count: 16 waves share one atomicAdd
constexpr int kMeshScanItems = 8;
constexpr int kMeshScanChunk = kMeshThreads * kMeshScanItems;
constexpr int kMeshInsertionMax = 24;   // longer rows are heap-sorted
static_assert(kMeshScanChunk == RS_MESH_SCAN_CHUNK, "the header states the scan's chunk");

__device__ __forceinline__ int64_t mesh_lane() {
  return static_cast<int64_t>(blockIdx.x) * kMeshThreads + threadIdx.x;
}

// parent is read and written by many lanes of one kernel: relaxed, device-wide
__device__ __forceinline__ int mesh_load(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void mesh_store(int32_t *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_init(int32_t *parent, int64_t nv) {
  const int64_t v = mesh_lane();
  if (v < nv) parent[v] = static_cast<int32_t>(v);
}

// ru and rv are the roots the round began with, or, where another lane's minimum has landed
// already, vertices further down: in either case ru <= u and rv <= v are connected to them.
__device__ __forceinline__ void mesh_hook(int32_t *parent, int u, int v, int32_t *changed) {
  if (u == v) return;
  const int ru = parent[u], rv = parent[v];
  if (ru == rv) return;
  atomicMin(parent + (ru > rv ? ru : rv), ru > rv ? rv : ru);
  *changed = 1;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_hook(const int32_t *faces, int64_t nf,
                                                            int32_t *parent, int32_t *changed) {
  const int64_t f = mesh_lane();
  if (f >= nf) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  mesh_hook(parent, a, b, changed);
  mesh_hook(parent, a, c, changed);
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_jump(int32_t *parent, int64_t nv) {
  const int64_t t = mesh_lane();
  if (t >= nv) return;
  const int v = static_cast<int>(t);
  int p = mesh_load(parent + v);
  if (p == v) return;
  for (;;) {
    const int pp = mesh_load(parent + p);
    if (static_cast<unsigned>(pp) >= static_cast<unsigned>(p)) break;   // p is a root
    mesh_store(parent + v, pp);
    p = pp;
  }
}

// Faces arrive component by component more often than not, and then every atomicAdd of a
// workgroup would go to one address.  A wave that lies in one component leaves (root, faces) in
// LDS, and thread 0 adds the runs of equal roots among the workgroup's 16 waves; a wave that
// spans components adds lane by lane.
__global__ __launch_bounds__(kMeshCountThreads) void k_mesh_face_count(const int32_t *faces,
                                                                       int64_t nf,
                                                                       const int32_t *parent,
                                                                       int32_t *fcount) {
  __shared__ int s_root[kMeshCountThreads / 64], s_faces[kMeshCountThreads / 64];
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kMeshCountThreads + threadIdx.x;
  const bool in = f < nf;
  const int r = in ? parent[faces[3 * f]] : -1;
  const int r0 = __shfl(r, 0);   // lane 0 is inside whenever a lane of its wave is
  const unsigned long long all = __ballot(in), odd = __ballot(in && r != r0);
  if (odd != 0 && in) atomicAdd(fcount + r, 1);
  if ((threadIdx.x & 63) == 0) {
    s_root[threadIdx.x >> 6] = r0;
    s_faces[threadIdx.x >> 6] = odd == 0 ? __popcll(all) : 0;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int root = -1, sum = 0;
  for (int w = 0; w < kMeshCountThreads / 64; ++w) {
    if (s_faces[w] == 0) continue;   // an empty wave, or one that has added lane by lane
    if (s_root[w] != root) {
      if (sum) atomicAdd(fcount + root, sum);
      root = s_root[w];
      sum = 0;
    }
    sum += s_faces[w];
  }
  if (sum) atomicAdd(fcount + root, sum);
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_sizes(const int32_t *parent, int64_t nv,
                                                             const int32_t *fcount,
                                                             int32_t *size, int32_t *count) {
  const int64_t v = mesh_lane();
  const bool in = v < nv;
  const int r = in ? parent[v] : -1;
  if (in) size[v] = fcount[r];
  const unsigned long long roots = __ballot(in && r == v);
  if ((threadIdx.x & 63) == 0 && roots) atomicAdd(count, __popcll(roots));
}

// ------------------------------------------------------------------------------------------
// exclusive scan of int32 in place: v[0 .. n) become offsets, v[n] the total
// ------------------------------------------------------------------------------------------
// Exclusive scan of one chunk held in registers (kMeshScanItems per thread, 0 past the end),
// started at `carry`; returns the chunk's sum.  All threads call it together.
__device__ __forceinline__ int mesh_scan_chunk(const int (&x)[kMeshScanItems], int32_t *out,
                                               int64_t base, int64_t end, int carry, int *lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int sum = 0;
#pragma unroll
  for (int k = 0; k < kMeshScanItems; ++k) sum += x[k];
  int incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kMeshThreads / 64; ++w) {
    if (w < wave) before += lds[w];
    all += lds[w];
  }
  int run = carry + before + incl - sum;
#pragma unroll
  for (int k = 0; k < kMeshScanItems; ++k) {
    if (base + k < end) out[base + k] = run;
    run += x[k];
  }
  __syncthreads();
  return all;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_scan_chunks(int32_t *v, int64_t n,
                                                                   int32_t *sums) {
  __shared__ int lds[kMeshThreads / 64];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kMeshScanChunk +
                       static_cast<int64_t>(threadIdx.x) * kMeshScanItems;
  int x[kMeshScanItems];
#pragma unroll
  for (int k = 0; k < kMeshScanItems; ++k) x[k] = base + k < n ? v[base + k] : 0;
  const int total = mesh_scan_chunk(x, v, base, n, 0, lds);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_scan_sums(int32_t *v, int64_t m) {
  __shared__ int lds[kMeshThreads / 64];
  int carry = 0;
  for (int64_t at = 0; at < m; at += kMeshScanChunk) {
    const int64_t base = at + static_cast<int64_t>(threadIdx.x) * kMeshScanItems;
    int x[kMeshScanItems];
#pragma unroll
    for (int k = 0; k < kMeshScanItems; ++k) x[k] = base + k < m ? v[base + k] : 0;
    carry += mesh_scan_chunk(x, v, base, m, carry, lds);
  }
  if (threadIdx.x == 0) v[m] = carry;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_scan_add(int32_t *v, int64_t n,
                                                                const int32_t *sums,
                                                                int nchunks) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kMeshScanChunk +
                       static_cast<int64_t>(threadIdx.x) * kMeshScanItems;
  const int add = sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kMeshScanItems; ++k)
    if (base + k < n) v[base + k] += add;
  if (blockIdx.x == 0 && threadIdx.x == 0) v[n] = sums[nchunks];
}

// ------------------------------------------------------------------------------------------
// compaction
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshThreads) void k_mesh_keep_flags(const uint8_t *keep,
                                                                  int64_t nv,
                                                                  const int32_t *faces,
                                                                  int64_t nf, int32_t *vflag,
                                                                  int32_t *fflag) {
  const int64_t t = mesh_lane();
  if (t < nv) vflag[t] = keep[t] ? 1 : 0;
  if (t < nf)
    fflag[t] = keep[faces[3 * t]] && keep[faces[3 * t + 1]] && keep[faces[3 * t + 2]] ? 1 : 0;
}

// vbase and fbase are the scanned flags: an element is kept iff its successor's offset is larger
__global__ __launch_bounds__(kMeshThreads) void k_mesh_compact_vertices(const double *vin,
                                                                        int64_t nv,
                                                                        const int32_t *vbase,
                                                                        double *vout,
                                                                        int32_t *vmap) {
  const int64_t v = mesh_lane();
  if (v >= nv) return;
  const int at = vbase[v];
  const bool kept = vbase[v + 1] > at;
  vmap[v] = kept ? at : -1;
  if (!kept) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) vout[3 * static_cast<int64_t>(at) + k] = vin[3 * v + k];
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_compact_faces(const int32_t *fin,
                                                                     int64_t nf,
                                                                     const int32_t *fbase,
                                                                     const int32_t *vbase,
                                                                     int32_t *fout) {
  const int64_t f = mesh_lane();
  if (f >= nf) return;
  const int at = fbase[f];
  if (fbase[f + 1] == at) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) fout[3 * static_cast<int64_t>(at) + k] = vbase[fin[3 * f + k]];
}

// ------------------------------------------------------------------------------------------
// smoothing
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshThreads) void k_mesh_degree(const int32_t *faces, int64_t nf,
                                                              int32_t *off) {
  const int64_t f = mesh_lane();
  if (f >= nf) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) atomicAdd(off + faces[3 * f + k], 2);
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_scatter(const int32_t *faces, int64_t nf,
                                                               const int32_t *off,
                                                               int32_t *cursor, int32_t *adj) {
  const int64_t f = mesh_lane();
  if (f >= nf) return;
  const int a[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int v = a[k];
    const int64_t at = static_cast<int64_t>(off[v]) + atomicAdd(cursor + v, 2);
    adj[at] = a[(k + 1) % 3];
    adj[at + 1] = a[(k + 2) % 3];
  }
}

__device__ __forceinline__ void mesh_sift(int32_t *row, int start, int end) {
  int root = start;
  const int x = row[root];
  for (;;) {
    int child = 2 * root + 1;
    if (child >= end) break;
    int cv = row[child];
    if (child + 1 < end) {
      const int c2 = row[child + 1];
      if (c2 > cv) {
        cv = c2;
        ++child;
      }
    }
    if (cv <= x) break;
    row[root] = cv;
    root = child;
  }
  row[root] = x;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_rows(const int32_t *off, int64_t nv,
                                                            int32_t *adj, const uint8_t *fixed,
                                                            int pin, int32_t *deg,
                                                            uint8_t *fixedf) {
  const int64_t t = mesh_lane();
  if (t >= nv) return;
  const int v = static_cast<int>(t);
  int32_t *row = adj + off[t];
  const int d = off[t + 1] - off[t];
  if (d <= kMeshInsertionMax) {
    for (int i = 1; i < d; ++i) {
      const int x = row[i];
      int j = i;
      while (j > 0 && row[j - 1] > x) {
        row[j] = row[j - 1];
        --j;
      }
      row[j] = x;
    }
  } else {
    for (int i = d / 2 - 1; i >= 0; --i) mesh_sift(row, i, d);
    for (int end = d - 1; end > 0; --end) {
      const int top = row[0];
      row[0] = row[end];
      row[end] = top;
      mesh_sift(row, 0, end);
    }
  }
  bool boundary = false;
  int w = 0;
  for (int i = 0; i < d;) {
    const int u = row[i];
    int j = i + 1;
    while (j < d && row[j] == u) ++j;
    if (u != v) {
      boundary |= j - i == 1;
      row[w++] = u;
    }
    i = j;
  }
  deg[t] = w;
  fixedf[t] = (fixed && fixed[t]) || (pin && boundary) ? 1 : 0;
}

__global__ __launch_bounds__(kMeshThreads) void k_mesh_smooth_pass(
    const double *xin, int64_t nv, const int32_t *off, const int32_t *adj, const int32_t *deg,
    const uint8_t *fixedf, double f, double *xout) {
#pragma clang fp contract(off)
  const int64_t v = mesh_lane();
  if (v >= nv) return;
  const double x0 = xin[3 * v], x1 = xin[3 * v + 1], x2 = xin[3 * v + 2];
  const int n = deg[v];
  double y0 = x0, y1 = x1, y2 = x2;
  if (n > 0 && !fixedf[v]) {
    const int32_t *row = adj + off[v];
    const double *p = xin + 3 * static_cast<int64_t>(row[0]);
    double s0 = p[0], s1 = p[1], s2 = p[2];
    for (int i = 1; i < n; ++i) {
      p = xin + 3 * static_cast<int64_t>(row[i]);
      s0 += p[0];
      s1 += p[1];
      s2 += p[2];
    }
    const double dn = static_cast<double>(n);
    y0 = x0 + f * (s0 / dn - x0);
    y1 = x1 + f * (s1 / dn - x1);
    y2 = x2 + f * (s2 / dn - x2);
  }
  xout[3 * v] = y0;
  xout[3 * v + 1] = y1;
  xout[3 * v + 2] = y2;
}

}  // namespace rsd

static_assert(RS_MESH_TIMING_SLOTS == 4, "components, compact, adjacency, smooth");
static_assert(6 * RS_MESH_MAX_FACES <= INT32_MAX, "the adjacency offsets are int32");

namespace rs {

// the argument rules every mesh call shares (rs_mesh_simplify of simplify.hip too)
int mesh_check(const rs_ctx *c, const int32_t *faces, int64_t nf, int64_t nv) {
  if (!c) return fail(RS_EINVAL, "null pointer");
  if (nv < 0 || nf < 0) return fail(RS_EINVAL, "negative size");
  if (nv > RS_MESH_MAX_VERTICES || nf > RS_MESH_MAX_FACES)
    return fail(RS_EINVAL, "more than 2^27 vertices or faces");
  if (nf > 0 && !faces) return fail(RS_EINVAL, "null pointer");
  for (int64_t k = 0; k < 3 * nf; ++k)
    if (faces[k] < 0 || faces[k] >= nv) return fail(RS_EINVAL, "a face index is out of range");
  return RS_OK;
}

// the exclusive scan of v[0 .. n) in place, the total in v[n]; sums holds nchunks + 1 items
void mesh_scan(hipStream_t s, int32_t *v, int64_t n, int32_t *sums) {
  const int nchunks = static_cast<int>(rs::blocks(n, rsd::kMeshScanChunk));
  const dim3 block(rsd::kMeshThreads), grid(static_cast<unsigned>(nchunks));
  hipLaunchKernelGGL(rsd::k_mesh_scan_chunks, grid, block, 0, s, v, n, sums);
  hipLaunchKernelGGL(rsd::k_mesh_scan_sums, dim3(1), block, 0, s, sums,
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_mesh_scan_add, grid, block, 0, s, v, n, sums, nchunks);
}

}  // namespace rs

using rs::mesh_check;
using rs::mesh_scan;

extern "C" int rs_mesh_components(rs_ctx *c, const int32_t *faces, int64_t nf, int64_t nv,
                                  int32_t *label, int32_t *size, int64_t *count,
                                  int32_t *rounds) {
  if (count) *count = 0;
  if (rounds) *rounds = 0;
  int st = mesh_check(c, faces, nf, nv);
  if (st) return st;
  if (!count || !rounds || (nv > 0 && (!label || !size))) return fail(RS_EINVAL, "null pointer");
  if (nv == 0) return RS_OK;
  if (nf == 0) {   // every vertex is its own component; nothing to launch
    for (int64_t v = 0; v < nv; ++v) {
      label[v] = static_cast<int32_t>(v);
      size[v] = 0;
    }
    *count = nv;
    return RS_OK;
  }

  const size_t n = static_cast<size_t>(nv);
  rs::Layout L;  // [faces] goes up, [parent | size | flags] come down
  const auto b_face = L.add<int32_t>(3 * static_cast<size_t>(nf));
  const auto b_parent = L.add<int32_t>(n), b_size = L.add<int32_t>(n);
  const auto b_flags = L.add<int32_t>(2);   // changed, count
  const auto b_fcount = L.add<int32_t>(n);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_face.dev(), faces, b_face.bytes, hipMemcpyHostToDevice, s));
  const dim3 block(rsd::kMeshThreads);
  const dim3 vgrid(rs::blocks(nv, rsd::kMeshThreads)), fgrid(rs::blocks(nf, rsd::kMeshThreads));
  if (c->mesh.on) c->mesh.ms[0] = 0.0;
  int r = 1;
  for (;; ++r) {
    int32_t changed = 0;
    if ((st = c->mesh.mark(0, s))) return st;
    if (r == 1)
      hipLaunchKernelGGL(rsd::k_mesh_init, vgrid, block, 0, s, b_parent.dev(), nv);
    else
      hipLaunchKernelGGL(rsd::k_mesh_jump, vgrid, block, 0, s, b_parent.dev(), nv);
    HIP_TRY(hipMemsetAsync(b_flags.dev(), 0, b_flags.bytes, s));
    hipLaunchKernelGGL(rsd::k_mesh_hook, fgrid, block, 0, s, b_face.dev(), nf, b_parent.dev(),
                       b_flags.dev());
    HIP_TRY(hipGetLastError());
    if ((st = c->mesh.mark(1, s))) return st;
    HIP_TRY(hipMemcpyAsync(&changed, b_flags.dev(), sizeof(changed), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((st = c->mesh.add(0, 0, 1))) return st;
    if (!changed) break;
    if (r == RS_MESH_MAX_ROUNDS)
      return fail(RS_EDEVICE, "rs_mesh_components: RS_MESH_MAX_ROUNDS = 64 hook rounds did not "
                              "join the components");
  }
  *rounds = r;

  // the last round hooked nothing, so parent still is what the jump before it left: all roots
  int32_t ncomp = 0;
  if ((st = c->mesh.mark(0, s))) return st;
  HIP_TRY(hipMemsetAsync(b_fcount.dev(), 0, b_fcount.bytes, s));
  hipLaunchKernelGGL(rsd::k_mesh_face_count, dim3(rs::blocks(nf, rsd::kMeshCountThreads)),
                     dim3(rsd::kMeshCountThreads), 0, s, b_face.dev(), nf, b_parent.dev(),
                     b_fcount.dev());
  hipLaunchKernelGGL(rsd::k_mesh_sizes, vgrid, block, 0, s, b_parent.dev(), nv, b_fcount.dev(),
                     b_size.dev(), b_flags.dev() + 1);
  HIP_TRY(hipGetLastError());
  if ((st = c->mesh.mark(1, s))) return st;
  HIP_TRY(hipMemcpyAsync(label, b_parent.dev(), b_parent.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(size, b_size.dev(), b_size.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&ncomp, b_flags.dev() + 1, sizeof(ncomp), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *count = ncomp;
  return c->mesh.add(0, 0, 1);
}

extern "C" int rs_mesh_compact(rs_ctx *c, const double *vertices, int64_t nv,
                               const int32_t *faces, int64_t nf, const uint8_t *keep,
                               double *vertices_out, int64_t vcap, int32_t *faces_out,
                               int64_t fcap, int32_t *vmap, int64_t *nv_out, int64_t *nf_out) {
  if (nv_out) *nv_out = 0;
  if (nf_out) *nf_out = 0;
  int st = mesh_check(c, faces, nf, nv);
  if (st) return st;
  if (!nv_out || !nf_out || (nv > 0 && (!vertices || !keep)))
    return fail(RS_EINVAL, "null pointer");
  if (vcap < 0 || fcap < 0 || (vcap > 0 && !vertices_out) || (fcap > 0 && !faces_out))
    return fail(RS_EINVAL, "a capacity is negative or its array is null");
  if (nv == 0) return RS_OK;   // and nf == 0: no index is in range

  const size_t n = static_cast<size_t>(nv), m = static_cast<size_t>(nf);
  const size_t vchunks = rs::blocks(nv, rsd::kMeshScanChunk);
  const size_t fchunks = rs::blocks(nf, rsd::kMeshScanChunk);
  const size_t vroom = static_cast<size_t>(vcap) < n ? static_cast<size_t>(vcap) : n;
  const size_t froom = static_cast<size_t>(fcap) < m ? static_cast<size_t>(fcap) : m;
  rs::Layout L;  // [keep | faces | vertices] go up, [vmap | vertices | faces] come down
  const auto b_keep = L.add<uint8_t>(n);
  const auto b_face = L.add<int32_t>(3 * m);
  const auto b_vert = L.add<double>(3 * n);
  const auto b_vbase = L.add<int32_t>(n + 1), b_fbase = L.add<int32_t>(m + 1);
  const auto b_vsums = L.add<int32_t>(vchunks + 1), b_fsums = L.add<int32_t>(fchunks + 1);
  const auto b_vmap = L.add<int32_t>(n);
  const auto b_vout = L.add<double>(3 * vroom);
  const auto b_fout = L.add<int32_t>(3 * froom);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_keep.dev(), keep, b_keep.bytes, hipMemcpyHostToDevice, s));
  if (nf) HIP_TRY(hipMemcpyAsync(b_face.dev(), faces, b_face.bytes, hipMemcpyHostToDevice, s));
  const dim3 block(rsd::kMeshThreads);
  const dim3 vgrid(rs::blocks(nv, rsd::kMeshThreads)), fgrid(rs::blocks(nf, rsd::kMeshThreads));
  if (c->mesh.on) c->mesh.ms[1] = 0.0;
  if ((st = c->mesh.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_mesh_keep_flags, dim3(rs::blocks(nv > nf ? nv : nf, rsd::kMeshThreads)),
                     block, 0, s, b_keep.dev(), nv, b_face.dev(), nf, b_vbase.dev(),
                     b_fbase.dev());
  mesh_scan(s, b_vbase.dev(), nv, b_vsums.dev());
  int32_t totals[2] = {0, 0};
  if (nf) mesh_scan(s, b_fbase.dev(), nf, b_fsums.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->mesh.mark(1, s))) return st;
  HIP_TRY(hipMemcpyAsync(&totals[0], b_vbase.dev() + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (nf)
    HIP_TRY(hipMemcpyAsync(&totals[1], b_fbase.dev() + m, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->mesh.add(1, 0, 1))) return st;
  *nv_out = totals[0];
  *nf_out = totals[1];
  if (*nv_out > vcap || *nf_out > fcap)
    return fail(RS_EINVAL,
                "the result does not fit the capacities (nv_out and nf_out state its size)");

  HIP_TRY(hipMemcpyAsync(b_vert.dev(), vertices, b_vert.bytes, hipMemcpyHostToDevice, s));
  if ((st = c->mesh.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_mesh_compact_vertices, vgrid, block, 0, s, b_vert.dev(), nv,
                     b_vbase.dev(), b_vout.dev(), b_vmap.dev());
  if (*nf_out)
    hipLaunchKernelGGL(rsd::k_mesh_compact_faces, fgrid, block, 0, s, b_face.dev(), nf,
                       b_fbase.dev(), b_vbase.dev(), b_fout.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->mesh.mark(1, s))) return st;
  if (vmap) HIP_TRY(hipMemcpyAsync(vmap, b_vmap.dev(), b_vmap.bytes, hipMemcpyDeviceToHost, s));
  if (*nv_out)
    HIP_TRY(hipMemcpyAsync(vertices_out, b_vout.dev(), sizeof(double) * 3 * *nv_out,
                           hipMemcpyDeviceToHost, s));
  if (*nf_out)
    HIP_TRY(hipMemcpyAsync(faces_out, b_fout.dev(), sizeof(int32_t) * 3 * *nf_out,
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return c->mesh.add(1, 0, 1);
}

extern "C" int rs_mesh_smooth(rs_ctx *c, const double *vertices, int64_t nv,
                              const int32_t *faces, int64_t nf, int32_t iterations,
                              double lambda, double mu, const uint8_t *fixed,
                              int32_t pin_boundary, double *out) {
  int st = mesh_check(c, faces, nf, nv);
  if (st) return st;
  if (nv > 0 && (!vertices || !out)) return fail(RS_EINVAL, "null pointer");
  if (iterations < 0 || iterations > RS_MESH_MAX_ITERATIONS)
    return fail(RS_EINVAL, "iterations must be in 0..65536");
  if (!std::isfinite(lambda) || !std::isfinite(mu))
    return fail(RS_EINVAL, "lambda and mu must be finite");
  for (int64_t k = 0; k < 3 * nv; ++k)
    if (!std::isfinite(vertices[k])) return fail(RS_EINVAL, "the vertices must be finite");
  if (nv == 0) return RS_OK;
  if (nf == 0 || iterations == 0) {   // nothing moves: the input bits
    if (out != vertices)
      for (int64_t k = 0; k < 3 * nv; ++k) out[k] = vertices[k];
    return RS_OK;
  }

  const size_t n = static_cast<size_t>(nv), m = static_cast<size_t>(nf);
  const size_t nchunks = rs::blocks(nv, rsd::kMeshScanChunk);
  rs::Layout L;  // [faces | fixed | x0] go up, x0 or x1 comes down
  const auto b_face = L.add<int32_t>(3 * m);
  const auto b_fixed = L.add<uint8_t>(fixed ? n : 0);
  const auto b_x0 = L.add<double>(3 * n), b_x1 = L.add<double>(3 * n);
  const auto b_off = L.add<int32_t>(n + 1), b_cursor = L.add<int32_t>(n);
  const auto b_sums = L.add<int32_t>(nchunks + 1);
  const auto b_deg = L.add<int32_t>(n);
  const auto b_fixedf = L.add<uint8_t>(n);
  const auto b_adj = L.add<int32_t>(6 * m);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_face.dev(), faces, b_face.bytes, hipMemcpyHostToDevice, s));
  if (fixed)
    HIP_TRY(hipMemcpyAsync(b_fixed.dev(), fixed, b_fixed.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_x0.dev(), vertices, b_x0.bytes, hipMemcpyHostToDevice, s));
  const dim3 block(rsd::kMeshThreads);
  const dim3 vgrid(rs::blocks(nv, rsd::kMeshThreads)), fgrid(rs::blocks(nf, rsd::kMeshThreads));

  if ((st = c->mesh.mark(0, s))) return st;
  HIP_TRY(hipMemsetAsync(b_off.dev(), 0, L.span(b_off, b_sums), s));   // off and cursor
  hipLaunchKernelGGL(rsd::k_mesh_degree, fgrid, block, 0, s, b_face.dev(), nf, b_off.dev());
  mesh_scan(s, b_off.dev(), nv, b_sums.dev());
  hipLaunchKernelGGL(rsd::k_mesh_scatter, fgrid, block, 0, s, b_face.dev(), nf, b_off.dev(),
                     b_cursor.dev(), b_adj.dev());
  hipLaunchKernelGGL(rsd::k_mesh_rows, vgrid, block, 0, s, b_off.dev(), nv, b_adj.dev(),
                     fixed ? b_fixed.dev() : nullptr, pin_boundary ? 1 : 0, b_deg.dev(),
                     b_fixedf.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->mesh.mark(1, s))) return st;
  double *src = b_x0.dev(), *dst = b_x1.dev();
  for (int32_t it = 0; it < 2 * iterations; ++it) {
    hipLaunchKernelGGL(rsd::k_mesh_smooth_pass, vgrid, block, 0, s, src, nv, b_off.dev(),
                       b_adj.dev(), b_deg.dev(), b_fixedf.dev(), it % 2 ? mu : lambda, dst);
    double *t = src;
    src = dst;
    dst = t;
  }
  HIP_TRY(hipGetLastError());
  if ((st = c->mesh.mark(2, s))) return st;
  HIP_TRY(hipMemcpyAsync(out, src, b_x0.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->mesh.read(2, 0, 1))) return st;
  return c->mesh.read(3, 1, 2);
}

extern "C" int rs_mesh_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->mesh.enable(enable != 0);
  if (st) return st;
  c->mesh.copy_out(ms);
  return RS_OK;
}
