// The surface stage on the GPU: depth maps fused into a truncated signed distance volume
// (rs_surface_integrate) and a welded triangle mesh extracted from it by marching tetrahedra
// (rs_surface_extract).  The definitions stand in include/rsamd.h; tests/surface_ref.py restates
// them in numpy.
//
// A volume is indexed [iz, iy, ix] with x fastest; every kernel runs one lane per node, so the 64
// lanes of a wave read 64 consecutive floats of a row and, in k_surface_integrate, project onto
// neighbouring pixels.  A cell is named by its lowest node and shares that node's index; the
// nodes on the upper faces of the volume name no cell.
//
//   k_surface_integrate   a loop over the views, all fp64: project, round, gather one depth (and
//                         one weight), accumulate.  The P rows are read from a device buffer at a
//                         wave-uniform index.  A gather without atomics: the same inputs give the
//                         same bits whatever the launch shape.
//   k_surface_cells       per cell: valid (bit 7) and the number of triangles, 0..12 (bits 0..3)
//   k_surface_nodes       per node: the 7-bit mask of the vertices it owns, from the flags of the
//                         (up to 8) cells around it and the signs of its 7 upper neighbours
//   k_surface_scan*       exclusive scans of popcount(mask) and of the triangle counts: every
//                         workgroup scans its chunk, one workgroup scans the chunk sums, every
//                         chunk adds its offset; a thread's 8 counts are one 8-byte load and its
//                         8 offsets two 16-byte stores
//   k_surface_vertices    vertex base[owner] + popcount(mask[owner] & ((1 << type) - 1))
//   k_surface_faces       per cell, tet by tet through the case table; a vertex id comes from the
//                         base and mask of one of the cell's own 8 nodes
// Every global index is bounded: a depth map is read only at a pixel the bounds test has placed
// in [0, w-1] x [0, h-1]; a neighbour node or cell is read at its own index only where its
// coordinates lie inside the volume, and at the lane's own node otherwise (the classifier's loads
// are unconditional so that they do not wait for each other); the scans move 8 items at once only
// where all 8 lie below the end; and the mesh is written only at offsets below the scanned
// totals, which the host has compared with the capacities before the emit kernels are launched.
#include <hip/hip_runtime.h>

#include <cmath>

#include "host.h"
#include "surface_table.h"

namespace rsd {

constexpr int kSurfThreads = 256;
constexpr int kSurfScanItems = 8;
constexpr int kSurfScanChunk = kSurfThreads * kSurfScanItems;
static_assert(kSurfScanChunk == RS_SURFACE_SCAN_CHUNK, "the header states the scan's chunk");

__constant__ uint8_t c_tet_corner[6][4] = RS_SURFACE_TET_CORNERS;
__constant__ uint8_t c_tet_table[6][16][7] = RS_SURFACE_TET_TABLE;

struct SurfGrid {
  double o[3], voxel;
  int nx, ny, nz;
  int64_t n;   // nx ny nz <= 2^27
};

struct SurfNode {
  int64_t t;
  int ix, iy, iz;
};

__device__ __forceinline__ bool surf_node(const SurfGrid &G, SurfNode *p) {
  p->t = static_cast<int64_t>(blockIdx.x) * kSurfThreads + threadIdx.x;
  if (p->t >= G.n) return false;
  const int t = static_cast<int>(p->t), row = t / G.nx;
  p->ix = t - row * G.nx;
  p->iz = row / G.ny;
  p->iy = row - p->iz * G.ny;
  return true;
}

// the index offset of cell corner c = dx | dy << 1 | dz << 2
__device__ __forceinline__ int64_t surf_corner(const SurfGrid &G, int c) {
  return (c & 1) + static_cast<int64_t>(c >> 1 & 1) * G.nx +
         static_cast<int64_t>(c >> 2) * G.nx * G.ny;
}

__global__ __launch_bounds__(kSurfThreads) void k_surface_integrate(
    const double *depth, const float *wmap, int V, int h, int w, const double *P, SurfGrid G,
    double trunc, int has_prior, float *tsdf, float *weight) {
  SurfNode p;
  if (!surf_node(G, &p)) return;
  const double X0 = G.o[0] + G.voxel * p.ix, X1 = G.o[1] + G.voxel * p.iy,
               X2 = G.o[2] + G.voxel * p.iz;
  const double wm1 = static_cast<double>(w - 1), hm1 = static_cast<double>(h - 1);
  const int64_t hw = static_cast<int64_t>(h) * w;
  double acc = 0.0, wsum = 0.0;
  for (int v = 0; v < V; ++v) {
    const double *Pv = P + 12 * v;
    const double q0 = Pv[0] * X0 + Pv[1] * X1 + Pv[2] * X2 + Pv[3];
    const double q1 = Pv[4] * X0 + Pv[5] * X1 + Pv[6] * X2 + Pv[7];
    const double z = Pv[8] * X0 + Pv[9] * X1 + Pv[10] * X2 + Pv[11];
    const double u = floor(q0 / z + 0.5), r = floor(q1 / z + 0.5);
    if (u >= 0.0 && u <= wm1 && r >= 0.0 && r <= hm1) {   // false for a NaN
      const int64_t at = v * hw + static_cast<int64_t>(r) * w + static_cast<int64_t>(u);
      const double d = depth[at];
      const double wv = wmap ? static_cast<double>(wmap[at]) : 1.0;
      if (isfinite(d) && d * z > 0.0 && isfinite(wv) && wv > 0.0) {
        const double s = fabs(d) - fabs(z);
        if (s >= -trunc) {
          acc += wv * fmin(1.0, s / trunc);
          wsum += wv;
        }
      }
    }
  }
  double W0 = has_prior ? static_cast<double>(weight[p.t]) : 0.0;
  if (!(W0 > 0.0)) W0 = 0.0;
  const double prior = W0 > 0.0 ? W0 * static_cast<double>(tsdf[p.t]) : 0.0;
  const double W = W0 + wsum;
  tsdf[p.t] = W > 0.0 ? static_cast<float>((prior + acc) / W) : __int_as_float(0x7fc00000);
  weight[p.t] = static_cast<float>(W);
}

// bit c of the result: corner c of the cell at node t is negative; *ok: all 8 are usable
__device__ __forceinline__ int surf_cell_signs(const SurfGrid &G, int64_t t, const float *tsdf,
                                               const float *weight, double min_weight,
                                               bool *ok) {
  int neg = 0;
  bool all = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t at = t + surf_corner(G, c);
    const float f = tsdf[at];
    if (weight) {   // no short circuit: the 16 loads of a cell are independent of each other
      const float wt = weight[at];
      all &= isfinite(f) & (static_cast<double>(wt) >= min_weight);
    }
    neg |= (f < 0.0f ? 1 : 0) << c;
  }
  if (ok) *ok = all;
  return neg;
}

__device__ __forceinline__ int surf_tet_code(int k, int neg) {
  int code = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) code |= (neg >> c_tet_corner[k][i] & 1) << i;
  return code;
}

__global__ __launch_bounds__(kSurfThreads) void k_surface_cells(SurfGrid G, const float *tsdf,
                                                                const float *weight,
                                                                double min_weight,
                                                                uint8_t *cellf) {
  SurfNode p;
  if (!surf_node(G, &p)) return;
  int flag = 0;
  if (p.ix < G.nx - 1 && p.iy < G.ny - 1 && p.iz < G.nz - 1) {
    bool ok;
    const int neg = surf_cell_signs(G, p.t, tsdf, weight, min_weight, &ok);
    if (ok) {
      int n = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) n += c_tet_table[k][surf_tet_code(k, neg)][0];
      flag = 0x80 | n;
    }
  }
  cellf[p.t] = static_cast<uint8_t>(flag);
}

__global__ __launch_bounds__(kSurfThreads) void k_surface_nodes(SurfGrid G, const float *tsdf,
                                                                const uint8_t *cellf,
                                                                uint8_t *nmask) {
  SurfNode p;
  if (!surf_node(G, &p)) return;
  // bit s of cv: the cell at node - (sx, sy, sz), s = sx | sy << 1 | sz << 2, is valid
  int cv = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    // the load is unconditional, at the node itself where the cell would lie outside
    const bool in = p.ix >= (s & 1) && p.iy >= (s >> 1 & 1) && p.iz >= (s >> 2);
    const int flag = cellf[in ? p.t - surf_corner(G, s) : p.t];
    cv |= (in ? flag >> 7 : 0) << s;
  }
  int mask = 0;
  if (cv) {
    const bool neg = tsdf[p.t] < 0.0f;
    constexpr int kEdge[7] = {1, 2, 4, 3, 5, 6, 7};   // the edge types as corner codes
#pragma unroll
    for (int ty = 0; ty < 7; ++ty) {
      const int e = kEdge[ty];
      // the cells that contain the edge: node - s for every s that is 0 where e is 1
      int cells = 0;
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if ((s & e) == 0) cells |= 1 << s;
      const bool in = p.ix + (e & 1) < G.nx && p.iy + (e >> 1 & 1) < G.ny && p.iz + (e >> 2) < G.nz;
      const bool other = tsdf[in ? p.t + surf_corner(G, e) : p.t] < 0.0f;
      if (in && (cv & cells) && other != neg) mask |= 1 << ty;
    }
  }
  nmask[p.t] = static_cast<uint8_t>(mask);
}

// What a byte of the two count arrays stands for.
struct SurfVertexCount {
  __device__ static int of(uint8_t b) { return __popc(static_cast<unsigned>(b) & 0x7fu); }
};
struct SurfFaceCount {
  __device__ static int of(uint8_t b) { return b & 0x0f; }
};

// Exclusive scan of one chunk of int values held in registers (kSurfScanItems per thread, 0 past
// the end), started at `carry`; returns the chunk's sum.  All threads call it together.
__device__ __forceinline__ int surf_scan_chunk(const int (&x)[kSurfScanItems], int32_t *out,
                                               int64_t base, int64_t end, int carry, int *lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int sum = 0;
#pragma unroll
  for (int k = 0; k < kSurfScanItems; ++k) sum += x[k];
  int incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kSurfThreads / 64; ++w) {
    if (w < wave) before += lds[w];
    all += lds[w];
  }
  int run = carry + before + incl - sum;
  if (base + kSurfScanItems <= end) {   // a whole, 32-byte aligned group: two 16-byte stores
    int y[kSurfScanItems];
#pragma unroll
    for (int k = 0; k < kSurfScanItems; ++k) {
      y[k] = run;
      run += x[k];
    }
    int4 *o = reinterpret_cast<int4 *>(out + base);
    o[0] = make_int4(y[0], y[1], y[2], y[3]);
    o[1] = make_int4(y[4], y[5], y[6], y[7]);
  } else {
#pragma unroll
    for (int k = 0; k < kSurfScanItems; ++k) {
      if (base + k < end) out[base + k] = run;
      run += x[k];
    }
  }
  __syncthreads();
  return all;
}
static_assert(kSurfScanItems == 8, "the scans move a thread's 8 items as 8 and 2 x 16 bytes");

// First every workgroup scans the counts of its own chunk into out and leaves the chunk's sum ...
template <class Count>
__global__ __launch_bounds__(kSurfThreads) void k_surface_scan_chunks(const uint8_t *in,
                                                                      int64_t n, int32_t *out,
                                                                      int32_t *sums) {
  __shared__ int lds[kSurfThreads / 64];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSurfScanChunk +
                       static_cast<int64_t>(threadIdx.x) * kSurfScanItems;
  int x[kSurfScanItems];
  if (base + kSurfScanItems <= n) {   // the thread's 8 bytes in one aligned load
    const uint2 raw = *reinterpret_cast<const uint2 *>(in + base);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = Count::of(static_cast<uint8_t>(raw.x >> (8 * k)));
      x[k + 4] = Count::of(static_cast<uint8_t>(raw.y >> (8 * k)));
    }
  } else {
#pragma unroll
    for (int k = 0; k < kSurfScanItems; ++k) x[k] = base + k < n ? Count::of(in[base + k]) : 0;
  }
  const int total = surf_scan_chunk(x, out, base, n, 0, lds);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ... then one workgroup turns v[0 .. m), the chunk sums, into exclusive offsets in place with the
// total in v[m] ...
__global__ __launch_bounds__(kSurfThreads) void k_surface_scan_sums(int32_t *v, int64_t m) {
  __shared__ int lds[kSurfThreads / 64];
  int carry = 0;
  for (int64_t at = 0; at < m; at += kSurfScanChunk) {
    const int64_t base = at + static_cast<int64_t>(threadIdx.x) * kSurfScanItems;
    int x[kSurfScanItems];
#pragma unroll
    for (int k = 0; k < kSurfScanItems; ++k) x[k] = base + k < m ? v[base + k] : 0;
    carry += surf_scan_chunk(x, v, base, m, carry, lds);
  }
  if (threadIdx.x == 0) v[m] = carry;
}

// ... and every chunk adds its offset: out[0 .. n) are the exclusive offsets, out[n] the total.
__global__ __launch_bounds__(kSurfThreads) void k_surface_scan_add(int32_t *out, int64_t n,
                                                                   const int32_t *sums,
                                                                   int nchunks) {
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kSurfScanChunk +
                       static_cast<int64_t>(threadIdx.x) * kSurfScanItems;
  const int add = sums[blockIdx.x];
  if (base + kSurfScanItems <= n) {
    int4 *o = reinterpret_cast<int4 *>(out + base);
    int4 a = o[0], b = o[1];
    a.x += add; a.y += add; a.z += add; a.w += add;
    b.x += add; b.y += add; b.z += add; b.w += add;
    o[0] = a;
    o[1] = b;
  } else {
#pragma unroll
    for (int k = 0; k < kSurfScanItems; ++k)
      if (base + k < n) out[base + k] += add;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = sums[nchunks];
}

__global__ __launch_bounds__(kSurfThreads) void k_surface_vertices(SurfGrid G, const float *tsdf,
                                                                   const uint8_t *nmask,
                                                                   const int32_t *vbase,
                                                                   double *vertices) {
  // no product fused with a sum: the positions are the bits of the same expression in numpy
#pragma clang fp contract(off)
  SurfNode p;
  if (!surf_node(G, &p)) return;
  const int mask = nmask[p.t];
  if (!mask) return;
  const double fa = static_cast<double>(tsdf[p.t]);
  int64_t at = 3 * static_cast<int64_t>(vbase[p.t]);
  constexpr int kEdge[7] = {1, 2, 4, 3, 5, 6, 7};
#pragma unroll
  for (int ty = 0; ty < 7; ++ty) {
    if (!(mask >> ty & 1)) continue;
    const int e = kEdge[ty];
    const double fb = static_cast<double>(tsdf[p.t + surf_corner(G, e)]);
    const double t = fa / (fa - fb);
    vertices[at] = G.o[0] + G.voxel * (p.ix + t * (e & 1));
    vertices[at + 1] = G.o[1] + G.voxel * (p.iy + t * (e >> 1 & 1));
    vertices[at + 2] = G.o[2] + G.voxel * (p.iz + t * (e >> 2));
    at += 3;
  }
}

__global__ __launch_bounds__(kSurfThreads) void k_surface_faces(SurfGrid G, const float *tsdf,
                                                                const uint8_t *cellf,
                                                                const uint8_t *nmask,
                                                                const int32_t *vbase,
                                                                const int32_t *fbase,
                                                                int32_t *faces) {
  SurfNode p;
  if (!surf_node(G, &p)) return;
  if (!(cellf[p.t] & 0x0f)) return;   // no triangle; a cell with triangles is valid and inside
  const int neg = surf_cell_signs(G, p.t, tsdf, nullptr, 0.0, nullptr);
  int64_t at = 3 * static_cast<int64_t>(fbase[p.t]);
  for (int k = 0; k < 6; ++k) {
    const uint8_t *row = c_tet_table[k][surf_tet_code(k, neg)];
    const int nv = 3 * row[0];
    for (int j = 0; j < nv; ++j) {
      const int ec = row[1 + j];
      const int64_t owner = p.t + surf_corner(G, ec >> 3);
      faces[at++] = vbase[owner] + __popc(static_cast<unsigned>(nmask[owner]) & ((1u << (ec & 7)) - 1u));
    }
  }
}

}  // namespace rsd

namespace {

bool all_finite(const double *v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

int check_grid(const double *origin, double voxel, int64_t nz, int64_t ny, int64_t nx,
               rsd::SurfGrid *G) {
  if (nz < 1 || ny < 1 || nx < 1 || nz > RS_SURFACE_MAX_SIDE || ny > RS_SURFACE_MAX_SIDE ||
      nx > RS_SURFACE_MAX_SIDE)
    return fail(RS_EINVAL, "each side of the volume must be in 1..2048");
  if (nz * ny * nx > RS_SURFACE_MAX_NODES) return fail(RS_EINVAL, "a volume of more than 2^27 nodes");
  if (!all_finite(origin, 3) || !std::isfinite(voxel) || !(voxel > 0.0))
    return fail(RS_EINVAL, "origin must be finite, voxel finite and positive");
  for (int a = 0; a < 3; ++a) G->o[a] = origin[a];
  G->voxel = voxel;
  G->nx = static_cast<int>(nx);
  G->ny = static_cast<int>(ny);
  G->nz = static_cast<int>(nz);
  G->n = nz * ny * nx;
  return RS_OK;
}

}  // namespace

extern "C" int rs_surface_integrate(rs_ctx *c, const double *depth, const float *weights,
                                    int32_t V, int64_t h, int64_t w, const double *P,
                                    const double *origin, double voxel, int64_t nz, int64_t ny,
                                    int64_t nx, double trunc, int32_t has_prior, float *tsdf,
                                    float *weight) {
  if (!c || !depth || !P || !origin || !tsdf || !weight) return fail(RS_EINVAL, "null pointer");
  if (V < 1 || V > RS_DENSE_MAX_VIEWS) return fail(RS_EINVAL, "1 to 128 views");
  if (h < 1 || w < 1 || h > RS_DENSE_MAX_SIDE || w > RS_DENSE_MAX_SIDE)
    return fail(RS_EINVAL, "each image side must be in 1..16384");
  if (h * w > RS_DENSE_MAX_PIXELS || V * h * w > RS_DENSE_MAX_VOLUME)
    return fail(RS_EINVAL, "more than 2^26 pixels per view or 2^28 in all");
  rsd::SurfGrid G;
  int st = check_grid(origin, voxel, nz, ny, nx, &G);
  if (st) return st;
  if (!std::isfinite(trunc) || !(trunc > 0.0))
    return fail(RS_EINVAL, "trunc must be finite and positive");
  if (!all_finite(P, 12 * V)) return fail(RS_EINVAL, "the cameras must be finite");

  const size_t m = static_cast<size_t>(V * h * w), n = static_cast<size_t>(G.n);
  rs::Layout L;  // [depth | weights | P | tsdf | weight] go up, [tsdf | weight] come down
  const auto b_depth = L.add<double>(m);
  const auto b_wmap = L.add<float>(weights ? m : 0);
  const auto b_P = L.add<double>(12 * V);
  const auto b_tsdf = L.add<float>(n), b_weight = L.add<float>(n);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_depth.dev(), depth, b_depth.bytes, hipMemcpyHostToDevice, s));
  if (weights)
    HIP_TRY(hipMemcpyAsync(b_wmap.dev(), weights, b_wmap.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_P.dev(), P, b_P.bytes, hipMemcpyHostToDevice, s));
  if (has_prior) {
    HIP_TRY(hipMemcpyAsync(b_tsdf.dev(), tsdf, b_tsdf.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b_weight.dev(), weight, b_weight.bytes, hipMemcpyHostToDevice, s));
  }
  if ((st = c->surface.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_surface_integrate, dim3(rs::blocks(G.n, rsd::kSurfThreads)),
                     dim3(rsd::kSurfThreads), 0, s, b_depth.dev(),
                     weights ? b_wmap.dev() : nullptr, V, static_cast<int>(h),
                     static_cast<int>(w), b_P.dev(), G, trunc, has_prior ? 1 : 0, b_tsdf.dev(),
                     b_weight.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->surface.mark(1, s))) return st;
  HIP_TRY(hipMemcpyAsync(tsdf, b_tsdf.dev(), b_tsdf.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(weight, b_weight.dev(), b_weight.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return c->surface.read(0, 0, 1);
}

extern "C" int rs_surface_extract(rs_ctx *c, const float *tsdf, const float *weight, int64_t nz,
                                  int64_t ny, int64_t nx, const double *origin, double voxel,
                                  double min_weight, double *vertices, int64_t vcap,
                                  int32_t *faces, int64_t fcap, int64_t *nv, int64_t *nf) {
  if (nv) *nv = 0;
  if (nf) *nf = 0;
  if (!c || !tsdf || !weight || !origin || !nv || !nf) return fail(RS_EINVAL, "null pointer");
  if (vcap < 0 || fcap < 0 || (vcap > 0 && !vertices) || (fcap > 0 && !faces))
    return fail(RS_EINVAL, "a capacity is negative or its array is null");
  rsd::SurfGrid G;
  int st = check_grid(origin, voxel, nz, ny, nx, &G);
  if (st) return st;
  if (!std::isfinite(min_weight) || !(min_weight > 0.0))
    return fail(RS_EINVAL, "min_weight must be finite and positive");

  const size_t n = static_cast<size_t>(G.n);
  const int nchunks = static_cast<int>(rs::blocks(G.n, rsd::kSurfScanChunk));
  // no mesh of this volume is larger than 7 vertices a node and 12 triangles a cell
  const size_t vroom = static_cast<size_t>(vcap) < 7 * n ? static_cast<size_t>(vcap) : 7 * n;
  const size_t froom = static_cast<size_t>(fcap) < 12 * n ? static_cast<size_t>(fcap) : 12 * n;
  rs::Layout L;  // [tsdf | weight] go up, [totals] and, when it fits, [vertices | faces] come down
  const auto b_tsdf = L.add<float>(n), b_weight = L.add<float>(n);
  const auto b_cellf = L.add<uint8_t>(n), b_nmask = L.add<uint8_t>(n);
  const auto b_vbase = L.add<int32_t>(n + 1), b_fbase = L.add<int32_t>(n + 1);
  const auto b_vsums = L.add<int32_t>(nchunks + 1), b_fsums = L.add<int32_t>(nchunks + 1);
  const auto b_vert = L.add<double>(3 * vroom);
  const auto b_face = L.add<int32_t>(3 * froom);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_tsdf.dev(), tsdf, b_tsdf.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_weight.dev(), weight, b_weight.bytes, hipMemcpyHostToDevice, s));

  const dim3 grid(rs::blocks(G.n, rsd::kSurfThreads)), block(rsd::kSurfThreads);
  const dim3 sgrid(static_cast<unsigned>(nchunks));
  if ((st = c->surface.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_surface_cells, grid, block, 0, s, G, b_tsdf.dev(), b_weight.dev(),
                     min_weight, b_cellf.dev());
  hipLaunchKernelGGL(rsd::k_surface_nodes, grid, block, 0, s, G, b_tsdf.dev(), b_cellf.dev(),
                     b_nmask.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->surface.mark(1, s))) return st;
  hipLaunchKernelGGL(rsd::k_surface_scan_chunks<rsd::SurfVertexCount>, sgrid, block, 0, s,
                     b_nmask.dev(), G.n, b_vbase.dev(), b_vsums.dev());
  hipLaunchKernelGGL(rsd::k_surface_scan_chunks<rsd::SurfFaceCount>, sgrid, block, 0, s,
                     b_cellf.dev(), G.n, b_fbase.dev(), b_fsums.dev());
  hipLaunchKernelGGL(rsd::k_surface_scan_sums, dim3(1), block, 0, s, b_vsums.dev(),
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_surface_scan_sums, dim3(1), block, 0, s, b_fsums.dev(),
                     static_cast<int64_t>(nchunks));
  hipLaunchKernelGGL(rsd::k_surface_scan_add, sgrid, block, 0, s, b_vbase.dev(), G.n,
                     b_vsums.dev(), nchunks);
  hipLaunchKernelGGL(rsd::k_surface_scan_add, sgrid, block, 0, s, b_fbase.dev(), G.n,
                     b_fsums.dev(), nchunks);
  HIP_TRY(hipGetLastError());
  if ((st = c->surface.mark(2, s))) return st;
  int32_t totals[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&totals[0], b_vbase.dev() + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&totals[1], b_fbase.dev() + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->surface.read(1, 0, 1))) return st;
  if ((st = c->surface.read(2, 1, 2))) return st;
  *nv = totals[0];
  *nf = totals[1];
  if (3 * *nf > INT32_MAX) return fail(RS_EINVAL, "the mesh has more than 2^31 - 1 face indices");
  if (*nv > vcap || *nf > fcap)
    return fail(RS_EINVAL, "the mesh does not fit the capacities (nv and nf state its size)");
  if (*nv == 0 && *nf == 0) return RS_OK;

  if ((st = c->surface.mark(3, s))) return st;
  hipLaunchKernelGGL(rsd::k_surface_vertices, grid, block, 0, s, G, b_tsdf.dev(), b_nmask.dev(),
                     b_vbase.dev(), b_vert.dev());
  hipLaunchKernelGGL(rsd::k_surface_faces, grid, block, 0, s, G, b_tsdf.dev(), b_cellf.dev(),
                     b_nmask.dev(), b_vbase.dev(), b_fbase.dev(), b_face.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->surface.mark(4, s))) return st;
  if (*nv)
    HIP_TRY(hipMemcpyAsync(vertices, b_vert.dev(), sizeof(double) * 3 * *nv, hipMemcpyDeviceToHost, s));
  if (*nf)
    HIP_TRY(hipMemcpyAsync(faces, b_face.dev(), sizeof(int32_t) * 3 * *nf, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return c->surface.read(3, 3, 4);
}

extern "C" int rs_surface_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->surface.enable(enable != 0);
  if (st) return st;
  c->surface.copy_out(ms);
  return RS_OK;
}
