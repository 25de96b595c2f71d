// Colour for the mesh of the surface stage: the mesh itself rendered into one z-buffer per view
// (rs_surface_render_depth) and a colour per vertex gathered from the views that see it
// (rs_surface_colorize).  The definitions stand in include/rsamd.h; tests/texture_ref.py restates
// them in numpy.  The host hands the kernels s_v P_v, s_v = sign det P_v[:, :3], so that "in front
// of the camera" is a positive third coordinate.
//
//   k_texture_fill          every z-buffer pixel to +inf, the list's counter to 0
//   k_texture_raster_small  one lane per face, a loop over the views (P read at a wave-uniform
//                           index): project, and walk the clipped bounding box if it holds at most
//                           RS_SURFACE_RASTER_SMALL pixels; a larger box is appended to a list as
//                           (face, view) with one atomic add on a counter
//   k_texture_raster_large  one wave per list entry, the 64 lanes across the box
//   k_texture_finish        +inf to NaN
//   k_texture_gather        one lane per vertex, a loop over the views, all fp64: project, test
//                           the depth against the four z-buffer pixels of the bilinear footprint,
//                           sample, accumulate
// A pixel's depth is folded with atomicMin on the bits of the positive float32, whose order is
// the floats' own; nothing reads the value back.  A minimum commutes, so the z-buffer depends on
// neither the launch shape, nor the order of the faces, nor which of the two kernels drew a face
// -- both call the same tex_project and tex_pixel, compiled without FMA contraction.  The order of
// the list therefore cannot matter either.  The list holds min(nf V, kTexListCap) entries; a large
// face that finds it full is walked by its own lane: slower, the same bits.
// Every global index is bounded: a vertex is read at a face index the host has checked against nv
// before any launch; a z-buffer pixel is written only inside the box that tex_project has clipped
// to [0, w-1] x [0, h-1]; the list is written below its capacity and read below
// min(counter, capacity); the gather indexes the z-buffer and the images only after its bounds
// test has placed (u, v) in the image.
#include <hip/hip_runtime.h>

#include <cmath>

#include "host.h"

namespace rsd {

constexpr int kTexThreads = 256;
constexpr int kTexListCap = 1 << 20;   // entries of 8 bytes
static_assert(RS_SURFACE_TEXTURE_LIST_CAP == kTexListCap, "the header states the list's capacity");
constexpr uint32_t kTexInf = 0x7f800000u, kTexNaN = 0x7fc00000u;

struct TexTri {
  double X[3][3];
};

// A face in one view, ready to be drawn: the projections, the depths, the doubled signed area and
// the clipped bounding box.
struct TexFace {
  double x[3], y[3], z[3], A;
  int px, py, bw, bh;
};

__device__ __forceinline__ void tex_load(const double *vertices, const int32_t *faces, int64_t f,
                                         TexTri *T) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int64_t at = 3 * static_cast<int64_t>(faces[3 * f + i]);
#pragma unroll
    for (int k = 0; k < 3; ++k) T->X[i][k] = vertices[at + k];
  }
}

// false: the face is not drawn in this view (a vertex not in front or not finite, no area, or a
// box that misses the image)
__device__ __forceinline__ bool tex_project(const TexTri &T, const double *Pv, int h, int w,
                                            TexFace *t) {
#pragma clang fp contract(off)
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double *X = T.X[i];
    const double q0 = Pv[0] * X[0] + Pv[1] * X[1] + Pv[2] * X[2] + Pv[3];
    const double q1 = Pv[4] * X[0] + Pv[5] * X[1] + Pv[6] * X[2] + Pv[7];
    const double q2 = Pv[8] * X[0] + Pv[9] * X[1] + Pv[10] * X[2] + Pv[11];
    ok = ok && isfinite(q0) && isfinite(q1) && isfinite(q2) && q2 > 0.0;
    t->x[i] = q0 / q2;
    t->y[i] = q1 / q2;
    t->z[i] = q2;
  }
  if (!ok) return false;
  t->A = (t->x[1] - t->x[0]) * (t->y[2] - t->y[0]) - (t->x[2] - t->x[0]) * (t->y[1] - t->y[0]);
  if (!isfinite(t->A) || t->A == 0.0) return false;
  // clipped while still fp64: a finite A does not bound the coordinates by what an int holds
  const double lox = fmax(ceil(fmin(t->x[0], fmin(t->x[1], t->x[2]))), 0.0);
  const double hix = fmin(floor(fmax(t->x[0], fmax(t->x[1], t->x[2]))), static_cast<double>(w - 1));
  const double loy = fmax(ceil(fmin(t->y[0], fmin(t->y[1], t->y[2]))), 0.0);
  const double hiy = fmin(floor(fmax(t->y[0], fmax(t->y[1], t->y[2]))), static_cast<double>(h - 1));
  if (!(lox <= hix && loy <= hiy)) return false;
  t->px = static_cast<int>(lox);
  t->py = static_cast<int>(loy);
  t->bw = static_cast<int>(hix) - t->px + 1;
  t->bh = static_cast<int>(hiy) - t->py + 1;   // bw bh <= h w <= 2^26
  return true;
}

// (px, py) lies in the clipped box, so inside the image; zview is the view's z-buffer
__device__ __forceinline__ void tex_pixel(const TexFace &t, int px, int py, int w,
                                          uint32_t *zview) {
#pragma clang fp contract(off)
  const double X = static_cast<double>(px), Y = static_cast<double>(py);
  const double b0 = ((t.x[2] - t.x[1]) * (Y - t.y[1]) - (t.y[2] - t.y[1]) * (X - t.x[1])) / t.A;
  const double b1 = ((t.x[0] - t.x[2]) * (Y - t.y[2]) - (t.y[0] - t.y[2]) * (X - t.x[2])) / t.A;
  const double b2 = ((t.x[1] - t.x[0]) * (Y - t.y[0]) - (t.y[1] - t.y[0]) * (X - t.x[0])) / t.A;
  if (b0 >= 0.0 && b1 >= 0.0 && b2 >= 0.0) {
    const float zeta = static_cast<float>(1.0 / (b0 / t.z[0] + b1 / t.z[1] + b2 / t.z[2]));
    // zeta >= 0; a NaN's bits lie above +inf's and would never win, it is not sent at all
    if (zeta == zeta) atomicMin(zview + static_cast<int64_t>(py) * w + px, __float_as_uint(zeta));
  }
}

// 4 words a thread where all 4 lie below n (z is 256-byte aligned)
__global__ __launch_bounds__(kTexThreads) void k_texture_fill(uint32_t *z, int64_t n,
                                                              unsigned long long *count) {
  const int64_t base = 4 * (static_cast<int64_t>(blockIdx.x) * kTexThreads + threadIdx.x);
  if (base == 0) *count = 0ull;
  if (base + 4 <= n) {
    *reinterpret_cast<uint4 *>(z + base) = make_uint4(kTexInf, kTexInf, kTexInf, kTexInf);
  } else {
    for (int64_t k = base; k < n; ++k) z[k] = kTexInf;
  }
}

__global__ __launch_bounds__(kTexThreads) void k_texture_finish(uint32_t *z, int64_t n) {
  const int64_t base = 4 * (static_cast<int64_t>(blockIdx.x) * kTexThreads + threadIdx.x);
  if (base + 4 <= n) {
    uint4 a = *reinterpret_cast<uint4 *>(z + base);
    a.x = a.x == kTexInf ? kTexNaN : a.x;
    a.y = a.y == kTexInf ? kTexNaN : a.y;
    a.z = a.z == kTexInf ? kTexNaN : a.z;
    a.w = a.w == kTexInf ? kTexNaN : a.w;
    *reinterpret_cast<uint4 *>(z + base) = a;
  } else {
    for (int64_t k = base; k < n; ++k)
      if (z[k] == kTexInf) z[k] = kTexNaN;
  }
}

__global__ __launch_bounds__(kTexThreads) void k_texture_raster_small(
    const double *vertices, const int32_t *faces, int64_t nf, int V, int h, int w, const double *P,
    uint32_t *zbuf, int2 *list, int cap, unsigned long long *count) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kTexThreads + threadIdx.x;
  if (f >= nf) return;
  TexTri T;
  tex_load(vertices, faces, f, &T);
  const int64_t hw = static_cast<int64_t>(h) * w;
  for (int v = 0; v < V; ++v) {
    TexFace t;
    if (!tex_project(T, P + 12 * v, h, w, &t)) continue;
    if (t.bw * t.bh > RS_SURFACE_RASTER_SMALL) {
      const unsigned long long at = atomicAdd(count, 1ull);
      if (at < static_cast<unsigned long long>(cap)) {
        list[at] = make_int2(static_cast<int>(f), v);
        continue;
      }
    }
    uint32_t *zview = zbuf + v * hw;
    for (int r = 0; r < t.bh; ++r)
      for (int c = 0; c < t.bw; ++c) tex_pixel(t, t.px + c, t.py + r, w, zview);
  }
}

__global__ __launch_bounds__(kTexThreads) void k_texture_raster_large(
    const double *vertices, const int32_t *faces, int h, int w, const double *P, uint32_t *zbuf,
    const int2 *list, int cap, const unsigned long long *count) {
  const unsigned long long total = *count;
  const int n = total < static_cast<unsigned long long>(cap) ? static_cast<int>(total) : cap;
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * (kTexThreads / 64);
  const int64_t hw = static_cast<int64_t>(h) * w;
  for (int e = blockIdx.x * (kTexThreads / 64) + (threadIdx.x >> 6); e < n; e += nwaves) {
    const int2 fv = list[e];
    // the entry is the wave's own: its face and view in scalar registers
    const int f = __builtin_amdgcn_readfirstlane(fv.x), v = __builtin_amdgcn_readfirstlane(fv.y);
    TexTri T;
    tex_load(vertices, faces, f, &T);
    TexFace t;
    if (!tex_project(T, P + 12 * v, h, w, &t)) continue;   // it was drawable when it was listed
    uint32_t *zview = zbuf + v * hw;
    const int npix = t.bw * t.bh;
    for (int k = lane; k < npix; k += 64) {
      const int r = k / t.bw;
      tex_pixel(t, t.px + (k - r * t.bw), t.py + r, w, zview);
    }
  }
}

template <int CH>
__global__ __launch_bounds__(kTexThreads) void k_texture_gather(
    const double *vertices, const double *normals, int64_t nv, const uint8_t *images, int V, int h,
    int w, const double *P, const double *centres, const float *zbuf, double rel_tol,
    double min_cos, double *colors, int32_t *count) {
#pragma clang fp contract(off)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kTexThreads + threadIdx.x;
  if (i >= nv) return;
  const double X0 = vertices[3 * i], X1 = vertices[3 * i + 1], X2 = vertices[3 * i + 2];
  double n0 = 0.0, n1 = 0.0, n2 = 0.0;
  if (normals) {
    n0 = normals[3 * i];
    n1 = normals[3 * i + 1];
    n2 = normals[3 * i + 2];
  }
  const double wm1 = static_cast<double>(w - 1), hm1 = static_cast<double>(h - 1);
  const int64_t hw = static_cast<int64_t>(h) * w;
  double acc[CH] = {}, wsum = 0.0;
  int seen = 0;
  for (int v = 0; v < V; ++v) {
    const double *Pv = P + 12 * v;
    const double q0 = Pv[0] * X0 + Pv[1] * X1 + Pv[2] * X2 + Pv[3];
    const double q1 = Pv[4] * X0 + Pv[5] * X1 + Pv[6] * X2 + Pv[7];
    const double z = Pv[8] * X0 + Pv[9] * X1 + Pv[10] * X2 + Pv[11];
    if (!(z > 0.0 && isfinite(z) && isfinite(q0) && isfinite(q1))) continue;
    const double u = q0 / z, r = q1 / z;
    if (!(u >= 0.0 && u <= wm1 && r >= 0.0 && r <= hm1)) continue;
    const double fu = floor(u), fr = floor(r);
    const int x0 = static_cast<int>(fu), y0 = static_cast<int>(fr);
    const int x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const int64_t a00 = v * hw + static_cast<int64_t>(y0) * w + x0;
    const int64_t a01 = v * hw + static_cast<int64_t>(y0) * w + x1;
    const int64_t a10 = v * hw + static_cast<int64_t>(y1) * w + x0;
    const int64_t a11 = v * hw + static_cast<int64_t>(y1) * w + x1;
    const float d00 = zbuf[a00], d01 = zbuf[a01], d10 = zbuf[a10], d11 = zbuf[a11];
    float far = -1.0f;   // the depths are >= 0
    if (isfinite(d00)) far = fmaxf(far, d00);
    if (isfinite(d01)) far = fmaxf(far, d01);
    if (isfinite(d10)) far = fmaxf(far, d10);
    if (isfinite(d11)) far = fmaxf(far, d11);
    if (far < 0.0f) continue;
    if (!(z <= static_cast<double>(far) * (1.0 + rel_tol))) continue;
    double g = 1.0;
    if (normals) {
      const double *cv = centres + 3 * v;
      const double d0 = cv[0] - X0, d1 = cv[1] - X1, d2 = cv[2] - X2;
      g = (n0 * d0 + n1 * d1 + n2 * d2) / sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      if (!(g > min_cos)) continue;   // false for a NaN
    }
    const double fx = u - fu, fy = r - fr;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const double i00 = images[a00 * CH + c], i01 = images[a01 * CH + c];
      const double i10 = images[a10 * CH + c], i11 = images[a11 * CH + c];
      const double top = i00 + fx * (i01 - i00), bot = i10 + fx * (i11 - i10);
      acc[c] += g * (top + fy * (bot - top));
    }
    wsum += g;
    ++seen;
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) colors[i * CH + c] = seen ? acc[c] / (255.0 * wsum) : 0.0;
  count[i] = seen;
}

}  // namespace rsd

namespace {

using rs::Layout;

// The buffers of the rasteriser inside a call's layout, and its launches.
struct TexRaster {
  Layout::Buf<double> vert, P;
  Layout::Buf<int32_t> face;
  Layout::Buf<uint32_t> z;
  Layout::Buf<int2> list;
  Layout::Buf<unsigned long long> count;
  int64_t nv, nf, hw;
  int V, h, w, cap;
  double Ps[12 * RS_DENSE_MAX_VIEWS];   // s_v P_v

  // RS_EINVAL for everything rs_surface_render_depth lists; fills Ps
  int check(const double *vertices, int64_t nv_, const int32_t *faces, int64_t nf_,
            const double *Pin, int32_t V_, int64_t h_, int64_t w_) {
    if (V_ < 1 || V_ > RS_DENSE_MAX_VIEWS) return fail(RS_EINVAL, "1 to 128 views");
    if (h_ < 1 || w_ < 1 || h_ > RS_DENSE_MAX_SIDE || w_ > RS_DENSE_MAX_SIDE)
      return fail(RS_EINVAL, "each image side must be in 1..16384");
    if (h_ * w_ > RS_DENSE_MAX_PIXELS || V_ * h_ * w_ > RS_DENSE_MAX_VOLUME)
      return fail(RS_EINVAL, "more than 2^26 pixels per view or 2^28 in all");
    if (nv_ < 0 || nf_ < 0 || nv_ > INT32_MAX || 3 * nf_ > INT32_MAX)
      return fail(RS_EINVAL, "nv and 3 nf must be in 0..2^31 - 1");
    if ((nv_ > 0 && !vertices) || (nf_ > 0 && !faces)) return fail(RS_EINVAL, "null pointer");
    for (int64_t k = 0; k < 3 * nf_; ++k)
      if (faces[k] < 0 || faces[k] >= nv_) return fail(RS_EINVAL, "a face index is out of range");
    for (int v = 0; v < V_; ++v) {
      const double *p = Pin + 12 * v;
      const double det = p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8]) +
                         p[2] * (p[4] * p[9] - p[5] * p[8]);
      bool finite = std::isfinite(det);
      for (int k = 0; k < 12; ++k) finite = finite && std::isfinite(p[k]);
      if (!finite || det == 0.0)
        return fail(RS_EINVAL, "a camera is not finite or det P[:, :3] is zero or not finite");
      for (int k = 0; k < 12; ++k) Ps[12 * v + k] = det < 0.0 ? -p[k] : p[k];
    }
    nv = nv_, nf = nf_, V = V_, h = static_cast<int>(h_), w = static_cast<int>(w_), hw = h_ * w_;
    const int64_t pairs = nf * V;
    cap = static_cast<int>(pairs < rsd::kTexListCap ? pairs : rsd::kTexListCap);
    return RS_OK;
  }

  void add(Layout &L) {
    vert = L.add<double>(3 * static_cast<size_t>(nv));
    face = L.add<int32_t>(3 * static_cast<size_t>(nf));
    P = L.add<double>(12 * static_cast<size_t>(V));
    z = L.add<uint32_t>(static_cast<size_t>(V * hw));
    list = L.add<int2>(static_cast<size_t>(cap));
    count = L.add<unsigned long long>(1);
  }

  // upload, then events 0 | fill, small | 1 | large, finish | 2 of the context's texture timer
  int run(rs_ctx *c, const double *vertices, const int32_t *faces) {
    hipStream_t s = c->stream;
    int st;
    if (nv) HIP_TRY(hipMemcpyAsync(vert.dev(), vertices, vert.bytes, hipMemcpyHostToDevice, s));
    if (nf) HIP_TRY(hipMemcpyAsync(face.dev(), faces, face.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(P.dev(), Ps, P.bytes, hipMemcpyHostToDevice, s));
    const int64_t n = V * hw;
    const dim3 block(rsd::kTexThreads), zgrid(rs::blocks(n, 4 * rsd::kTexThreads));
    if ((st = c->texture.mark(0, s))) return st;
    hipLaunchKernelGGL(rsd::k_texture_fill, zgrid, block, 0, s, z.dev(), n, count.dev());
    if (nf)
      hipLaunchKernelGGL(rsd::k_texture_raster_small, dim3(rs::blocks(nf, rsd::kTexThreads)),
                         block, 0, s, vert.dev(), face.dev(), nf, V, h, w, P.dev(), z.dev(),
                         list.dev(), cap, count.dev());
    HIP_TRY(hipGetLastError());
    if ((st = c->texture.mark(1, s))) return st;
    if (nf) {
      // one wave per entry; a grid of at most 2048 workgroups strides over longer lists
      const unsigned need = rs::blocks(cap, rsd::kTexThreads / 64);
      hipLaunchKernelGGL(rsd::k_texture_raster_large, dim3(need < 2048u ? need : 2048u), block, 0,
                         s, vert.dev(), face.dev(), h, w, P.dev(), z.dev(), list.dev(), cap,
                         count.dev());
    }
    hipLaunchKernelGGL(rsd::k_texture_finish, zgrid, block, 0, s, z.dev(), n);
    HIP_TRY(hipGetLastError());
    return c->texture.mark(2, s);
  }

  int read_times(rs_ctx *c) {
    const int st = c->texture.read(0, 0, 1);
    return st ? st : c->texture.read(1, 1, 2);
  }
};

}  // namespace

extern "C" int rs_surface_render_depth(rs_ctx *c, const double *vertices, int64_t nv,
                                       const int32_t *faces, int64_t nf, const double *P,
                                       int32_t V, int64_t h, int64_t w, float *depth) {
  if (!c || !P || !depth) return fail(RS_EINVAL, "null pointer");
  TexRaster R;
  int st = R.check(vertices, nv, faces, nf, P, V, h, w);
  if (st) return st;
  Layout L;   // [vertices | faces | P] go up, [z] comes down
  R.add(L);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  if ((st = R.run(c, vertices, faces))) return st;
  HIP_TRY(hipMemcpyAsync(depth, R.z.dev(), R.z.bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return R.read_times(c);
}

extern "C" int rs_surface_colorize(rs_ctx *c, const double *vertices, int64_t nv,
                                   const int32_t *faces, int64_t nf, const uint8_t *images,
                                   int32_t channels, const double *P, int32_t V, int64_t h,
                                   int64_t w, const double *normals, double rel_tol,
                                   double min_cos, double *colors, int32_t *count, float *depth) {
  if (!c || !P || !images) return fail(RS_EINVAL, "null pointer");
  if (channels != 1 && channels != 3) return fail(RS_EINVAL, "images of 1 or 3 channels");
  if (!std::isfinite(rel_tol) || rel_tol < 0.0 || !std::isfinite(min_cos))
    return fail(RS_EINVAL, "rel_tol must be finite and not negative, min_cos finite");
  TexRaster R;
  int st = R.check(vertices, nv, faces, nf, P, V, h, w);
  if (st) return st;
  if (nv > 0 && (!colors || !count)) return fail(RS_EINVAL, "null pointer");
  // the camera centres c_v = -M^-1 p of s_v P_v, by the adjugate
  double centres[3 * RS_DENSE_MAX_VIEWS];
  for (int v = 0; v < V; ++v) {
    const double *p = R.Ps + 12 * v;
    const double a = p[0], b = p[1], cc = p[2], d = p[4], e = p[5], f = p[6], g = p[8], hh = p[9],
                 k = p[10];
    const double adj[9] = {e * k - f * hh, cc * hh - b * k, b * f - cc * e,
                           f * g - d * k,  a * k - cc * g,  cc * d - a * f,
                           d * hh - e * g, b * g - a * hh,  a * e - b * d};
    const double det = a * adj[0] + b * adj[3] + cc * adj[6];
    for (int r = 0; r < 3; ++r)
      centres[3 * v + r] = -(adj[3 * r] * p[3] + adj[3 * r + 1] * p[7] + adj[3 * r + 2] * p[11]) / det;
  }

  const size_t m = static_cast<size_t>(V * h * w), n = static_cast<size_t>(nv);
  Layout L;   // the rasteriser's, [images | normals | centres] go up, [colors | count] come down
  R.add(L);
  const auto b_img = L.add<uint8_t>(m * channels);
  const auto b_nrm = L.add<double>(normals ? 3 * n : 0);
  const auto b_ctr = L.add<double>(3 * static_cast<size_t>(V));
  const auto b_col = L.add<double>(n * channels);
  const auto b_cnt = L.add<int32_t>(n);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_img.dev(), images, b_img.bytes, hipMemcpyHostToDevice, s));
  if (normals && nv)
    HIP_TRY(hipMemcpyAsync(b_nrm.dev(), normals, b_nrm.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_ctr.dev(), centres, b_ctr.bytes, hipMemcpyHostToDevice, s));
  if ((st = R.run(c, vertices, faces))) return st;
  if (nv) {
    const dim3 grid(rs::blocks(nv, rsd::kTexThreads)), block(rsd::kTexThreads);
    const float *zf = reinterpret_cast<const float *>(R.z.dev());
    const double *nrm = normals ? b_nrm.dev() : nullptr;
    if (channels == 1)
      hipLaunchKernelGGL(rsd::k_texture_gather<1>, grid, block, 0, s, R.vert.dev(), nrm, nv,
                         b_img.dev(), V, R.h, R.w, R.P.dev(), b_ctr.dev(), zf, rel_tol, min_cos,
                         b_col.dev(), b_cnt.dev());
    else
      hipLaunchKernelGGL(rsd::k_texture_gather<3>, grid, block, 0, s, R.vert.dev(), nrm, nv,
                         b_img.dev(), V, R.h, R.w, R.P.dev(), b_ctr.dev(), zf, rel_tol, min_cos,
                         b_col.dev(), b_cnt.dev());
    HIP_TRY(hipGetLastError());
  }
  if ((st = c->texture.mark(3, s))) return st;
  if (nv) {
    HIP_TRY(hipMemcpyAsync(colors, b_col.dev(), b_col.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(count, b_cnt.dev(), b_cnt.bytes, hipMemcpyDeviceToHost, s));
  }
  if (depth) HIP_TRY(hipMemcpyAsync(depth, R.z.dev(), R.z.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = R.read_times(c))) return st;
  return c->texture.read(2, 2, 3);
}

extern "C" int rs_surface_texture_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->texture.enable(enable != 0);
  if (st) return st;
  c->texture.copy_out(ms);
  return RS_OK;
}
