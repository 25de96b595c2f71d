// The image front end on the GPU: the chain of fun.py:130-151 that turns two images into putative
// correspondences -- lab3.harris (lab3.py:131-157), lab3.non_max_suppression (lab3.py:160-185),
// the 0.001 * max threshold (fun.py:135-138), lab3.cut_out_rois (lab3.py:565-602) fused into
// fun.matchingMatrix (fun.py:113-120), and the argmins lab3.joint_min (lab3.py:529-563) needs.
// Plain HIP, no floating-point atomics: the same inputs give bitwise the same outputs.
//
// k_harris       one workgroup per 32 x 16 output tile.  The image tile with a halo of
//                max(1, kernel_size / 2) + block_size goes to LDS as bytes; Ix and Iy of the
//                (32 + block_size - 1) x (16 + block_size - 1) derivative tile go to LDS as
//                int32; every thread then box-sums Ix^2, IxIy, Iy^2 of two outputs in int64
//                (exact) and evaluates the response once in fp64.  Both reflections of the
//                definition (the image under the Sobel taps, the derivative image under the box)
//                are applied to coordinates, so a tile computes exactly what the whole image would.
// k_nms          one thread per pixel over its window; the borders are zero.
// k_corner_max / k_corner_count / k_corner_scan / k_corner_write
//                max(H) as per-block maxima re-reduced by every block (no atomics), hits per
//                2048-pixel chunk, one-block exclusive scan of the chunk counts, then every chunk
//                writes its hits at offset + rank: the list is in row-major scan order.
// k_match<T>     one workgroup per 64 x 64 tile of the (n1, n2) pair grid.  The patches of the
//                tile's 64 + 64 centres are gathered from the images into LDS element-major
//                ([element][patch], so that the four patches of a thread are one LDS word for
//                bytes); a thread accumulates a 4 x 4 register block of pairs over the elements in
//                raster order (uint32 for bytes: exact; fp64 for doubles, in chunks of 32 elements
//                so that the tile fits LDS), writes M = sqrt(d2) if asked, and the workgroup
//                reduces its tile to one (value, index) per row and per column, first index on ties.
// k_match_argmin one thread per row / column scans the tiles' partial minima in ascending tile
//                order with a strict "<": np.argmin's smallest index, whatever the block schedule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "host.h"

namespace rsd {

// ------------------------------------------------------------------------------------------
// Harris
// ------------------------------------------------------------------------------------------
constexpr int kHarrisTW = 32, kHarrisTH = 16, kHarrisThreads = 256;

// The Sobel pair of aperture ks (1, 3, 5, 7): smoothing taps and derivative taps, both of
// 2 r + 1 entries with r = max(1, ks / 2) (aperture 1 smooths with [0 1 0]).
__constant__ int c_sobel_smooth[4][7] = {{0, 1, 0, 0, 0, 0, 0},
                                         {1, 2, 1, 0, 0, 0, 0},
                                         {1, 4, 6, 4, 1, 0, 0},
                                         {1, 6, 15, 20, 15, 6, 1}};
__constant__ int c_sobel_deriv[4][7] = {{-1, 0, 1, 0, 0, 0, 0},
                                        {-1, 0, 1, 0, 0, 0, 0},
                                        {-1, -2, 0, 2, 1, 0, 0},
                                        {-1, -4, -5, 0, 5, 4, 1}};

// Reflect-101 (gfedcb|abcdefgh|gfedcba) for -n < p < 2n - 1; the entry point guarantees n is
// larger than every overhang, the clamp only keeps the discarded outputs of a partial tile legal.
__device__ __forceinline__ int reflect101(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * (n - 1) - p;
  return min(max(p, 0), n - 1);
}

struct HarrisArgs {
  const uint8_t *img;
  float *out;
  int h, w;
  int bs, ks;     // block_size, kernel_size
  int r, R;       // Sobel radius, halo r + bs
  double k, s2;   // Harris parameter, scale^2
  int raw;
};

__global__ __launch_bounds__(kHarrisThreads) void k_harris(HarrisArgs A) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int r = A.r, R = A.R, bs = A.bs, anchor = A.bs / 2;
  const int IW = kHarrisTW + 2 * R, IH = kHarrisTH + 2 * R;            // image tile
  const int DW = kHarrisTW + bs - 1, DH = kHarrisTH + bs - 1;          // derivative tile
  int32_t *dx = reinterpret_cast<int32_t *>(lds_raw);
  int32_t *dy = dx + DW * DH;
  uint8_t *tile = reinterpret_cast<uint8_t *>(dy + DW * DH);
  const int tx0 = blockIdx.x * kHarrisTW, ty0 = blockIdx.y * kHarrisTH;
  const int tid = threadIdx.x;

  // image tile: tile[i][j] = img[reflect(ty0 - R + i)][reflect(tx0 - R + j)]
  for (int idx = tid; idx < IW * IH; idx += kHarrisThreads) {
    const int i = idx / IW, j = idx - i * IW;
    tile[idx] = A.img[static_cast<size_t>(reflect101(ty0 - R + i, A.h)) * A.w +
                      reflect101(tx0 - R + j, A.w)];
  }
  __syncthreads();

  // derivative tile: position (ty0 - anchor + i, tx0 - anchor + j) of the derivative image,
  // which outside the image is the derivative AT the reflected pixel (second reflection); the
  // taps of that pixel reflect on the image again (first reflection).  Every coordinate the
  // valid outputs reach lies inside the image tile (|overhang| <= R); the clamp covers the rest.
  const int kk = A.ks == 1 ? 0 : A.ks / 2;   // row of the tap tables
  for (int idx = tid; idx < DW * DH; idx += kHarrisThreads) {
    const int i = idx / DW, j = idx - i * DW;
    const int qy = reflect101(ty0 - anchor + i, A.h), qx = reflect101(tx0 - anchor + j, A.w);
    int gx = 0, gy = 0;
    for (int a = -r; a <= r; ++a) {
      const int iy = min(max(reflect101(qy + a, A.h) - (ty0 - R), 0), IH - 1);
      const int sy = c_sobel_smooth[kk][a + r], dyw = c_sobel_deriv[kk][a + r];
      for (int b = -r; b <= r; ++b) {
        const int ix = min(max(reflect101(qx + b, A.w) - (tx0 - R), 0), IW - 1);
        const int v = tile[iy * IW + ix];
        gx += sy * c_sobel_deriv[kk][b + r] * v;
        gy += dyw * c_sobel_smooth[kk][b + r] * v;
      }
    }
    dx[idx] = gx;
    dy[idx] = gy;
  }
  __syncthreads();

  // two outputs per thread, rows ly and ly + 8
  const int lx = tid & (kHarrisTW - 1), ly = tid / kHarrisTW;
  for (int half = 0; half < 2; ++half) {
    const int oy = ly + half * (kHarrisTH / 2);
    const int x = tx0 + lx, y = ty0 + oy;
    if (x >= A.w || y >= A.h) continue;
    long long sxx = 0, sxy = 0, syy = 0;
    for (int i = 0; i < bs; ++i) {
      const int32_t *px = dx + (oy + i) * DW + lx, *py = dy + (oy + i) * DW + lx;
      for (int j = 0; j < bs; ++j) {
        const long long gx = px[j], gy = py[j];
        sxx += gx * gx;
        sxy += gx * gy;
        syy += gy * gy;
      }
    }
    // |sums| < 31^2 * (255 * 640)^2 < 2^45: exact in fp64.  The response is evaluated once.
    const double a = static_cast<double>(sxx) * A.s2, b = static_cast<double>(sxy) * A.s2,
                 c = static_cast<double>(syy) * A.s2;
    const double resp = a * c - b * b - A.k * (a + c) * (a + c);
    float f = static_cast<float>(resp);
    if (!A.raw && f < 0.0f) f = 0.0f;
    A.out[static_cast<size_t>(y) * A.w + x] = f;
  }
}

// ------------------------------------------------------------------------------------------
// Non-maximum suppression
// ------------------------------------------------------------------------------------------
// lab3.py:179-185: kept pixels are True * v = v, the others False * v = 0 * v (a signed zero).
__global__ __launch_bounds__(256) void k_nms(const float *img, float *out, int h, int w, int m) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= w || y >= h) return;
  const float v = img[static_cast<size_t>(y) * w + x];
  bool keep = x >= m && y >= m && x < w - m && y < h - m;
  if (keep) {
    for (int i = -m; i <= m && keep; ++i) {
      const float *row = img + static_cast<size_t>(y + i) * w + x;
      for (int j = -m; j <= m; ++j) keep = keep && !(row[j] > v);
    }
  }
  out[static_cast<size_t>(y) * w + x] = keep ? v : 0.0f * v;
}

// ------------------------------------------------------------------------------------------
// Corner list
// ------------------------------------------------------------------------------------------
constexpr int kCornerThreads = 256, kCornerItems = 8;
constexpr int kCornerChunk = kCornerThreads * kCornerItems;   // pixels per workgroup
constexpr int kCornerMaxBlocks = 1024;                        // partial maxima

// max over the workgroup (NaN never wins); every thread gets the result.
__device__ __forceinline__ float block_max(float v, float *lds) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = lds[0];
  for (int k = 1; k < static_cast<int>(blockDim.x >> 6); ++k) r = fmaxf(r, lds[k]);
  return r;
}

// Inclusive sum scan over the workgroup's 256 threads; *total gets the sum.
__device__ __forceinline__ int block_scan(int v, int *lds, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < kCornerThreads / 64; ++k) {
    if (k < wave) before += lds[k];
    all += lds[k];
  }
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(kCornerThreads) void k_corner_max(const float *H, int64_t n,
                                                               float *partial) {
  __shared__ float lds[kCornerThreads / 64];
  float v = -INFINITY;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kCornerThreads + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kCornerThreads)
    v = fmaxf(v, H[i]);
  v = block_max(v, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// The threshold rel * (double)max(H), from the partial maxima (the same expression in both
// passes, so both see the same value).
__device__ __forceinline__ double corner_threshold(const float *partial, int nparts, double rel,
                                                   float *lds) {
  float v = -INFINITY;
  for (int i = threadIdx.x; i < nparts; i += kCornerThreads) v = fmaxf(v, partial[i]);
  return rel * static_cast<double>(block_max(v, lds));
}

__device__ __forceinline__ unsigned corner_flags(const float *H, int64_t n, int64_t base,
                                                 double thr) {
  unsigned f = 0;
  for (int k = 0; k < kCornerItems; ++k) {
    const int64_t i = base + k;
    if (i < n && static_cast<double>(H[i]) > thr) f |= 1u << k;
  }
  return f;
}

__global__ __launch_bounds__(kCornerThreads) void k_corner_count(const float *H, int64_t n,
                                                                 const float *partial, int nparts,
                                                                 double rel, int32_t *counts) {
  __shared__ float fl[kCornerThreads / 64];
  __shared__ int il[kCornerThreads / 64];
  const double thr = corner_threshold(partial, nparts, rel, fl);
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kCornerChunk + threadIdx.x * kCornerItems;
  int total;
  block_scan(__popc(corner_flags(H, n, base, thr)), il, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// One workgroup: counts[0 .. nb) -> exclusive offsets in place, the total in counts[nb].
__global__ __launch_bounds__(kCornerThreads) void k_corner_scan(int32_t *counts, int nb) {
  __shared__ int il[kCornerThreads / 64];
  int carry = 0;
  for (int at = 0; at < nb; at += kCornerThreads) {
    const int i = at + threadIdx.x;
    const int v = i < nb ? counts[i] : 0;
    int total;
    const int incl = block_scan(v, il, &total);
    if (i < nb) counts[i] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) counts[nb] = carry;
}

__global__ __launch_bounds__(kCornerThreads) void k_corner_write(const float *H, int64_t n, int w,
                                                                 const float *partial, int nparts,
                                                                 double rel, const int32_t *offsets,
                                                                 int32_t *xs, int32_t *ys) {
  __shared__ float fl[kCornerThreads / 64];
  __shared__ int il[kCornerThreads / 64];
  const double thr = corner_threshold(partial, nparts, rel, fl);
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kCornerChunk + threadIdx.x * kCornerItems;
  const unsigned f = corner_flags(H, n, base, thr);
  const int cnt = __popc(f);
  int total;
  int at = offsets[blockIdx.x] + block_scan(cnt, il, &total) - cnt;
  for (int k = 0; k < kCornerItems; ++k) {
    if (f & (1u << k)) {
      const int64_t i = base + k;      // i < n, and the hits before it are exactly `at`
      ys[at] = static_cast<int32_t>(i / w);
      xs[at] = static_cast<int32_t>(i % w);
      ++at;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Patch matching
// ------------------------------------------------------------------------------------------
constexpr int kMatchTile = 64;      // pairs per side of a workgroup's tile
constexpr int kMatchThreads = 256;  // 16 x 16 threads, 4 x 4 pairs each
constexpr int kMatchRoiMax = RS_MATCH_MAX_ROI;

template <typename T>
struct MatchTraits;
template <>
struct MatchTraits<uint8_t> {
  using Acc = uint32_t;
  static constexpr int kChunk = kMatchRoiMax * kMatchRoiMax;   // all elements at once
};
template <>
struct MatchTraits<double> {
  using Acc = double;
  static constexpr int kChunk = 32;
};

template <typename T>
struct MatchArgs {
  const T *img1, *img2;
  const int32_t *xy1, *xy2;    // (2, n): x row, y row
  int w1, w2, n1, n2;
  int roi, wrap;
  double *M;                   // (n1, n2) or null
  double *row_val, *col_val;   // [nt2][n1], [nt1][n2] partial minima
  int32_t *row_idx, *col_idx;
};

__device__ __forceinline__ uint32_t match_sq(uint8_t a, uint8_t b, int wrap) {
  int d = static_cast<int>(a) - static_cast<int>(b);
  if (wrap) d &= 255;          // uint8 arithmetic of roi1[i] - roi2[j] (fun.py:118)
  return static_cast<uint32_t>(d * d);
}
__device__ __forceinline__ double match_sq(double a, double b, int) {
  const double d = a - b;
  return d * d;
}

// Four consecutive patches of one element (p is a multiple of 4 elements from a 16-byte base):
// bytes come as one LDS word.
__device__ __forceinline__ void match_load4(const uint8_t *p, uint8_t *out) {
  const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
  for (int q = 0; q < 4; ++q) out[q] = static_cast<uint8_t>(w >> (8 * q));
}
__device__ __forceinline__ void match_load4(const double *p, double *out) {
#pragma unroll
  for (int q = 0; q < 4; ++q) out[q] = p[q];
}

template <typename T>
__global__ __launch_bounds__(kMatchThreads) void k_match(MatchArgs<T> A) {
  using Acc = typename MatchTraits<T>::Acc;
  constexpr int kChunk = MatchTraits<T>::kChunk;
  __shared__ __align__(16) T pa[kChunk * kMatchTile];
  __shared__ __align__(16) T pb[kChunk * kMatchTile];
  __shared__ int ca[2 * kMatchTile], cb[2 * kMatchTile];      // top-left corners (x, y), -1: none
  __shared__ double red_val[kMatchTile * 16];
  __shared__ int red_idx[kMatchTile * 16];

  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * kMatchTile, j0 = blockIdx.x * kMatchTile;
  const int roi = A.roi, m = roi / 2, ne = roi * roi;

  if (tid < kMatchTile) {
    const int i = i0 + tid;
    ca[tid] = i < A.n1 ? A.xy1[i] - m : -1;
    ca[kMatchTile + tid] = i < A.n1 ? A.xy1[A.n1 + i] - m : -1;
  } else if (tid < 2 * kMatchTile) {
    const int t = tid - kMatchTile, j = j0 + t;
    cb[t] = j < A.n2 ? A.xy2[j] - m : -1;
    cb[kMatchTile + t] = j < A.n2 ? A.xy2[A.n2 + j] - m : -1;
  }

  Acc acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0;

  for (int e0 = 0; e0 < ne; e0 += kChunk) {
    const int ec = min(kChunk, ne - e0);
    __syncthreads();   // the corners are there; the previous chunk has been consumed
    for (int idx = tid; idx < ec * kMatchTile; idx += kMatchThreads) {
      const int p = idx & (kMatchTile - 1), e = e0 + idx / kMatchTile;
      const int ey = e / roi, ex = e - ey * roi;
      const int ax = ca[p], bx = cb[p];
      pa[idx] = ax < 0 ? T(0)
                       : A.img1[static_cast<size_t>(ca[kMatchTile + p] + ey) * A.w1 + ax + ex];
      pb[idx] = bx < 0 ? T(0)
                       : A.img2[static_cast<size_t>(cb[kMatchTile + p] + ey) * A.w2 + bx + ex];
    }
    __syncthreads();
    for (int e = 0; e < ec; ++e) {
      T a[4], b[4];
      match_load4(pa + e * kMatchTile + ty * 4, a);
      match_load4(pb + e * kMatchTile + tx * 4, b);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] += match_sq(a[r], b[c], A.wrap);
    }
  }

  // M = sqrt(d2); pairs outside the grid count as +inf and never win a minimum
  double v[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty * 4 + r, j = j0 + tx * 4 + c;
      const bool in = i < A.n1 && j < A.n2;
      v[r][c] = in ? sqrt(static_cast<double>(acc[r][c])) : INFINITY;
      if (in && A.M) A.M[static_cast<size_t>(i) * A.n2 + j] = v[r][c];
    }

  // rows: the thread's 4 columns in ascending order, then the 16 threads of the row
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double bv = v[r][0];
    int bi = 0;
#pragma unroll
    for (int c = 1; c < 4; ++c)
      if (v[r][c] < bv) bv = v[r][c], bi = c;
    red_val[(ty * 4 + r) * 16 + tx] = bv;
    red_idx[(ty * 4 + r) * 16 + tx] = j0 + tx * 4 + bi;
  }
  __syncthreads();
  if (tid < kMatchTile && i0 + tid < A.n1) {
    double bv = red_val[tid * 16];
    int bi = red_idx[tid * 16];
    for (int k = 1; k < 16; ++k)
      if (red_val[tid * 16 + k] < bv) bv = red_val[tid * 16 + k], bi = red_idx[tid * 16 + k];
    A.row_val[static_cast<size_t>(blockIdx.x) * A.n1 + i0 + tid] = bv;
    A.row_idx[static_cast<size_t>(blockIdx.x) * A.n1 + i0 + tid] = bi;
  }
  __syncthreads();
  // columns: the thread's 4 rows in ascending order, then the 16 threads of the column
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double bv = v[0][c];
    int bi = 0;
#pragma unroll
    for (int r = 1; r < 4; ++r)
      if (v[r][c] < bv) bv = v[r][c], bi = r;
    red_val[(tx * 4 + c) * 16 + ty] = bv;
    red_idx[(tx * 4 + c) * 16 + ty] = i0 + ty * 4 + bi;
  }
  __syncthreads();
  if (tid < kMatchTile && j0 + tid < A.n2) {
    double bv = red_val[tid * 16];
    int bi = red_idx[tid * 16];
    for (int k = 1; k < 16; ++k)
      if (red_val[tid * 16 + k] < bv) bv = red_val[tid * 16 + k], bi = red_idx[tid * 16 + k];
    A.col_val[static_cast<size_t>(blockIdx.y) * A.n2 + j0 + tid] = bv;
    A.col_idx[static_cast<size_t>(blockIdx.y) * A.n2 + j0 + tid] = bi;
  }
}

// Element t < n1 is row t (over nt2 partials), the rest are the columns (over nt1 partials).
__global__ __launch_bounds__(256) void k_match_argmin(const double *row_val, const int32_t *row_idx,
                                                      const double *col_val, const int32_t *col_idx,
                                                      int n1, int n2, int nt1, int nt2,
                                                      int32_t *row_min, double *row_minval,
                                                      int32_t *col_min) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n1 + n2) return;
  const bool is_row = t < n1;
  const int at = is_row ? t : t - n1, stride = is_row ? n1 : n2, parts = is_row ? nt2 : nt1;
  const double *val = is_row ? row_val : col_val;
  const int32_t *idx = is_row ? row_idx : col_idx;
  double bv = val[at];
  int bi = idx[at];
  for (int k = 1; k < parts; ++k) {
    const double x = val[static_cast<size_t>(k) * stride + at];
    if (x < bv) bv = x, bi = idx[static_cast<size_t>(k) * stride + at];
  }
  if (is_row) {
    row_min[at] = bi;
    row_minval[at] = bv;
  } else {
    col_min[at] = bi;
  }
}

}  // namespace rsd

namespace {

bool image_size_ok(int64_t h, int64_t w) {
  return h >= 1 && w >= 1 && h <= RS_IMAGE_MAX_SIDE && w <= RS_IMAGE_MAX_SIDE;
}

}  // namespace

extern "C" int rs_harris(rs_ctx *c, const uint8_t *image, int64_t h, int64_t w, int32_t block_size,
                         int32_t kernel_size, double k, int32_t raw, float *out) {
  if (!c || !image || !out) return fail(RS_EINVAL, "null pointer");
  if (kernel_size != 1 && kernel_size != 3 && kernel_size != 5 && kernel_size != 7)
    return fail(RS_EINVAL, "kernel_size must be 1, 3, 5, or 7");
  if (block_size < 1 || block_size > RS_HARRIS_MAX_BLOCK)
    return fail(RS_EINVAL, "block_size must be between 1 and RS_HARRIS_MAX_BLOCK");
  if (!std::isfinite(k)) return fail(RS_EINVAL, "k must be finite");
  if (!image_size_ok(h, w)) return fail(RS_EINVAL, "bad image size");
  rsd::HarrisArgs A;
  A.r = kernel_size == 1 ? 1 : kernel_size / 2;
  A.R = A.r + block_size;
  if (h <= A.R || w <= A.R)
    return fail(RS_EINVAL, "the image must be larger than kernel_size / 2 + block_size per side");

  const size_t npx = static_cast<size_t>(h) * w;
  HIP_TRY(hipSetDevice(c->device));
  rs::Layout L;
  const auto b_img = L.add<uint8_t>(npx);
  const auto b_out = L.add<float>(npx);
  int st = L.bind(c, 0);
  if (st) return st;
  A.img = b_img.dev();
  A.out = b_out.dev();
  A.h = static_cast<int>(h);
  A.w = static_cast<int>(w);
  A.bs = block_size;
  A.ks = kernel_size;
  A.k = k;
  const double s = 1.0 / (static_cast<double>(1 << (kernel_size - 1)) * block_size * 255.0);
  A.s2 = s * s;
  A.raw = raw;
  const int DW = rsd::kHarrisTW + block_size - 1, DH = rsd::kHarrisTH + block_size - 1;
  const int IW = rsd::kHarrisTW + 2 * A.R, IH = rsd::kHarrisTH + 2 * A.R;
  const size_t lds = sizeof(int32_t) * 2 * DW * DH + static_cast<size_t>(IW) * IH;
  hipStream_t s_ = c->stream;
  HIP_TRY(hipMemcpyAsync(b_img.dev(), image, npx, hipMemcpyHostToDevice, s_));
  const dim3 grid((A.w + rsd::kHarrisTW - 1) / rsd::kHarrisTW,
                  (A.h + rsd::kHarrisTH - 1) / rsd::kHarrisTH);
  if ((st = c->feat.mark(0, s_))) return st;
  hipLaunchKernelGGL(rsd::k_harris, grid, dim3(rsd::kHarrisThreads), lds, s_, A);
  HIP_TRY(hipGetLastError());
  if ((st = c->feat.mark(1, s_))) return st;
  HIP_TRY(hipMemcpyAsync(out, A.out, npx * sizeof(float), hipMemcpyDeviceToHost, s_));
  HIP_TRY(hipStreamSynchronize(s_));
  return c->feat.read(0, 0, 1);
}

extern "C" int rs_non_max_suppression(rs_ctx *c, const float *image, int64_t h, int64_t w,
                                      int32_t window_size, float *out) {
  if (!c || !image || !out) return fail(RS_EINVAL, "null pointer");
  if (window_size < 1 || window_size % 2 != 1) return fail(RS_EINVAL, "window_size must be odd");
  if (!image_size_ok(h, w)) return fail(RS_EINVAL, "bad image size");
  const size_t bytes = static_cast<size_t>(h) * w * sizeof(float);
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = static_cast<size_t>(h) * w;
  rs::Layout L;
  const auto b_in = L.add<float>(npx), b_out = L.add<float>(npx);
  int st = L.bind(c, 0);
  if (st) return st;
  float *d_in = b_in.dev(), *d_out = b_out.dev();
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_in, image, bytes, hipMemcpyHostToDevice, s));
  // a window wider than the image leaves no valid position: m is capped so that y + m stays small
  const int m = static_cast<int>(std::min<int64_t>((window_size - 1) / 2, RS_IMAGE_MAX_SIDE));
  const dim3 grid(static_cast<unsigned>((w + 31) / 32), static_cast<unsigned>((h + 7) / 8));
  if ((st = c->feat.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_nms, grid, dim3(256), 0, s, d_in, d_out, static_cast<int>(h),
                     static_cast<int>(w), m);
  HIP_TRY(hipGetLastError());
  if ((st = c->feat.mark(1, s))) return st;
  HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return c->feat.read(0, 0, 1);
}

extern "C" int rs_corners(rs_ctx *c, const float *H, int64_t h, int64_t w, double rel, int32_t *xy,
                          int64_t cap, int64_t *count) {
  if (!c || !H || !count || (cap > 0 && !xy)) return fail(RS_EINVAL, "null pointer");
  if (!image_size_ok(h, w)) return fail(RS_EINVAL, "bad image size");
  if (!std::isfinite(rel)) return fail(RS_EINVAL, "rel must be finite");
  if (cap < 0) return fail(RS_EINVAL, "bad capacity");
  const int64_t n = h * w;   // <= 2^30
  const int nb = static_cast<int>((n + rsd::kCornerChunk - 1) / rsd::kCornerChunk);
  const int nparts = std::min(nb, rsd::kCornerMaxBlocks);
  rs::Layout L;
  const auto b_H = L.add<float>(n), b_part = L.add<float>(rsd::kCornerMaxBlocks);
  const auto b_cnt = L.add<int32_t>(nb + 1);
  const auto b_xs = L.add<int32_t>(n), b_ys = L.add<int32_t>(n);
  HIP_TRY(hipSetDevice(c->device));
  int st = L.bind(c, 0);
  if (st) return st;
  float *d_H = b_H.dev(), *d_part = b_part.dev();
  int32_t *d_cnt = b_cnt.dev(), *d_xs = b_xs.dev(), *d_ys = b_ys.dev();
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_H, H, n * sizeof(float), hipMemcpyHostToDevice, s));
  const dim3 blk(rsd::kCornerThreads);
  if ((st = c->feat.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_corner_max, dim3(nparts), blk, 0, s, d_H, n, d_part);
  hipLaunchKernelGGL(rsd::k_corner_count, dim3(nb), blk, 0, s, d_H, n, d_part, nparts, rel, d_cnt);
  hipLaunchKernelGGL(rsd::k_corner_scan, dim3(1), blk, 0, s, d_cnt, nb);
  hipLaunchKernelGGL(rsd::k_corner_write, dim3(nb), blk, 0, s, d_H, n, static_cast<int>(w), d_part,
                     nparts, rel, d_cnt, d_xs, d_ys);
  HIP_TRY(hipGetLastError());
  if ((st = c->feat.mark(1, s))) return st;
  int32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_cnt + nb, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->feat.read(0, 0, 1))) return st;
  *count = total;
  if (total > cap) return fail(RS_EINVAL, "more corners than the capacity of xy");
  if (total > 0) {
    HIP_TRY(hipMemcpyAsync(xy, d_xs, sizeof(int32_t) * total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(xy + cap, d_ys, sizeof(int32_t) * total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return RS_OK;
}

namespace {

int centres_check(const int32_t *xy, int64_t n, int64_t h, int64_t w, int m) {
  for (int64_t i = 0; i < n; ++i) {
    const int32_t x = xy[i], y = xy[n + i];
    if (x < m || y < m || x >= w - m || y >= h - m)
      return fail(RS_EINVAL, "a patch centre is too close to the image border");
  }
  return RS_OK;
}

template <typename T>
int match_run(rs_ctx *c, const T *img1, int64_t h1, int64_t w1, const int32_t *xy1, int64_t n1,
              const T *img2, int64_t h2, int64_t w2, const int32_t *xy2, int64_t n2,
              int32_t roi_size, int32_t wrap, int32_t *row_min, int32_t *col_min, double *row_val,
              double *M) {
  if (!c || !img1 || !img2 || !xy1 || !xy2 || !row_min || !col_min || !row_val)
    return fail(RS_EINVAL, "null pointer");
  if (roi_size < 1 || roi_size % 2 != 1) return fail(RS_EINVAL, "ROI size must be odd");
  if (roi_size > RS_MATCH_MAX_ROI) return fail(RS_EINVAL, "ROI size above RS_MATCH_MAX_ROI");
  if (!image_size_ok(h1, w1) || !image_size_ok(h2, w2)) return fail(RS_EINVAL, "bad image size");
  if (n1 < 1 || n2 < 1 || n1 > RS_MATCH_MAX_N || n2 > RS_MATCH_MAX_N)
    return fail(RS_EINVAL, "n1 and n2 must be between 1 and RS_MATCH_MAX_N");
  if (M && n1 * n2 > RS_MATCH_MAX_PAIRS)
    return fail(RS_EINVAL, "n1 * n2 above RS_MATCH_MAX_PAIRS with the matrix requested");
  const int m = roi_size / 2;
  int st = centres_check(xy1, n1, h1, w1, m);
  if (st) return st;
  st = centres_check(xy2, n2, h2, w2, m);
  if (st) return st;

  const int nt1 = static_cast<int>((n1 + rsd::kMatchTile - 1) / rsd::kMatchTile);
  const int nt2 = static_cast<int>((n2 + rsd::kMatchTile - 1) / rsd::kMatchTile);
  const size_t D = sizeof(double);
  rs::Layout L;
  const auto b_img1 = L.add<T>(h1 * w1), b_img2 = L.add<T>(h2 * w2);
  const auto b_xy1 = L.add<int32_t>(2 * n1), b_xy2 = L.add<int32_t>(2 * n2);
  // the partial minima per tile row / column, then the results
  const auto b_row_val = L.add<double>(nt2 * n1), b_col_val = L.add<double>(nt1 * n2);
  const auto b_row_idx = L.add<int32_t>(nt2 * n1), b_col_idx = L.add<int32_t>(nt1 * n2);
  const auto b_rmin = L.add<int32_t>(n1), b_cmin = L.add<int32_t>(n2);
  const auto b_rval = L.add<double>(n1);
  HIP_TRY(hipSetDevice(c->device));
  st = L.bind(c, 0);
  if (st) return st;
  double *d_M = nullptr;   // the matrix is not kept in the grow-only scratch
  if (M) HIP_TRY(hipMalloc(&d_M, D * n1 * n2));

  hipStream_t s = c->stream;
  rsd::MatchArgs<T> A;
  A.img1 = b_img1.dev();
  A.img2 = b_img2.dev();
  A.xy1 = b_xy1.dev();
  A.xy2 = b_xy2.dev();
  A.w1 = static_cast<int>(w1);
  A.w2 = static_cast<int>(w2);
  A.n1 = static_cast<int>(n1);
  A.n2 = static_cast<int>(n2);
  A.roi = roi_size;
  A.wrap = wrap ? 1 : 0;
  A.M = d_M;
  A.row_val = b_row_val.dev();
  A.col_val = b_col_val.dev();
  A.row_idx = b_row_idx.dev();
  A.col_idx = b_col_idx.dev();
  int32_t *d_rmin = b_rmin.dev(), *d_cmin = b_cmin.dev();
  double *d_rval = b_rval.dev();

  // one error path, so that the matrix is freed: the timer's events are recorded by hand
  hipError_t e = hipMemcpyAsync(b_img1.dev(), img1, b_img1.bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(b_img2.dev(), img2, b_img2.bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(b_xy1.dev(), xy1, b_xy1.bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(b_xy2.dev(), xy2, b_xy2.bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && c->feat.on) e = hipEventRecord(c->feat.ev[0], s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(rsd::k_match<T>, dim3(nt2, nt1), dim3(rsd::kMatchThreads), 0, s, A);
    hipLaunchKernelGGL(rsd::k_match_argmin, dim3(static_cast<unsigned>((n1 + n2 + 255) / 256)),
                       dim3(256), 0, s, A.row_val, A.row_idx, A.col_val, A.col_idx, A.n1, A.n2,
                       nt1, nt2, d_rmin, d_rval, d_cmin);
    e = hipGetLastError();
  }
  if (e == hipSuccess && c->feat.on) e = hipEventRecord(c->feat.ev[1], s);
  if (e == hipSuccess) e = hipMemcpyAsync(row_min, d_rmin, b_rmin.bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(col_min, d_cmin, b_cmin.bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(row_val, d_rval, b_rval.bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && M) e = hipMemcpyAsync(M, d_M, D * n1 * n2, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (d_M) (void)hipFree(d_M);
  if (e != hipSuccess) return hip_fail(e, "rs_match_rois");
  return c->feat.read(0, 0, 1);
}

}  // namespace

extern "C" int rs_match_rois_u8(rs_ctx *c, const uint8_t *img1, int64_t h1, int64_t w1,
                                const int32_t *xy1, int64_t n1, const uint8_t *img2, int64_t h2,
                                int64_t w2, const int32_t *xy2, int64_t n2, int32_t roi_size,
                                int32_t wrap, int32_t *row_min, int32_t *col_min, double *row_val,
                                double *M) {
  return match_run<uint8_t>(c, img1, h1, w1, xy1, n1, img2, h2, w2, xy2, n2, roi_size, wrap,
                            row_min, col_min, row_val, M);
}

extern "C" int rs_match_rois_f64(rs_ctx *c, const double *img1, int64_t h1, int64_t w1,
                                 const int32_t *xy1, int64_t n1, const double *img2, int64_t h2,
                                 int64_t w2, const int32_t *xy2, int64_t n2, int32_t roi_size,
                                 int32_t *row_min, int32_t *col_min, double *row_val, double *M) {
  return match_run<double>(c, img1, h1, w1, xy1, n1, img2, h2, w2, xy2, n2, roi_size, 0, row_min,
                           col_min, row_val, M);
}

// An event before the first and after the last kernel of a call, read after the call's
// synchronise.
extern "C" int rs_features_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->feat.enable(enable != 0);
  if (st) return st;
  c->feat.copy_out(ms);
  return RS_OK;
}
