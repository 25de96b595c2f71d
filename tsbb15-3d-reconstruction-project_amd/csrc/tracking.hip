// The tracking stage on the GPU: a pyramidal Lucas-Kanade tracker, by the definition in
// include/rsamd.h ("The tracking stage").  Integer pyramids, integer Sobel gradients, 14-bit
// bilinear weights and exact int64 window sums; the few fp64 steps are written in the header's
// order and compiled without contraction, so the results are the restatement's bit for bit.
//
// k_pyr_down     one output pixel per lane: the 5 x 5 binomial sum of the level below around
//                (2 y, 2 x), reflect-101, (S + 128) >> 8.
// k_klt_track<R> one wave per feature, four features per workgroup, all levels of a feature in one
//                launch.  Window pixel e = 64 k + lane belongs to round k < R of its lane (R = 1,
//                2, 4, 8, 16: the smallest with 64 R >= window^2), and the lane keeps T, Gx, Gy of
//                its pixels in registers while the feature iterates at a level.  Image 1 is read
//                through the cache: four bytes per window pixel and iteration.  The int64 sums
//                of a step are reduced by a butterfly over the wave, after which every lane
//                holds the same integers, evaluates the same fp64 update and takes the same
//                branch.  Features of a workgroup finish after different numbers of iterations:
//                nothing in the kernel is a workgroup barrier, the waves never meet.
//                The backward launch of the forward-backward test is the same kernel with the
//                two pyramids exchanged, started from the forward results.
#include <hip/hip_runtime.h>

#include <cmath>

#include "host.h"

namespace rsd {

constexpr int kKltWavesPerBlock = 4;
constexpr int kKltThreads = 64 * kKltWavesPerBlock;

// Reflect-101 for -n < p < 2 n - 1; the clamp only keeps a coordinate nobody uses legal.
__device__ __forceinline__ int trk_reflect(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * (n - 1) - p;
  return min(max(p, 0), n - 1);
}

__global__ __launch_bounds__(256) void k_pyr_down(const uint8_t *in, int h, int w, uint8_t *out,
                                                  int oh, int ow) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= ow || y >= oh) return;
  const int taps[5] = {1, 4, 6, 4, 1};
  int cols[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) cols[j] = trk_reflect(2 * x - 2 + j, w);
  int S = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint8_t *row = in + static_cast<size_t>(trk_reflect(2 * y - 2 + i, h)) * w;
    int rs = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) rs += taps[j] * row[cols[j]];
    S += taps[i] * rs;
  }
  out[static_cast<size_t>(y) * ow + x] = static_cast<uint8_t>((S + 128) >> 8);
}

struct KltArgs {
  const uint8_t *from, *to;          // the pyramids: template image, searched image
  int w[RS_KLT_MAX_LEVELS], h[RS_KLT_MAX_LEVELS];
  long long off[RS_KLT_MAX_LEVELS];  // start of a level in its pyramid
  double scale[RS_KLT_MAX_LEVELS];   // 2^-l
  const double *pts;                 // (2, n) starts
  const double *guess;               // (2, n) or null
  const double *orig;                // backward: the forward starts the results are compared with
  int n, r, levels, max_iter, backward;
  double eps2, tau, fb_tol;
  double *pos;                       // (2, n)
  int32_t *status, *iters;
  double *resid, *fb;
};

struct KltWeights {
  int ix, iy, w00, w01, w10, w11;
};

__device__ __forceinline__ bool klt_inside(double qx, double qy, int w, int h, int r) {
  return qx >= static_cast<double>(r) && qx < static_cast<double>(w - 1 - r) &&
         qy >= static_cast<double>(r) && qy < static_cast<double>(h - 1 - r);
}

// (qx, qy) is inside: the conversions are safe
__device__ __forceinline__ KltWeights klt_weights(double qx, double qy) {
#pragma clang fp contract(off)
  const double fx = floor(qx), fy = floor(qy);
  const double a = qx - fx, b = qy - fy;
  KltWeights t;
  t.ix = static_cast<int>(fx);
  t.iy = static_cast<int>(fy);
  t.w00 = static_cast<int>(floor(((1.0 - a) * (1.0 - b)) * 16384.0 + 0.5));
  t.w01 = static_cast<int>(floor((a * (1.0 - b)) * 16384.0 + 0.5));
  t.w10 = static_cast<int>(floor(((1.0 - a) * b) * 16384.0 + 0.5));
  t.w11 = 16384 - t.w00 - t.w01 - t.w10;
  return t;
}

__device__ __forceinline__ int klt_mix(const KltWeights &t, int v00, int v01, int v10, int v11) {
  return (t.w00 * v00 + t.w01 * v01 + t.w10 * v10 + t.w11 * v11 + 256) >> 9;
}

// the grey sample whose top-left pixel is (y, x); (y + 1, x + 1) is inside the level
__device__ __forceinline__ int klt_grey(const uint8_t *v, int w, int y, int x,
                                        const KltWeights &t) {
  const uint8_t *p = v + static_cast<size_t>(y) * w + x;
  return klt_mix(t, p[0], p[1], p[w], p[w + 1]);
}

// the samples of the Sobel pair: the 4 x 4 pixels around the cell give the gradients at its four
// corners
__device__ __forceinline__ void klt_grad(const uint8_t *v, int w, int h, int y, int x,
                                         const KltWeights &t, int *gx, int *gy) {
  int u[4][4], cx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cx[j] = trk_reflect(x - 1 + j, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint8_t *row = v + static_cast<size_t>(trk_reflect(y - 1 + i, h)) * w;
#pragma unroll
    for (int j = 0; j < 4; ++j) u[i][j] = row[cx[j]];
  }
  int sx[2][2], sy[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      sx[i][j] = (u[i][j + 2] - u[i][j]) + 2 * (u[i + 1][j + 2] - u[i + 1][j]) +
                 (u[i + 2][j + 2] - u[i + 2][j]);
      sy[i][j] = (u[i + 2][j] - u[i][j]) + 2 * (u[i + 2][j + 1] - u[i][j + 1]) +
                 (u[i + 2][j + 2] - u[i][j + 2]);
    }
  *gx = klt_mix(t, sx[0][0], sx[0][1], sx[1][0], sx[1][1]);
  *gy = klt_mix(t, sy[0][0], sy[0][1], sy[1][0], sy[1][1]);
}

// every lane gets the sum over the wave
__device__ __forceinline__ long long klt_wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct KltResult {
  int status, iters;
  double x, y, resid;
};

// One feature from pyramid `from` into pyramid `to`; every lane of the wave returns the same.
template <int R>
__device__ __forceinline__ KltResult klt_feature(const KltArgs &A, const uint8_t *from,
                                                 const uint8_t *to, double px, double py,
                                                 double gx, double gy, int lane) {
#pragma clang fp contract(off)
  const int r = A.r, W = 2 * r + 1, n = W * W;
  KltResult out;
  out.status = RS_KLT_LOST;
  out.iters = 0;
  out.x = out.y = out.resid = -1.0;

  // window offsets (i, j) in -r .. r of the lane's pixels, packed; the pixels e >= n do not exist
  int dij[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int e = min(k * 64 + lane, n - 1), i = e / W;
    dij[k] = (i - r) * 256 + (e - i * W - r + 128);
  }
  int T[R], Gx[R], Gy[R];
#pragma unroll
  for (int k = 0; k < R; ++k) T[k] = Gx[k] = Gy[k] = 0;

  for (int l = A.levels - 1; l >= 0; --l) {
    const int w = A.w[l], h = A.h[l];
    const uint8_t *va = from + A.off[l], *vb = to + A.off[l];
    const double plx = px * A.scale[l], ply = py * A.scale[l];
    if (!klt_inside(plx, ply, w, h, r)) {
      if (l == 0) return out;
      gx = 2.0 * gx;
      gy = 2.0 * gy;
      continue;
    }
    const KltWeights t = klt_weights(plx, ply);
    long long sA = 0, sB = 0, sC = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (k * 64 + lane < n) {
        const int y = t.iy + (dij[k] >> 8), x = t.ix + (dij[k] & 255) - 128;
        T[k] = klt_grey(va, w, y, x, t);
        klt_grad(va, w, h, y, x, t, &Gx[k], &Gy[k]);
        sA += static_cast<long long>(Gx[k]) * Gx[k];
        sB += static_cast<long long>(Gx[k]) * Gy[k];
        sC += static_cast<long long>(Gy[k]) * Gy[k];
      }
    }
    const double a = static_cast<double>(klt_wave_sum(sA));
    const double b = static_cast<double>(klt_wave_sum(sB));
    const double c = static_cast<double>(klt_wave_sum(sC));
    const double det = a * c - b * b;
    const bool textured =
        a + c >= 2.0 * A.tau && (a - A.tau) * (c - A.tau) - b * b >= 0.0 && det > 0.0;
    if (!textured) {
      if (l == 0) {
        out.status = RS_KLT_FLAT;
        return out;
      }
      gx = 2.0 * gx;
      gy = 2.0 * gy;
      continue;
    }
    double d0 = gx, d1 = gy;
    for (int it = 0; it < A.max_iter; ++it) {
      const double qx = plx + d0, qy = ply + d1;
      if (!klt_inside(qx, qy, w, h, r)) {
        if (l == 0) return out;
        break;
      }
      const KltWeights u = klt_weights(qx, qy);
      long long sx = 0, sy = 0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (k * 64 + lane < n) {
          const int y = u.iy + (dij[k] >> 8), x = u.ix + (dij[k] & 255) - 128;
          const int e = T[k] - klt_grey(vb, w, y, x, u);
          sx += e * Gx[k];   // |e Gx| <= 8160 * 32640 < 2^31
          sy += e * Gy[k];
        }
      }
      const double bx = static_cast<double>(klt_wave_sum(sx));
      const double by = static_cast<double>(klt_wave_sum(sy));
      const double dx = (8.0 * (c * bx - b * by)) / det;
      const double dy = (8.0 * (a * by - b * bx)) / det;
      d0 = d0 + dx;
      d1 = d1 + dy;
      if (l == 0) ++out.iters;
      if (dx * dx + dy * dy <= A.eps2) break;
    }
    gx = l > 0 ? 2.0 * d0 : d0;
    gy = l > 0 ? 2.0 * d1 : d1;
    if (l == 0) {
      const double qx = plx + gx, qy = ply + gy;
      if (!klt_inside(qx, qy, w, h, r)) return out;
      const KltWeights u = klt_weights(qx, qy);
      long long sr = 0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        if (k * 64 + lane < n) {
          const int y = u.iy + (dij[k] >> 8), x = u.ix + (dij[k] & 255) - 128;
          sr += abs(T[k] - klt_grey(vb, w, y, x, u));
        }
      }
      out.resid = static_cast<double>(klt_wave_sum(sr)) / static_cast<double>(32 * n);
      out.x = qx;
      out.y = qy;
      out.status = RS_KLT_OK;
    }
  }
  return out;
}

template <int R>
__global__ __launch_bounds__(kKltThreads) void k_klt_track(KltArgs A) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * kKltWavesPerBlock + (threadIdx.x >> 6);
  if (f >= A.n) return;   // the whole wave
  const double px = A.pts[f], py = A.pts[A.n + f];
  double gx = 0.0, gy = 0.0;
  if (A.backward) {
    if (A.status[f] != RS_KLT_OK) {
      if (lane == 0) A.fb[f] = -1.0;
      return;
    }
  } else if (A.guess) {
    gx = A.guess[f];
    gy = A.guess[A.n + f];
  }
  const KltResult res = klt_feature<R>(A, A.from, A.to, px, py, gx, gy, lane);
  if (lane != 0) return;
  if (!A.backward) {
    A.pos[f] = res.x;
    A.pos[A.n + f] = res.y;
    A.status[f] = res.status;
    A.resid[f] = res.resid;
    A.iters[f] = res.iters;
    A.fb[f] = -1.0;
    return;
  }
  double dist = -1.0;
  bool failed = true;
  if (res.status == RS_KLT_OK) {
    dist = fmax(fabs(res.x - A.orig[f]), fabs(res.y - A.orig[A.n + f]));
    failed = dist > A.fb_tol;
  }
  A.fb[f] = dist;
  if (failed) {
    A.status[f] = RS_KLT_FB;
    A.pos[f] = A.pos[A.n + f] = -1.0;
    A.resid[f] = -1.0;
  }
}

void pyr_down_launch(hipStream_t s, const uint8_t *in, int h, int w, uint8_t *out) {
  const int oh = (h + 1) / 2, ow = (w + 1) / 2;
  hipLaunchKernelGGL(k_pyr_down, dim3((ow + 31) / 32, (oh + 7) / 8), dim3(256), 0, s, in, h, w, out,
                     oh, ow);
}

void klt_launch(hipStream_t s, const KltArgs &A) {
  const int npx = (2 * A.r + 1) * (2 * A.r + 1);
  const dim3 grid((A.n + kKltWavesPerBlock - 1) / kKltWavesPerBlock), blk(kKltThreads);
  if (npx <= 64)
    hipLaunchKernelGGL(k_klt_track<1>, grid, blk, 0, s, A);
  else if (npx <= 128)
    hipLaunchKernelGGL(k_klt_track<2>, grid, blk, 0, s, A);
  else if (npx <= 256)
    hipLaunchKernelGGL(k_klt_track<4>, grid, blk, 0, s, A);
  else if (npx <= 512)
    hipLaunchKernelGGL(k_klt_track<8>, grid, blk, 0, s, A);
  else
    hipLaunchKernelGGL(k_klt_track<16>, grid, blk, 0, s, A);
}

}  // namespace rsd

extern "C" int rs_pyr_down(rs_ctx *c, const uint8_t *image, int64_t h, int64_t w, uint8_t *out) {
  if (!c || !image || !out) return fail(RS_EINVAL, "null pointer");
  if (h < 3 || w < 3) return fail(RS_EINVAL, "both sides of a level that is reduced must be at least 3");
  if (h > RS_IMAGE_MAX_SIDE || w > RS_IMAGE_MAX_SIDE) return fail(RS_EINVAL, "bad image size");
  const size_t oh = (h + 1) / 2, ow = (w + 1) / 2;
  HIP_TRY(hipSetDevice(c->device));
  rs::Layout L;
  const auto b_in = L.add<uint8_t>(static_cast<size_t>(h) * w), b_out = L.add<uint8_t>(oh * ow);
  int st = L.bind(c, 0);
  if (st) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_in.dev(), image, b_in.bytes, hipMemcpyHostToDevice, s));
  rsd::pyr_down_launch(s, b_in.dev(), static_cast<int>(h), static_cast<int>(w), b_out.dev());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, b_out.dev(), b_out.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return RS_OK;
}

extern "C" int rs_klt_track(rs_ctx *c, const uint8_t *img0, const uint8_t *img1, int64_t h,
                            int64_t w, const double *pts, const double *guess, int64_t n,
                            int32_t window, int32_t levels, int32_t max_iter, double eps,
                            double min_eig, double fb_tol, double *pos, int32_t *status,
                            double *residual, int32_t *iters, double *fb) {
  if (!c || !img0 || !img1) return fail(RS_EINVAL, "null pointer");
  if (n > 0 && (!pts || !pos || !status || !residual || !iters || !fb))
    return fail(RS_EINVAL, "null pointer");
  if (h < 1 || w < 1 || h > RS_IMAGE_MAX_SIDE || w > RS_IMAGE_MAX_SIDE)
    return fail(RS_EINVAL, "bad image size");
  if (window < 3 || window > RS_KLT_MAX_WINDOW || window % 2 != 1)
    return fail(RS_EINVAL, "window must be odd, between 3 and RS_KLT_MAX_WINDOW");
  if (levels < 1 || levels > RS_KLT_MAX_LEVELS)
    return fail(RS_EINVAL, "levels must be between 1 and RS_KLT_MAX_LEVELS");
  if (max_iter < 1 || max_iter > RS_KLT_MAX_ITER)
    return fail(RS_EINVAL, "max_iter must be between 1 and RS_KLT_MAX_ITER");
  if (!(eps >= 0.0)) return fail(RS_EINVAL, "eps must not be negative");
  if (!std::isfinite(min_eig) || min_eig < 0.0)
    return fail(RS_EINVAL, "min_eig must be finite and not negative");
  if (std::isnan(fb_tol)) return fail(RS_EINVAL, "fb_tol must not be NaN");
  if (n < 0 || n > RS_KLT_MAX_N) return fail(RS_EINVAL, "n must be between 0 and RS_KLT_MAX_N");

  rsd::KltArgs A = {};
  size_t pyr_bytes = 0;
  int64_t lh = h, lw = w;
  for (int l = 0; l < levels; ++l) {
    if (l > 0) {
      if (lh < 3 || lw < 3)
        return fail(RS_EINVAL, "both sides of a level that is reduced must be at least 3");
      lh = (lh + 1) / 2;
      lw = (lw + 1) / 2;
    }
    A.h[l] = static_cast<int>(lh);
    A.w[l] = static_cast<int>(lw);
    A.off[l] = static_cast<long long>(pyr_bytes);
    A.scale[l] = std::ldexp(1.0, -l);
    pyr_bytes += rs::align256(static_cast<size_t>(lh) * lw);
  }
  if (n == 0) return RS_OK;

  const size_t N = static_cast<size_t>(n);
  rs::Layout L;
  const auto b_p0 = L.add<uint8_t>(pyr_bytes), b_p1 = L.add<uint8_t>(pyr_bytes);
  const auto b_pts = L.add<double>(2 * N), b_guess = L.add<double>(guess ? 2 * N : 0);
  const auto b_pos = L.add<double>(2 * N), b_res = L.add<double>(N), b_fb = L.add<double>(N);
  const auto b_status = L.add<int32_t>(N), b_iters = L.add<int32_t>(N);
  HIP_TRY(hipSetDevice(c->device));
  int st = L.bind(c, 0);
  if (st) return st;

  hipStream_t s = c->stream;
  const size_t npx = static_cast<size_t>(h) * w;
  HIP_TRY(hipMemcpyAsync(b_p0.dev(), img0, npx, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_p1.dev(), img1, npx, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_pts.dev(), pts, b_pts.bytes, hipMemcpyHostToDevice, s));
  if (guess) HIP_TRY(hipMemcpyAsync(b_guess.dev(), guess, b_guess.bytes, hipMemcpyHostToDevice, s));
  if ((st = c->track.mark(0, s))) return st;
  for (int l = 1; l < levels; ++l) {
    rsd::pyr_down_launch(s, b_p0.dev() + A.off[l - 1], A.h[l - 1], A.w[l - 1], b_p0.dev() + A.off[l]);
    rsd::pyr_down_launch(s, b_p1.dev() + A.off[l - 1], A.h[l - 1], A.w[l - 1], b_p1.dev() + A.off[l]);
  }
  if ((st = c->track.mark(1, s))) return st;
  A.from = b_p0.dev();
  A.to = b_p1.dev();
  A.pts = b_pts.dev();
  A.guess = guess ? b_guess.dev() : nullptr;
  A.orig = nullptr;
  A.n = static_cast<int>(n);
  A.r = window / 2;
  A.levels = levels;
  A.max_iter = max_iter;
  A.backward = 0;
  A.eps2 = eps * eps;
  A.tau = (min_eig * static_cast<double>(window * window)) * 65536.0;
  A.fb_tol = fb_tol;
  A.pos = b_pos.dev();
  A.status = b_status.dev();
  A.iters = b_iters.dev();
  A.resid = b_res.dev();
  A.fb = b_fb.dev();
  rsd::klt_launch(s, A);
  if ((st = c->track.mark(2, s))) return st;
  if (fb_tol >= 0.0) {
    rsd::KltArgs B = A;
    B.from = A.to;
    B.to = A.from;
    B.pts = A.pos;
    B.guess = nullptr;
    B.orig = A.pts;
    B.backward = 1;
    rsd::klt_launch(s, B);
  }
  HIP_TRY(hipGetLastError());
  if ((st = c->track.mark(3, s))) return st;
  HIP_TRY(hipMemcpyAsync(pos, b_pos.dev(), b_pos.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(residual, b_res.dev(), b_res.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(fb, b_fb.dev(), b_fb.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(status, b_status.dev(), b_status.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(iters, b_iters.dev(), b_iters.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < RS_TRACKING_TIMING_SLOTS; ++k)
    if ((st = c->track.read(k, k, k + 1))) return st;
  if (c->track.on && !(fb_tol >= 0.0)) c->track.ms[2] = -1.0;   // no backward launch
  return RS_OK;
}

extern "C" int rs_tracking_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->track.enable(enable != 0);
  if (st) return st;
  c->track.copy_out(ms);
  return RS_OK;
}
