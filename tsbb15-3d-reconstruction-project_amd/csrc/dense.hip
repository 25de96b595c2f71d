// The dense stage on the GPU: plane-sweep depth maps (rs_dense_plane_sweep) and the
// cross-view depth agreement count that fuses them (rs_dense_consistency).  The definitions
// stand in include/rsamd.h; tests/dense_ref.py restates them in numpy.
//
// k_dense_sweep<R> (R = patch / 2, one instantiation per patch size so the window loops unroll):
//   one workgroup of 256 threads owns a tile of 32 x 8 reference pixels plus an R-wide halo,
//   (32 + 2R) x (8 + 2R) pixels.
//   * The reference tile, shifted by 128, goes into LDS once (s_a).  Every pixel forms sum a and
//     sum a^2 of its window from it once; they are integers, exact in fp32, and the reference-side
//     variance test n sum a^2 - (sum a)^2 >= min_var n^2 is done on int32.
//   * For each plane k and source s every thread warps its (at most three) tile-plus-halo pixels
//     through q = d_k A_s p + b_s in fp64, fetches the bilinear sample as four byte loads (the
//     sources are a few hundred KB and sit in L2), and writes the shifted sample to the LDS tile
//     s_b; an invalid sample is a NaN there.  After a barrier every pixel reads its window from
//     s_a and s_b -- 2n four-byte LDS reads -- and forms sum b, sum b^2, sum ab.  A NaN in the
//     window makes the warped variance NaN, which fails the variance test: "all n samples valid"
//     needs no flag of its own.
//   * A row of the tile is 32 consecutive floats, so the 32 lanes of a read group hit 32
//     different banks whatever the row stride.
//   * The running best, the cost before it, the previous cost and a flag that catches the cost
//     after the best stay in registers; the cost volume is written only when asked for.
//   Every barrier is reached by every thread: pixels outside the image or with a flat reference
//   window skip the arithmetic, never the loop.  Every global index is bounded: the reference
//   tile is read only inside the image, and a source is read only at a sample the validity
//   predicate has placed in [0, w-1] x [0, h-1], with the right and lower neighbour clamped.
//
// k_dense_consistency: one lane per (view, pixel), a loop over the other views, all fp64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "host.h"

namespace rsd {

constexpr int kDenseTX = 32, kDenseTY = 8, kDenseThreads = kDenseTX * kDenseTY;

struct DenseWarp {
  double A[RS_DENSE_MAX_SOURCES][9];
  double b[RS_DENSE_MAX_SOURCES][3];
};

__device__ __forceinline__ float dense_nan() { return __int_as_float(0x7fc00000); }

template <int R>
__global__ __launch_bounds__(kDenseThreads) void k_dense_sweep(
    const uint8_t *ref, const uint8_t *src, int h, int w, int S, DenseWarp W,
    const double *depths, int D, double thr, int32_t *index, float *delta, float *score,
    uint8_t *nvalid, float *volume) {
  constexpr int TW = kDenseTX + 2 * R, TH = kDenseTY + 2 * R, NT = TW * TH;
  constexpr int P = 2 * R + 1, N = P * P;
  constexpr int PER = (NT + kDenseThreads - 1) / kDenseThreads;
  __shared__ float s_a[NT], s_b[NT];
  const int tid = threadIdx.x, tx = tid & (kDenseTX - 1), ty = tid / kDenseTX;
  const int x0t = static_cast<int>(blockIdx.x) * kDenseTX - R;
  const int y0t = static_cast<int>(blockIdx.y) * kDenseTY - R;
  const int64_t hw = static_cast<int64_t>(h) * w;

  // this thread's tile-plus-halo pixels: LDS slot, image position, inside the image or not
  int slot[PER], gx[PER], gy[PER];
  bool inside[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int i = tid + e * kDenseThreads;
    slot[e] = i < NT ? i : -1;
    gx[e] = x0t + i % TW;
    gy[e] = y0t + i / TW;
    inside[e] = i < NT && gx[e] >= 0 && gx[e] < w && gy[e] >= 0 && gy[e] < h;
    if (slot[e] >= 0)
      s_a[i] = inside[e]
                   ? static_cast<float>(static_cast<int>(ref[gy[e] * static_cast<int64_t>(w) + gx[e]]) - 128)
                   : 0.0f;
  }
  __syncthreads();

  const int px = x0t + R + tx, py = y0t + R + ty;
  const bool in_image = px < w && py < h;
  bool ok = px >= R && px < w - R && py >= R && py < h - R;   // the window lies inside
  float Sa = 0.0f, va = 0.0f;
  if (ok) {
    float Saa = 0.0f;
#pragma unroll
    for (int dy = 0; dy < P; ++dy)
#pragma unroll
      for (int dx = 0; dx < P; ++dx) {
        const float a = s_a[(ty + dy) * TW + tx + dx];
        Sa += a;              // integers below 2^24: exact
        Saa += a * a;
      }
    const int iSa = static_cast<int>(Sa), iSaa = static_cast<int>(Saa);
    const int iva = N * iSaa - iSa * iSa;   // at most 121^2 * 128^2 < 2^31
    ok = static_cast<double>(iva) >= thr;
    va = static_cast<float>(iva);
  }
  const float thr_f = static_cast<float>(thr);
  const double wm1 = static_cast<double>(w - 1), hm1 = static_cast<double>(h - 1);

  float best = -INFINITY, before = dense_nan(), after = dense_nan(), prev = dense_nan();
  int best_k = -1, best_nv = 0;
  bool want_next = false;
  for (int k = 0; k < D; ++k) {
    const double d = depths[k];
    float acc = 0.0f;
    int nv = 0;
    for (int s = 0; s < S; ++s) {
      const double *A = W.A[s], *b = W.b[s];
      const uint8_t *im = src + s * hw;
      __syncthreads();   // the previous (k, s)'s window reads are done
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        float v = dense_nan();
        if (inside[e]) {
          const double X = static_cast<double>(gx[e]), Y = static_cast<double>(gy[e]);
          const double q0 = d * (A[0] * X + A[1] * Y + A[2]) + b[0];
          const double q1 = d * (A[3] * X + A[4] * Y + A[5]) + b[1];
          const double q2 = d * (A[6] * X + A[7] * Y + A[8]) + b[2];
          const double xs = q0 / q2, ys = q1 / q2;
          if (q2 * d > 0.0 && xs >= 0.0 && xs <= wm1 && ys >= 0.0 && ys <= hm1) {
            const double xf = floor(xs), yf = floor(ys);
            const int ix = static_cast<int>(xf), iy = static_cast<int>(yf);   // in [0, w-1], [0, h-1]
            const int ix1 = min(ix + 1, w - 1), iy1 = min(iy + 1, h - 1);
            const float fx = static_cast<float>(xs - xf), fy = static_cast<float>(ys - yf);
            const uint8_t *r0 = im + static_cast<int64_t>(iy) * w;
            const uint8_t *r1 = im + static_cast<int64_t>(iy1) * w;
            const float i00 = static_cast<float>(static_cast<int>(r0[ix]) - 128);
            const float i01 = static_cast<float>(static_cast<int>(r0[ix1]) - 128);
            const float i10 = static_cast<float>(static_cast<int>(r1[ix]) - 128);
            const float i11 = static_cast<float>(static_cast<int>(r1[ix1]) - 128);
            const float top = i00 + fx * (i01 - i00);
            const float bot = i10 + fx * (i11 - i10);
            v = top + fy * (bot - top);
          }
        }
        if (slot[e] >= 0) s_b[slot[e]] = v;
      }
      __syncthreads();
      if (ok) {
        float Sb = 0.0f, Sbb = 0.0f, Sab = 0.0f;
#pragma unroll
        for (int dy = 0; dy < P; ++dy)
#pragma unroll
          for (int dx = 0; dx < P; ++dx) {
            const int i = (ty + dy) * TW + tx + dx;
            const float a = s_a[i], bb = s_b[i];
            Sb += bb;
            Sbb += bb * bb;
            Sab += a * bb;
          }
        const float vb = static_cast<float>(N) * Sbb - Sb * Sb;
        if (vb >= thr_f) {   // false for a NaN: some sample of the window was invalid
          const float num = static_cast<float>(N) * Sab - Sa * Sb;
          acc += num / sqrtf(va * vb);
          ++nv;
        }
      }
    }
    const float cost = nv > 0 ? acc / static_cast<float>(nv) : dense_nan();
    if (volume && in_image) volume[k * hw + static_cast<int64_t>(py) * w + px] = cost;
    if (want_next) {
      after = cost;
      want_next = false;
    }
    if (nv > 0 && cost > best) {   // strict: ties stay with the smallest k
      best = cost;
      best_k = k;
      best_nv = nv;
      before = prev;
      after = dense_nan();
      want_next = true;
    }
    prev = cost;
  }

  if (!in_image) return;
  float dl = 0.0f;
  if (best_k >= 0 && before == before && after == after) {
    const float den = before - 2.0f * best + after;
    if (den < 0.0f) dl = fminf(0.5f, fmaxf(-0.5f, 0.5f * (before - after) / den));
  }
  const int64_t o = static_cast<int64_t>(py) * w + px;
  index[o] = best_k;
  delta[o] = dl;
  score[o] = best_k >= 0 ? best : dense_nan();
  nvalid[o] = static_cast<uint8_t>(best_nv);
}

// One lane per (view i, pixel): X = Minv_i (d p - m_i), then every other view j in turn.
__global__ __launch_bounds__(kDenseThreads) void k_dense_consistency(
    const double *depth, int V, int h, int w, const double *P, const double *Minv,
    double rel_tol, uint8_t *count) {
  const int64_t hw = static_cast<int64_t>(h) * w;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kDenseThreads + threadIdx.x;
  if (t >= hw * V) return;
  const int i = static_cast<int>(t / hw);
  const int64_t pix = t - i * hw;
  const int y = static_cast<int>(pix / w), x = static_cast<int>(pix - static_cast<int64_t>(y) * w);
  const double d = depth[t];
  int c = 0;
  if (isfinite(d)) {
    const double *Pi = P + 12 * i, *Mi = Minv + 9 * i;
    const double r0 = d * x - Pi[3], r1 = d * y - Pi[7], r2 = d - Pi[11];
    const double X0 = Mi[0] * r0 + Mi[1] * r1 + Mi[2] * r2;
    const double X1 = Mi[3] * r0 + Mi[4] * r1 + Mi[5] * r2;
    const double X2 = Mi[6] * r0 + Mi[7] * r1 + Mi[8] * r2;
    const double wm1 = static_cast<double>(w - 1), hm1 = static_cast<double>(h - 1);
    for (int j = 0; j < V; ++j) {
      if (j == i) continue;
      const double *Pj = P + 12 * j;
      const double q0 = Pj[0] * X0 + Pj[1] * X1 + Pj[2] * X2 + Pj[3];
      const double q1 = Pj[4] * X0 + Pj[5] * X1 + Pj[6] * X2 + Pj[7];
      const double q2 = Pj[8] * X0 + Pj[9] * X1 + Pj[10] * X2 + Pj[11];
      const double u = floor(q0 / q2 + 0.5), v = floor(q1 / q2 + 0.5);
      if (u >= 0.0 && u <= wm1 && v >= 0.0 && v <= hm1) {   // false for a NaN
        const double dj = depth[j * hw + static_cast<int64_t>(v) * w + static_cast<int64_t>(u)];
        if (isfinite(dj) && fabs(dj - q2) <= rel_tol * fabs(q2)) ++c;
      }
    }
  }
  count[t] = static_cast<uint8_t>(c);
}

}  // namespace rsd

namespace {

bool all_finite(const double *v, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

template <int R>
void launch_sweep(dim3 grid, hipStream_t s, const uint8_t *ref, const uint8_t *src, int h, int w,
                  int S, const rsd::DenseWarp &W, const double *depths, int D, double thr,
                  int32_t *index, float *delta, float *score, uint8_t *nvalid, float *volume) {
  hipLaunchKernelGGL(rsd::k_dense_sweep<R>, grid, dim3(rsd::kDenseThreads), 0, s, ref, src, h, w,
                     S, W, depths, D, thr, index, delta, score, nvalid, volume);
}

}  // namespace

int rs::dense_sweep_check(int64_t h, int64_t w, int32_t S, const double *A, const double *b,
                          const double *depths, int64_t D, int32_t patch, double min_var,
                          bool with_volume) {
  if (patch < 3 || patch > RS_DENSE_MAX_PATCH || patch % 2 == 0)
    return fail(RS_EINVAL, "patch must be odd, in 3..11");
  if (S < 1 || S > RS_DENSE_MAX_SOURCES) return fail(RS_EINVAL, "1 to 8 source views");
  if (D < 1 || D > RS_DENSE_MAX_DEPTHS) return fail(RS_EINVAL, "1 to 4096 depth hypotheses");
  if (h <= patch || w <= patch || h > RS_DENSE_MAX_SIDE || w > RS_DENSE_MAX_SIDE)
    return fail(RS_EINVAL, "each image side must be above patch and at most 16384");
  if (h * w > RS_DENSE_MAX_PIXELS) return fail(RS_EINVAL, "more than 2^26 pixels");
  if (with_volume && D * h * w > RS_DENSE_MAX_VOLUME)
    return fail(RS_EINVAL, "a cost volume of more than 2^28 entries");
  if (!std::isfinite(min_var) || !(min_var > 0.0))
    return fail(RS_EINVAL, "min_var must be finite and positive");
  if (!all_finite(A, 9 * S) || !all_finite(b, 3 * S))
    return fail(RS_EINVAL, "the warps A, b must be finite");
  for (int64_t k = 0; k < D; ++k) {
    if (!std::isfinite(depths[k]) || depths[k] == 0.0)
      return fail(RS_EINVAL, "depths must be finite and nonzero");
    if ((depths[k] > 0.0) != (depths[0] > 0.0))
      return fail(RS_EINVAL, "depths must all have one sign");
  }
  return RS_OK;
}

void rs::dense_sweep_launch(hipStream_t s, const uint8_t *ref, const uint8_t *src, int64_t h,
                            int64_t w, int32_t S, const double *A, const double *b,
                            const double *depths, int64_t D, int32_t patch, double min_var,
                            int32_t *index, float *delta, float *score, uint8_t *nvalid,
                            float *volume) {
  rsd::DenseWarp W;
  std::memset(&W, 0, sizeof(W));
  std::memcpy(W.A, A, sizeof(double) * 9 * S);
  std::memcpy(W.b, b, sizeof(double) * 3 * S);
  const double n = static_cast<double>(patch) * patch;
  const double thr = min_var * n * n;
  const dim3 grid(static_cast<unsigned>((w + rsd::kDenseTX - 1) / rsd::kDenseTX),
                  static_cast<unsigned>((h + rsd::kDenseTY - 1) / rsd::kDenseTY));
#define RS_DENSE_LAUNCH(R)                                                                      \
  launch_sweep<R>(grid, s, ref, src, static_cast<int>(h), static_cast<int>(w), S, W, depths,   \
                  static_cast<int>(D), thr, index, delta, score, nvalid, volume)
  switch (patch / 2) {
    case 1: RS_DENSE_LAUNCH(1); break;
    case 2: RS_DENSE_LAUNCH(2); break;
    case 3: RS_DENSE_LAUNCH(3); break;
    case 4: RS_DENSE_LAUNCH(4); break;
    default: RS_DENSE_LAUNCH(5); break;
  }
#undef RS_DENSE_LAUNCH
}

extern "C" int rs_dense_plane_sweep(rs_ctx *c, const uint8_t *ref, int64_t h, int64_t w,
                                    const uint8_t *src, int32_t S, const double *A,
                                    const double *b, const double *depths, int64_t D,
                                    int32_t patch, double min_var, int32_t *index, float *delta,
                                    float *score, uint8_t *nvalid, float *volume) {
  if (!c || !ref || !src || !A || !b || !depths || !index || !delta || !score || !nvalid)
    return fail(RS_EINVAL, "null pointer");
  int st = rs::dense_sweep_check(h, w, S, A, b, depths, D, patch, min_var, volume != nullptr);
  if (st) return st;

  const size_t hw = static_cast<size_t>(h * w);
  // [ref | src | depths] go up, [index | delta | score | nvalid | volume] come down
  rs::Layout L;
  const auto b_ref = L.add<uint8_t>(hw), b_src = L.add<uint8_t>(hw * S);
  const auto b_depths = L.add<double>(D);
  const auto b_index = L.add<int32_t>(hw);
  const auto b_delta = L.add<float>(hw), b_score = L.add<float>(hw);
  const auto b_nvalid = L.add<uint8_t>(hw);
  const auto b_volume = L.add<float>(volume ? hw * D : 0);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_ref.dev(), ref, b_ref.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_src.dev(), src, b_src.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_depths.dev(), depths, b_depths.bytes, hipMemcpyHostToDevice, s));

  int32_t *d_index = b_index.dev();
  float *d_delta = b_delta.dev(), *d_score = b_score.dev();
  uint8_t *d_nvalid = b_nvalid.dev();
  float *d_volume = volume ? b_volume.dev() : nullptr;
  if ((st = c->dense.mark(0, s))) return st;
  rs::dense_sweep_launch(s, b_ref.dev(), b_src.dev(), h, w, S, A, b, b_depths.dev(), D, patch,
                         min_var, d_index, d_delta, d_score, d_nvalid, d_volume);
  HIP_TRY(hipGetLastError());
  if ((st = c->dense.mark(1, s))) return st;
  HIP_TRY(hipMemcpyAsync(index, d_index, b_index.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(delta, d_delta, b_delta.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(score, d_score, b_score.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(nvalid, d_nvalid, b_nvalid.bytes, hipMemcpyDeviceToHost, s));
  if (volume) HIP_TRY(hipMemcpyAsync(volume, d_volume, b_volume.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return c->dense.read(0, 0, 1);
}

extern "C" int rs_dense_consistency(rs_ctx *c, const double *depth, int32_t V, int64_t h,
                                    int64_t w, const double *P, const double *Minv,
                                    double rel_tol, uint8_t *count) {
  if (!c || !depth || !P || !Minv || !count) return fail(RS_EINVAL, "null pointer");
  if (V < 1 || V > RS_DENSE_MAX_VIEWS) return fail(RS_EINVAL, "1 to 128 views");
  if (h < 1 || w < 1 || h > RS_DENSE_MAX_SIDE || w > RS_DENSE_MAX_SIDE)
    return fail(RS_EINVAL, "each image side must be in 1..16384");
  if (h * w > RS_DENSE_MAX_PIXELS || V * h * w > RS_DENSE_MAX_VOLUME)
    return fail(RS_EINVAL, "more than 2^26 pixels per view or 2^28 in all");
  if (!std::isfinite(rel_tol) || rel_tol < 0.0)
    return fail(RS_EINVAL, "rel_tol must be finite and not negative");
  if (!all_finite(P, 12 * V) || !all_finite(Minv, 9 * V))
    return fail(RS_EINVAL, "the cameras must be finite");

  const size_t n = static_cast<size_t>(V * h * w);
  rs::Layout L;  // [depth | P | Minv] go up, [count] comes down
  const auto b_depth = L.add<double>(n), b_P = L.add<double>(12 * V), b_Minv = L.add<double>(9 * V);
  const auto b_count = L.add<uint8_t>(n);
  HIP_TRY(hipSetDevice(c->device));
  int st = L.bind(c);
  if (st) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_depth.dev(), depth, b_depth.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_P.dev(), P, b_P.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_Minv.dev(), Minv, b_Minv.bytes, hipMemcpyHostToDevice, s));
  if ((st = c->dense.mark(0, s))) return st;
  hipLaunchKernelGGL(rsd::k_dense_consistency,
                     dim3(static_cast<unsigned>((n + rsd::kDenseThreads - 1) / rsd::kDenseThreads)),
                     dim3(rsd::kDenseThreads), 0, s, b_depth.dev(), V, static_cast<int>(h),
                     static_cast<int>(w), b_P.dev(), b_Minv.dev(), rel_tol, b_count.dev());
  HIP_TRY(hipGetLastError());
  if ((st = c->dense.mark(1, s))) return st;
  HIP_TRY(hipMemcpyAsync(count, b_count.dev(), b_count.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return c->dense.read(1, 0, 1);
}

extern "C" int rs_dense_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->dense.enable(enable != 0);
  if (st) return st;
  c->dense.copy_out(ms);
  return RS_OK;
}
