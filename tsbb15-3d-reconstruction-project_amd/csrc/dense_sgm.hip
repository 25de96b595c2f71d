// Semi-global aggregation of the plane-sweep volume on the GPU (rs_dense_aggregate,
// rs_dense_plane_sweep_sgm).  The definition stands in include/rsamd.h; tests/dense_sgm_ref.py
// restates it in numpy, and the result here equals it bit for bit.
//
// Layouts.  The sweep's volume v is (D, h, w).  The cost c and the sum S are kept (h, w, D), k
// innermost, so the lanes of a line read and write consecutive floats.
//
// k_sgm_cost       v (D, hw) -> c (hw, D) = 1 - v (1 for a NaN), a 32 x 32 tile through LDS.
// k_sgm_path<G, J, FIRST>
//                  one launch per direction, in direction order; the first writes S = L, the
//                  others S = S + L, so S comes out as the ordered sum without atomics.
//   * A line is held by a group of G lanes (G a power of two, 1..64) with J hypotheses per lane,
//     k = g + G j: D <= 64 takes the smallest G >= D and J = 1, so a wave carries 64 / G lines
//     (D <= 32 packs two or more); D in 65..256 takes G = 64 and J = 2..4, a whole line in one
//     wave.  m is a butterfly of DPP moves inside 16 lanes and four scalar reads across the
//     wave's rows, k +- 1 a DPP shift by one lane (and lane 63 <-> lane 0 between the J
//     registers through a scalar): no LDS, and no barrier anywhere.
//   * Every line of a launch has the same number of steps.  Horizontal directions: one line per
//     row, w steps.  All others: one line per start column x0, h steps, x = (x0 + dx i) mod w;
//     when x wraps, the predecessor is outside the image and the path restarts with L = c.  The w
//     wrapped lines visit every pixel once and restart exactly where a diagonal enters the image.
//   * Hypotheses k >= D and lines past the last keep L = +inf: they drop out of every min,
//     store nothing, and load (and ignore) an entry of a live lane, so no load needs a branch.
//     Every global index is (y w + x) D + k with 0 <= x < w, 0 <= y < h, k < D: x wraps, y is
//     clamped, k is clamped.
//   * c and S of the next 16 or 8 steps (sgm_ahead) are loaded ahead of the recursion, which they
//     do not depend on, so the chain of a step is the lane moves and a handful of adds and mins.
//     The main loop is a straight run of that many steps with no branch, so that the compiler
//     never drains the loads in flight; the last, partial run is a copy with a test per step.
// k_sgm_to_volume  S (hw, D) -> (D, hw), the volume's own layout (into c's buffer, which is dead
//                  by then): the select reads it coalesced over pixels, and agg is a plain copy.
// k_sgm_select     one lane per pixel, a loop over k.
#include <hip/hip_runtime.h>

#include <cmath>

#include "host.h"

namespace rsd {

constexpr int kSgmThreads = 256;
constexpr int kSgmTile = 32;   // transposes: 32 x 32 entries per block of 32 x 8 threads
// k_sgm_path: one wave per block, so the few hundred waves of a direction spread over all CUs;
// nothing in it needs a bigger block
constexpr int kSgmPathThreads = 64;
// steps whose c and S are in flight ahead of the recursion, 2 J registers each
constexpr int sgm_ahead(int J) { return J <= 2 ? 16 : 8; }

__device__ __forceinline__ float sgm_nan() { return __int_as_float(0x7fc00000); }

// in (D, P) -> out (P, D) = 1 - in, 1 for a NaN
__global__ __launch_bounds__(kSgmThreads) void k_sgm_cost(const float *in, int D, int64_t P,
                                                          float *out) {
  __shared__ float tile[kSgmTile][kSgmTile + 1];
  const int tx = threadIdx.x & (kSgmTile - 1), ty = threadIdx.x / kSgmTile;
  const int64_t p0 = static_cast<int64_t>(blockIdx.x) * kSgmTile;
  const int k0 = static_cast<int>(blockIdx.y) * kSgmTile;
#pragma unroll
  for (int j = 0; j < kSgmTile; j += kSgmThreads / kSgmTile) {
    const int k = k0 + ty + j;
    const int64_t p = p0 + tx;
    if (k < D && p < P) {
      const float v = in[k * P + p];
      tile[ty + j][tx] = v == v ? 1.0f - v : 1.0f;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSgmTile; j += kSgmThreads / kSgmTile) {
    const int64_t p = p0 + ty + j;
    const int k = k0 + tx;
    if (k < D && p < P) out[p * D + k] = tile[tx][ty + j];
  }
}

// in (P, D) -> out (D, P)
__global__ __launch_bounds__(kSgmThreads) void k_sgm_to_volume(const float *in, int D, int64_t P,
                                                               float *out) {
  __shared__ float tile[kSgmTile][kSgmTile + 1];
  const int tx = threadIdx.x & (kSgmTile - 1), ty = threadIdx.x / kSgmTile;
  const int64_t p0 = static_cast<int64_t>(blockIdx.x) * kSgmTile;
  const int k0 = static_cast<int>(blockIdx.y) * kSgmTile;
#pragma unroll
  for (int j = 0; j < kSgmTile; j += kSgmThreads / kSgmTile) {
    const int64_t p = p0 + ty + j;
    const int k = k0 + tx;
    if (k < D && p < P) tile[ty + j][tx] = in[p * D + k];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSgmTile; j += kSgmThreads / kSgmTile) {
    const int k = k0 + ty + j;
    const int64_t p = p0 + tx;
    if (k < D && p < P) out[k * P + p] = tile[tx][ty + j];
  }
}

// Cross-lane moves without LDS.  A DPP move gives every lane the value of the lane the control
// names (a lane without a source keeps its own); all lanes are active wherever these are used.
constexpr int kDppQuadXor1 = 0xB1, kDppQuadXor2 = 0x4E;      // quad_perm [1,0,3,2], [2,3,0,1]
constexpr int kDppRowHalfMirror = 0x141, kDppRowMirror = 0x140;
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;    // lane l reads l + 1, l - 1

template <int CTRL>
__device__ __forceinline__ float sgm_dpp(float v) {
  const int i = __float_as_int(v);
  return __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
}

__device__ __forceinline__ float sgm_lane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// The min over each aligned group of G lanes, in every lane of the group: butterflies inside a
// quad, mirrors inside 8 and 16 lanes, then the four rows of the wave through scalar registers.
// min is exact and commutative, so the order is free.
template <int G>
__device__ __forceinline__ float sgm_group_min(float m, int lane) {
  if (G >= 2) m = fminf(m, sgm_dpp<kDppQuadXor1>(m));
  if (G >= 4) m = fminf(m, sgm_dpp<kDppQuadXor2>(m));
  if (G >= 8) m = fminf(m, sgm_dpp<kDppRowHalfMirror>(m));
  if (G >= 16) m = fminf(m, sgm_dpp<kDppRowMirror>(m));
  if (G >= 32) {
    const float lo = fminf(sgm_lane(m, 0), sgm_lane(m, 16));
    const float hi = fminf(sgm_lane(m, 32), sgm_lane(m, 48));
    m = G == 64 ? fminf(lo, hi) : (lane < 32 ? lo : hi);
  }
  return m;
}

// The pixel of a line at its current step.  next() moves one step along (dx, dy) and says
// whether x wrapped, which is where the path leaves the image and restarts.  y stops at the
// first and last row, so a cursor moved past the line's end still names a pixel of the image.
struct SgmCursor {
  int x, y;
  __device__ __forceinline__ bool next(int dx, int dy, int h, int w) {
    x += dx;
    y = min(max(y + dy, 0), h - 1);
    const bool over = x >= w, under = x < 0;
    x = over ? 0 : under ? w - 1 : x;
    return over || under;
  }
};

template <int G, int J, bool FIRST>
__global__ __launch_bounds__(kSgmPathThreads) void k_sgm_path(const float *__restrict__ cost,
                                                              float *S, int h, int w, int D,
                                                              int dx, int dy, float p1, float p2) {
  static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a group: a power of two within a wave");
  static_assert(J == 1 || G == 64, "several hypotheses per lane only once the wave is full");
  constexpr int kLines = kSgmPathThreads / G, kAhead = sgm_ahead(J);
  const int g = threadIdx.x % G, lane = threadIdx.x;
  const int line = static_cast<int>(blockIdx.x) * kLines + threadIdx.x / G;
  const int nlines = dy ? w : h, nsteps = dy ? h : w;
  const bool line_ok = line < nlines;

  // a dead lane (k >= D, or a line past the last) loads what the last live k of line 0 loads
  // and ignores it, so no load needs a branch and every address lies inside the volume
  bool live[J];
  int kk[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    live[j] = line_ok && g + G * j < D;
    kk[j] = min(g + G * j, D - 1);
  }

  // the line's first pixel: row `line` from its left or right end, or column `line` from the
  // top or bottom row
  SgmCursor at, ahead;
  if (dy) {
    at.x = line_ok ? line : 0;
    at.y = dy > 0 ? 0 : h - 1;
  } else {
    at.x = dx > 0 ? 0 : w - 1;
    at.y = line_ok ? line : 0;
  }
  ahead = at;

  float cb[kAhead][J], sb[kAhead][J];
  auto fetch = [&](int u) {   // c and S of the pixel `ahead` names, then one step on
    const int o = (ahead.y * w + ahead.x) * D;   // o + k < D h w <= 2^27
#pragma unroll
    for (int j = 0; j < J; ++j) {
      cb[u][j] = cost[o + kk[j]];
      if (!FIRST) sb[u][j] = S[o + kk[j]];
    }
    ahead.next(dx, dy, h, w);
  };
#pragma unroll
  for (int u = 0; u < kAhead; ++u) fetch(u);

  float L[J];
#pragma unroll
  for (int j = 0; j < J; ++j) L[j] = INFINITY;
  bool restart = true;

  // One step of the recursion on slot u, whose c and S were fetched kAhead steps ago; the slot
  // is refilled at once.  Past the line's end the refill reads the image's edge and nobody uses
  // it.  Every lane of the wave is active here, as the lane moves need.
  auto step = [&](int u) {
    float m = L[0];
#pragma unroll
    for (int j = 1; j < J; ++j) m = fminf(m, L[j]);
    m = sgm_group_min<G>(m, lane);
    const float mp2 = m + p2;
    float Ln[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      float lo = INFINITY, hi = INFINITY;
      if (G > 1) {
        // lane l reads lanes l - 1 and l + 1; the ends of a group take the neighbouring
        // register's last and first lane (J > 1 has G = 64: one group per wave) or nothing
        const float up = sgm_dpp<kDppWaveShr1>(L[j]), down = sgm_dpp<kDppWaveShl1>(L[j]);
        const float below = j > 0 ? sgm_lane(L[j > 0 ? j - 1 : 0], 63) : INFINITY;
        const float above = j < J - 1 ? sgm_lane(L[j < J - 1 ? j + 1 : 0], 0) : INFINITY;
        lo = g > 0 ? up : below;
        hi = g < G - 1 ? down : above;
      }
      const float t = fminf(fminf(L[j], mp2), fminf(lo + p1, hi + p1));
      const float c = cb[u][j];
      const float v = restart ? c : (c + t) - m;
      Ln[j] = live[j] ? v : INFINITY;
    }
    const int o = (at.y * w + at.x) * D;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      L[j] = Ln[j];
      if (live[j]) S[o + kk[j]] = FIRST ? Ln[j] : sb[u][j] + Ln[j];
    }
    restart = at.next(dx, dy, h, w);
    fetch(u);
  };

  int i0 = 0;
  for (; i0 + kAhead <= nsteps; i0 += kAhead) {
#pragma unroll
    for (int u = 0; u < kAhead; ++u) step(u);
  }
#pragma unroll
  for (int u = 0; u < kAhead; ++u)
    if (i0 + u < nsteps) step(u);   // uniform over the launch
}

// One lane per pixel; vol and agg are (D, P).
__global__ __launch_bounds__(kSgmThreads) void k_sgm_select(const float *vol, const float *agg,
                                                            int D, int64_t P, int32_t *index,
                                                            float *delta, float *score) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kSgmThreads + threadIdx.x;
  if (p >= P) return;
  float best = INFINITY;
  int bk = -1;
  for (int k = 0; k < D; ++k) {
    const float v = vol[k * P + p], s = agg[k * P + p];
    if (v == v && (bk < 0 || s < best)) {   // strict: ties stay with the smallest k
      best = s;
      bk = k;
    }
  }
  float dl = 0.0f, sc = sgm_nan();
  if (bk >= 0) {
    sc = vol[bk * P + p];
    if (bk > 0 && bk < D - 1) {
      const float vb = vol[(bk - 1) * P + p], va = vol[(bk + 1) * P + p];
      if (vb == vb && va == va) {
        const float b = agg[(bk - 1) * P + p], a = agg[(bk + 1) * P + p];
        const float den = (b - 2.0f * best) + a;   // 2 best is exact: fusing it changes nothing
        if (den > 0.0f) dl = fminf(0.5f, fmaxf(-0.5f, (0.5f * (b - a)) / den));
      }
    }
  }
  index[p] = bk;
  delta[p] = dl;
  score[p] = sc;
}

}  // namespace rsd

namespace {

const int kSgmDirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};

template <int G, int J>
void launch_path(hipStream_t s, const float *cost, float *S, int h, int w, int D, int dx, int dy,
                 int first, float p1, float p2) {
  const dim3 grid(rs::blocks(dy ? w : h, rsd::kSgmPathThreads / G)), block(rsd::kSgmPathThreads);
  if (first)
    hipLaunchKernelGGL((rsd::k_sgm_path<G, J, true>), grid, block, 0, s, cost, S, h, w, D, dx, dy,
                       p1, p2);
  else
    hipLaunchKernelGGL((rsd::k_sgm_path<G, J, false>), grid, block, 0, s, cost, S, h, w, D, dx,
                       dy, p1, p2);
}

void launch_path(hipStream_t s, const float *cost, float *S, int h, int w, int D, int dx, int dy,
                 int first, float p1, float p2) {
#define RS_SGM_PATH(G, J) launch_path<G, J>(s, cost, S, h, w, D, dx, dy, first, p1, p2)
  if (D <= 1) RS_SGM_PATH(1, 1);
  else if (D <= 2) RS_SGM_PATH(2, 1);
  else if (D <= 4) RS_SGM_PATH(4, 1);
  else if (D <= 8) RS_SGM_PATH(8, 1);
  else if (D <= 16) RS_SGM_PATH(16, 1);
  else if (D <= 32) RS_SGM_PATH(32, 1);
  else if (D <= 64) RS_SGM_PATH(64, 1);
  else if (D <= 128) RS_SGM_PATH(64, 2);
  else if (D <= 192) RS_SGM_PATH(64, 3);
  else RS_SGM_PATH(64, 4);
#undef RS_SGM_PATH
}

int sgm_check(int64_t D, int64_t h, int64_t w, float p1, float p2, int32_t paths) {
  if (D < 1 || D > RS_DENSE_SGM_MAX_DEPTHS)
    return fail(RS_EINVAL, "1 to 256 depth hypotheses for the aggregation");
  if (h < 1 || w < 1 || h > RS_DENSE_MAX_SIDE || w > RS_DENSE_MAX_SIDE)
    return fail(RS_EINVAL, "each image side must be in 1..16384");
  if (D * h * w > RS_DENSE_SGM_MAX_VOLUME)
    return fail(RS_EINVAL, "a volume of more than 2^27 entries for the aggregation");
  if (paths != 4 && paths != 8) return fail(RS_EINVAL, "paths must be 4 or 8");
  if (!std::isfinite(p1) || !std::isfinite(p2) || !(p1 >= 0.0f) || !(p1 <= p2))
    return fail(RS_EINVAL, "p1 and p2 must be finite with 0 <= p1 <= p2");
  return RS_OK;
}

// Events 1, 2, 3 of the timer around: [cost, the directions, S to (D, hw) in `cost`] and
// [select].  vol is (D, hw); cost and S are buffers of D hw floats; afterwards `cost` holds S in
// the volume's layout.
int sgm_enqueue(rs_ctx *c, hipStream_t s, const float *vol, float *cost, float *S, int D, int h,
                int w, float p1, float p2, int paths, int32_t *index, float *delta, float *score) {
  const int64_t P = static_cast<int64_t>(h) * w;
  const dim3 tiles(rs::blocks(P, rsd::kSgmTile), rs::blocks(D, rsd::kSgmTile));
  int st;
  if ((st = c->dense_sgm.mark(1, s))) return st;
  hipLaunchKernelGGL(rsd::k_sgm_cost, tiles, dim3(rsd::kSgmThreads), 0, s, vol, D, P, cost);
  for (int r = 0; r < paths; ++r)
    launch_path(s, cost, S, h, w, D, kSgmDirs[r][0], kSgmDirs[r][1], r == 0, p1, p2);
  hipLaunchKernelGGL(rsd::k_sgm_to_volume, tiles, dim3(rsd::kSgmThreads), 0, s, S, D, P, cost);
  HIP_TRY(hipGetLastError());
  if ((st = c->dense_sgm.mark(2, s))) return st;
  hipLaunchKernelGGL(rsd::k_sgm_select, dim3(rs::blocks(P, rsd::kSgmThreads)),
                     dim3(rsd::kSgmThreads), 0, s, vol, cost, D, P, index, delta, score);
  HIP_TRY(hipGetLastError());
  return c->dense_sgm.mark(3, s);
}

}  // namespace

extern "C" int rs_dense_aggregate(rs_ctx *c, const float *volume, int64_t D, int64_t h, int64_t w,
                                  float p1, float p2, int32_t paths, int32_t *index, float *delta,
                                  float *score, float *agg) {
  if (!c || !volume || !index || !delta || !score) return fail(RS_EINVAL, "null pointer");
  int st = sgm_check(D, h, w, p1, p2, paths);
  if (st) return st;

  const size_t hw = static_cast<size_t>(h * w), n = hw * static_cast<size_t>(D);
  rs::Layout L;  // [volume] goes up, [index | delta | score] and S (in cost's buffer) come down
  const auto b_vol = L.add<float>(n), b_cost = L.add<float>(n), b_S = L.add<float>(n);
  const auto b_index = L.add<int32_t>(hw);
  const auto b_delta = L.add<float>(hw), b_score = L.add<float>(hw);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_vol.dev(), volume, b_vol.bytes, hipMemcpyHostToDevice, s));
  if ((st = sgm_enqueue(c, s, b_vol.dev(), b_cost.dev(), b_S.dev(), static_cast<int>(D),
                        static_cast<int>(h), static_cast<int>(w), p1, p2, paths, b_index.dev(),
                        b_delta.dev(), b_score.dev())))
    return st;
  HIP_TRY(hipMemcpyAsync(index, b_index.dev(), b_index.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(delta, b_delta.dev(), b_delta.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(score, b_score.dev(), b_score.bytes, hipMemcpyDeviceToHost, s));
  if (agg) HIP_TRY(hipMemcpyAsync(agg, b_cost.dev(), b_cost.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->dense_sgm.read(1, 1, 2))) return st;
  return c->dense_sgm.read(2, 2, 3);
}

extern "C" int rs_dense_plane_sweep_sgm(rs_ctx *c, const uint8_t *ref, int64_t h, int64_t w,
                                        const uint8_t *src, int32_t S, const double *A,
                                        const double *b, const double *depths, int64_t D,
                                        int32_t patch, double min_var, float p1, float p2,
                                        int32_t paths, int32_t *index, float *delta, float *score,
                                        uint8_t *nvalid, float *volume, float *agg) {
  if (!c || !ref || !src || !A || !b || !depths || !index || !delta || !score || !nvalid)
    return fail(RS_EINVAL, "null pointer");
  int st = rs::dense_sweep_check(h, w, S, A, b, depths, D, patch, min_var, true);
  if (!st) st = sgm_check(D, h, w, p1, p2, paths);
  if (st) return st;

  const size_t hw = static_cast<size_t>(h * w), n = hw * static_cast<size_t>(D);
  // [ref | src | depths] go up; the sweep's own winner maps stay on the device except nvalid;
  // [index | delta | score | nvalid], the volume and S (in cost's buffer) come down
  rs::Layout L;
  const auto b_ref = L.add<uint8_t>(hw), b_src = L.add<uint8_t>(hw * S);
  const auto b_depths = L.add<double>(D);
  const auto b_wta_index = L.add<int32_t>(hw);
  const auto b_wta_delta = L.add<float>(hw), b_wta_score = L.add<float>(hw);
  const auto b_nvalid = L.add<uint8_t>(hw);
  const auto b_vol = L.add<float>(n), b_cost = L.add<float>(n), b_S = L.add<float>(n);
  const auto b_index = L.add<int32_t>(hw);
  const auto b_delta = L.add<float>(hw), b_score = L.add<float>(hw);
  HIP_TRY(hipSetDevice(c->device));
  if ((st = L.bind(c))) return st;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(b_ref.dev(), ref, b_ref.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_src.dev(), src, b_src.bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(b_depths.dev(), depths, b_depths.bytes, hipMemcpyHostToDevice, s));
  if ((st = c->dense_sgm.mark(0, s))) return st;
  rs::dense_sweep_launch(s, b_ref.dev(), b_src.dev(), h, w, S, A, b, b_depths.dev(), D, patch,
                         min_var, b_wta_index.dev(), b_wta_delta.dev(), b_wta_score.dev(),
                         b_nvalid.dev(), b_vol.dev());
  HIP_TRY(hipGetLastError());
  if ((st = sgm_enqueue(c, s, b_vol.dev(), b_cost.dev(), b_S.dev(), static_cast<int>(D),
                        static_cast<int>(h), static_cast<int>(w), p1, p2, paths, b_index.dev(),
                        b_delta.dev(), b_score.dev())))
    return st;
  HIP_TRY(hipMemcpyAsync(index, b_index.dev(), b_index.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(delta, b_delta.dev(), b_delta.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(score, b_score.dev(), b_score.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(nvalid, b_nvalid.dev(), b_nvalid.bytes, hipMemcpyDeviceToHost, s));
  if (volume) HIP_TRY(hipMemcpyAsync(volume, b_vol.dev(), b_vol.bytes, hipMemcpyDeviceToHost, s));
  if (agg) HIP_TRY(hipMemcpyAsync(agg, b_cost.dev(), b_cost.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = c->dense_sgm.read(0, 0, 1))) return st;
  if ((st = c->dense_sgm.read(1, 1, 2))) return st;
  return c->dense_sgm.read(2, 2, 3);
}

extern "C" int rs_dense_sgm_timing(rs_ctx *c, int32_t enable, double *ms) {
  if (!c || !ms) return fail(RS_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const int st = c->dense_sgm.enable(enable != 0);
  if (st) return st;
  c->dense_sgm.copy_out(ms);
  return RS_OK;
}
