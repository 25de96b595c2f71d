// The wash step on the GPU: the two steps main.py names and leaves empty (main.py:101-107 WASH1
// "Re-triangulate & Remove outliers", main.py:140-168 WASH2 "remove either 3D points or
// observation").  rs_wash_points re-triangulates every point robustly from its own track and
// marks the observations and points that do not fit; rs_triangulate_nview is the plain N-view
// triangulation it is built on.  All fp64, plain HIP.
//
// Mapping.  The host builds the CSR by point (stable counting sort, as rs_bundle_adjust) and
// sorts the points into three classes by track length m.  A team of T lanes owns one point; a
// workgroup is one wave of 64 / T teams:
//   m <= 6    T = 8    (<= 15 pairs)    8 points per wave
//   m <= 12   T = 16   (<= 66 pairs)    4 points per wave
//   m <= 128  T = 64   (<= 8128 pairs)  1 point per wave
// so a 2-view point does not hold 64 lanes for its one pair.  One launch serves all three: the
// first workgroups take the long tracks, the last the short ones.
//
// k_wash, per team:
//   stage      the track's cameras, uv and views into LDS (15 doubles per observation: 12 + 2
//              and one of padding, so that lanes on consecutive observations spread over the banks)
//   hypotheses lanes stride over the pairs a < b; a lane solves the two-view normal equations by
//              Cholesky and scores X_ab against the whole track (every lane reads the same LDS
//              record at the same time: a broadcast); it keeps its best (count, sum, ordinal)
//   selection  butterfly over the team's lanes on the total order (count, sum, ordinal): the
//              result does not depend on the shape of the reduction; X comes from the winner
//   refit x 2  every lane of the team carries the same X, lambda, cost; per linearisation each
//              lane writes the normal-equation terms of its observations to LDS and every lane
//              adds them up in track order, likewise the trial cost.  Teams that are done wait
//              at the barriers (the loop runs while any team of the wave is active)
//   verdict    err2, obs_keep per observation; point_keep, the failure flag, the hypothesis
//              count and the new X per point
// No floating-point atomics; every sum in track order: the same inputs give bitwise the same
// outputs.  One upload, one download, no host synchronisation between them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "host.h"

namespace rsd {

constexpr int kWashRec = 15;    // doubles per staged observation: camera 12, uv 2, padding 1
constexpr int kWashTerm = 11;   // V 6, g 3, e of the LM, e of the classification
constexpr int kWashMaxLin = 20;
constexpr int kWashLds = RS_WASH_MAX_TRACK * (kWashRec + kWashTerm + 1);  // doubles per workgroup

struct WashArgs {
  const double *cams, *uv;
  const int32_t *ov, *pt_off, *pt_obs;
  const int32_t *list;    // the points sorted by class: class k is list[cls_off[k] .. cls_off[k + 1])
  int cls_off[4];
  int cls_blocks[3];      // workgroups of class k
  int mode;               // 0 wash, 1 plain N-view triangulation
  double t2;
  int min_views, depth_sign;
  double *pts, *err2;
  int32_t *obs_keep, *point_keep, *point_fail, *hyp;
};

// x = N^-1 g for the symmetric N (00 01 02 11 12 22) through its Cholesky factor.  False on a
// non-positive (or NaN) pivot or a non-finite x.
__device__ __forceinline__ bool wash_chol3(const double *N, const double *g, double *x) {
  bool ok = N[0] > 0.0;
  const double l00 = sqrt(N[0]);
  const double l10 = N[1] / l00, l20 = N[2] / l00;
  const double d1 = N[3] - l10 * l10;
  ok = ok && d1 > 0.0;
  const double l11 = sqrt(d1);
  const double l21 = (N[4] - l20 * l10) / l11;
  const double d2 = N[5] - l20 * l20 - l21 * l21;
  ok = ok && d2 > 0.0;
  const double l22 = sqrt(d2);
  const double y0 = g[0] / l00;
  const double y1 = (g[1] - l10 * y0) / l11;
  const double y2 = (g[2] - l20 * y0 - l21 * y1) / l22;
  x[2] = y2 / l22;
  x[1] = (y1 - l21 * x[2]) / l11;
  x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
  return ok && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// The two equations (u c3 - c1).[X;1] = 0, (v c3 - c2).[X;1] = 0 of one staged observation
// added to the normal equations: N += A^T A, g -= A^T b, row u then row v.
__device__ __forceinline__ void wash_add_rows(const double *rec, double *N, double *g) {
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const double y = rec[12 + row];
    const double a0 = y * rec[8] - rec[4 * row], a1 = y * rec[9] - rec[4 * row + 1];
    const double a2 = y * rec[10] - rec[4 * row + 2], b = y * rec[11] - rec[4 * row + 3];
    N[0] += a0 * a0;
    N[1] += a0 * a1;
    N[2] += a0 * a2;
    N[3] += a1 * a1;
    N[4] += a1 * a2;
    N[5] += a2 * a2;
    g[0] -= a0 * b;
    g[1] -= a1 * b;
    g[2] -= a2 * b;
  }
}

// e = |uv - proj(X)|^2 of one staged observation and its depth w.
__device__ __forceinline__ double wash_err(const double *rec, const double *X, double &w) {
  const double a = rec[0] * X[0] + rec[1] * X[1] + rec[2] * X[2] + rec[3];
  const double b = rec[4] * X[0] + rec[5] * X[1] + rec[6] * X[2] + rec[7];
  w = rec[8] * X[0] + rec[9] * X[1] + rec[10] * X[2] + rec[11];
  const double ru = rec[12] - a / w, rv = rec[13] - b / w;
  return ru * ru + rv * rv;
}

// Ordered comparison: a NaN error is never an inlier.
__device__ __forceinline__ bool wash_inlier(double e, double w, double t2, int depth_sign) {
  return e <= t2 && (depth_sign == 0 || (depth_sign > 0 ? w > 0.0 : w < 0.0));
}

// Levenberg-Marquardt on X over the observations with in[i] != 0: Marquardt diagonal damping,
// lambda0 = 1e-3, Nielsen's update, at most kWashMaxLin linearisations, stop when an accepted
// step gains <= 1e-15 cost or lambda > 1e32 (the scheme of rs_bundle_adjust).  Every lane of a
// team holds the same state; `act` is uniform over the team.  All lanes of the wave call this
// together and leave it together.
template <int T>
__device__ void wash_refit(const double *rec, double *term, const int *in, int m, int l, bool act,
                           double *X) {
  if (act)
    for (int i = l; i < m; i += T)
      if (in[i]) {
        double w;
        term[kWashTerm * i + 9] = wash_err(rec + kWashRec * i, X, w);
      }
  __syncthreads();
  double cost = 0.0;
  if (act)
    for (int i = 0; i < m; ++i)
      if (in[i]) cost += term[kWashTerm * i + 9];
  cost *= 0.5;
  __syncthreads();
  double lam = 1e-3, nu = 2.0;
  double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  int it = 0;
  bool done = !act, need_lin = true;
  while (__any(!done)) {
    const bool lin = !done && need_lin;
    if (lin)
      for (int i = l; i < m; i += T)
        if (in[i]) {
          const double *c = rec + kWashRec * i;
          const double a = c[0] * X[0] + c[1] * X[1] + c[2] * X[2] + c[3];
          const double b = c[4] * X[0] + c[5] * X[1] + c[6] * X[2] + c[7];
          const double w = c[8] * X[0] + c[9] * X[1] + c[10] * X[2] + c[11];
          const double iw = 1.0 / w, iw2 = iw * iw;
          const double r0 = c[12] - a / w, r1 = c[13] - b / w;
          double j0[3], j1[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            j0[k] = -(c[k] * w - a * c[8 + k]) * iw2;
            j1[k] = -(c[4 + k] * w - b * c[8 + k]) * iw2;
          }
          double *t = term + kWashTerm * i;
          t[0] = j0[0] * j0[0] + j1[0] * j1[0];
          t[1] = j0[0] * j0[1] + j1[0] * j1[1];
          t[2] = j0[0] * j0[2] + j1[0] * j1[2];
          t[3] = j0[1] * j0[1] + j1[1] * j1[1];
          t[4] = j0[1] * j0[2] + j1[1] * j1[2];
          t[5] = j0[2] * j0[2] + j1[2] * j1[2];
#pragma unroll
          for (int k = 0; k < 3; ++k) t[6 + k] = j0[k] * r0 + j1[k] * r1;
        }
    __syncthreads();
    if (lin) {
#pragma unroll
      for (int k = 0; k < 6; ++k) V[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = 0.0;
      for (int i = 0; i < m; ++i)
        if (in[i]) {
          const double *t = term + kWashTerm * i;
#pragma unroll
          for (int k = 0; k < 6; ++k) V[k] += t[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) g[k] += t[6 + k];
        }
      ++it;
      need_lin = false;
    }
    double dx[3] = {0.0, 0.0, 0.0}, Xn[3];
    bool ok = false;
    if (!done) {
      const double Vd[6] = {V[0] + lam * V[0], V[1], V[2], V[3] + lam * V[3], V[4],
                            V[5] + lam * V[5]};
      const double mg[3] = {-g[0], -g[1], -g[2]};
      ok = wash_chol3(Vd, mg, dx);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) Xn[k] = X[k] + dx[k];
    if (!done && ok)
      for (int i = l; i < m; i += T)
        if (in[i]) {
          double w;
          term[kWashTerm * i + 9] = wash_err(rec + kWashRec * i, Xn, w);
        }
    __syncthreads();
    if (!done) {
      double cost_n = 0.0;
      if (ok)
        for (int i = 0; i < m; ++i)
          if (in[i]) cost_n += term[kWashTerm * i + 9];
      cost_n *= 0.5;
      const double pred = 0.5 * ((lam * dx[0] * V[0] * dx[0] - dx[0] * g[0]) +
                                 (lam * dx[1] * V[3] * dx[1] - dx[1] * g[1]) +
                                 (lam * dx[2] * V[5] * dx[2] - dx[2] * g[2]));
      if (ok && isfinite(cost_n) && cost_n < cost && pred > 0.0) {
        const double rho = (cost - cost_n) / pred;
        const bool small = (cost - cost_n) <= 1e-15 * cost;
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = Xn[k];
        cost = cost_n;
        const double t = 2.0 * rho - 1.0;
        lam *= fmax(1.0 / 3.0, 1.0 - t * t * t);
        nu = 2.0;
        if (small || it >= kWashMaxLin)
          done = true;
        else
          need_lin = true;
      } else {
        lam *= nu;
        nu *= 2.0;
        if (lam > 1e32) done = true;
      }
    }
    __syncthreads();
  }
}

// e of every observation of the track at X into term slot 10 and the inlier flags into in[];
// returns the number of inliers (the same in every lane of the team).
template <int T>
__device__ int wash_classify(const double *rec, double *term, int *in, int m, int l,
                             const double *X, double t2, int depth_sign) {
  __syncthreads();
  for (int i = l; i < m; i += T) {
    double w;
    const double e = wash_err(rec + kWashRec * i, X, w);
    term[kWashTerm * i + 10] = e;
    in[i] = wash_inlier(e, w, t2, depth_sign) ? 1 : 0;
  }
  __syncthreads();
  int cnt = 0;
  for (int i = 0; i < m; ++i) cnt += in[i];
  return cnt;
}

// One workgroup (one wave) of a class: 64 / T teams of T lanes, a point with a track of at most
// MAXM observations per team.  `list` / `count` are the class's points, `block` the workgroup's
// index within the class, `lds` the workgroup's kWashLds doubles.
template <int T, int MAXM>
__device__ void wash_wave(const WashArgs &A, const int32_t *list, int count, int block,
                          double *lds) {
  constexpr int kTeams = 64 / T;
  static_assert(kTeams * MAXM * (kWashRec + kWashTerm + 1) <= kWashLds, "LDS of a class");
  const int team = threadIdx.x / T, l = threadIdx.x % T;
  const int slot = block * kTeams + team;
  const bool has = slot < count;
  const int j = has ? list[slot] : 0;
  const int lo = has ? A.pt_off[j] : 0;
  int m = has ? A.pt_off[j + 1] - lo : 0;
  if (m > MAXM) m = 0;  // the host sorts every point into a class that holds its track
  double *rec = lds + team * MAXM * kWashRec;
  double *term = lds + kTeams * MAXM * kWashRec + team * MAXM * kWashTerm;
  int *view = reinterpret_cast<int *>(lds + kTeams * MAXM * (kWashRec + kWashTerm)) + team * MAXM;
  int *in = view + kTeams * MAXM;

  for (int i = l; i < m; i += T) {
    const int64_t o = A.pt_obs[lo + i];
    const int v = A.ov[o];
    view[i] = v;
    double *r = rec + kWashRec * i;
#pragma unroll
    for (int k = 0; k < 12; ++k) r[k] = A.cams[12 * static_cast<int64_t>(v) + k];
    r[12] = A.uv[2 * o];
    r[13] = A.uv[2 * o + 1];
    in[i] = 1;
  }
  __syncthreads();

  double X[3] = {0.0, 0.0, 0.0};
  bool fail = !has || m < 2;
  int nvalid = 0, n_in = m;
  if (A.mode == 0) {
    // ---- hypotheses: pair ordinal p (a-major, b-minor) on lane p % T
    int bc = 0, bo = 0x7fffffff;
    double bs = 0.0, bX[3] = {0.0, 0.0, 0.0};
    const int npairs = m * (m - 1) / 2;
    int a = 0, b = 1 + l;
    for (int p = l; p < npairs; p += T) {
      while (b >= m) {
        b -= m;
        ++a;
        b += a + 1;
      }
      if (view[a] != view[b]) {
        double N[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, Y[3];
        wash_add_rows(rec + kWashRec * a, N, g);
        wash_add_rows(rec + kWashRec * b, N, g);
        if (wash_chol3(N, g, Y)) {
          ++nvalid;
          int cnt = 0;
          double sum = 0.0;
          for (int i = 0; i < m; ++i) {
            double w;
            const double e = wash_err(rec + kWashRec * i, Y, w);
            if (wash_inlier(e, w, A.t2, A.depth_sign)) {
              ++cnt;
              sum += e;
            }
          }
          if (cnt > bc || (cnt == bc && sum < bs)) {  // ordinals ascend on a lane
            bc = cnt;
            bs = sum;
            bo = p;
#pragma unroll
            for (int k = 0; k < 3; ++k) bX[k] = Y[k];
          }
        }
      }
      b += T;
    }
    // ---- selection: larger count, then smaller sum, then smaller ordinal
#pragma unroll
    for (int off = T / 2; off > 0; off >>= 1) {
      const int oc = __shfl_xor(bc, off), oo = __shfl_xor(bo, off);
      const double os = __shfl_xor(bs, off);
      if (oc > bc || (oc == bc && (os < bs || (os == bs && oo < bo)))) {
        bc = oc;
        bs = os;
        bo = oo;
      }
      nvalid += __shfl_xor(nvalid, off);
    }
    const int src = team * T + (bc >= 2 ? bo % T : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = __shfl(bX[k], src);
    if (bc < 2) fail = true;
    // ---- refit twice over the current inlier set
    n_in = wash_classify<T>(rec, term, in, m, l, X, A.t2, A.depth_sign);
    for (int pass = 0; pass < 2; ++pass) {
      if (n_in < 2) fail = true;
      wash_refit<T>(rec, term, in, m, l, !fail, X);
      n_in = wash_classify<T>(rec, term, in, m, l, X, A.t2, A.depth_sign);
    }
  } else {
    // ---- the linear solution of all 2m equations, then one refit over the whole track
    double N[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    for (int i = 0; i < m; ++i) wash_add_rows(rec + kWashRec * i, N, g);
    if (!wash_chol3(N, g, X)) fail = true;
    wash_refit<T>(rec, term, in, m, l, !fail, X);
  }

  // ---- verdict
  const bool finite = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
  const bool kept = !fail && finite && (A.mode != 0 || n_in >= A.min_views);
  if (!has) return;
  if (A.mode == 0)
    for (int i = l; i < m; i += T) {
      const int64_t o = A.pt_obs[lo + i];
      A.err2[o] = fail ? __longlong_as_double(0x7ff8000000000000LL) : term[kWashTerm * i + 10];
      A.obs_keep[o] = kept && in[i] ? 1 : 0;
    }
  if (l == 0) {
    A.point_keep[j] = kept ? 1 : 0;
    A.point_fail[j] = fail ? 1 : 0;
    A.hyp[j] = nvalid;
    if (kept) {
#pragma unroll
      for (int k = 0; k < 3; ++k) A.pts[3 * static_cast<int64_t>(j) + k] = X[k];
    }
  }
}

// The long tracks first: their workgroups take the longest.
__global__ __launch_bounds__(64) void k_wash(WashArgs A) {
  __shared__ double lds[kWashLds];
  int b = blockIdx.x;
  if (b < A.cls_blocks[2]) {
    wash_wave<64, RS_WASH_MAX_TRACK>(A, A.list + A.cls_off[2], A.cls_off[3] - A.cls_off[2], b, lds);
    return;
  }
  b -= A.cls_blocks[2];
  if (b < A.cls_blocks[1]) {
    wash_wave<16, 12>(A, A.list + A.cls_off[1], A.cls_off[2] - A.cls_off[1], b, lds);
    return;
  }
  b -= A.cls_blocks[1];
  wash_wave<8, 6>(A, A.list, A.cls_off[1], b, lds);
}

}  // namespace rsd

namespace {

constexpr int kClasses = 3;
constexpr int kClassMax[kClasses] = {6, 12, RS_WASH_MAX_TRACK};  // MAXM of k_wash's three branches
constexpr int kClassTeams[kClasses] = {8, 4, 1};                 // their 64 / T

// Both entry points: the CSR by point, the classes, one upload, one launch, one download.
// point_keep is per point (nP); err2, obs_keep and info are filled in mode 0 only.
int wash_run(rs_ctx *c, int mode, const double *cams, int64_t nC, double *pts, int64_t nP,
             const int32_t *obs_view, const int32_t *obs_point, const double *uv, int64_t n,
             double thresh, int32_t min_views, int32_t depth_sign, int32_t *obs_keep,
             int32_t *point_keep, double *err2, rs_wash_info *info) {
  if (nC < 1 || n < 1) return fail(RS_EINVAL, "the wash needs at least one camera and one observation");
  if (n > (1 << 24)) return fail(RS_EINVAL, "bad sizes");
  int st = rs::ba_check(nC, nP, obs_view, obs_point, n);
  if (st) return st;

  std::vector<int32_t> pt_off(nP + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++pt_off[obs_point[i] + 1];
  int cls_count[kClasses] = {0, 0, 0};
  std::vector<int8_t> cls(nP);
  for (int64_t p = 0; p < nP; ++p) {
    const int m = pt_off[p + 1];
    if (m > RS_WASH_MAX_TRACK) return fail(RS_EINVAL, "a track longer than RS_WASH_MAX_TRACK");
    int k = 0;
    while (m > kClassMax[k]) ++k;
    cls[p] = static_cast<int8_t>(k);
    ++cls_count[k];
    pt_off[p + 1] += pt_off[p];
  }
  int cls_off[kClasses + 1] = {0, 0, 0, 0};
  for (int k = 0; k < kClasses; ++k) cls_off[k + 1] = cls_off[k] + cls_count[k];

  // one buffer: [cams | uv | ov | pt_off | pt_obs | list | pts] go up, [pts | err2 | obs_keep |
  // point_keep | point_fail | hyp] come down
  rs::Layout L;
  const auto b_cams = L.add<double>(12 * nC), b_uv = L.add<double>(2 * n);
  const auto b_ov = L.add<int32_t>(n), b_pt_off = L.add<int32_t>(nP + 1);
  const auto b_pt_obs = L.add<int32_t>(n), b_list = L.add<int32_t>(nP);
  const auto b_pts = L.add<double>(3 * nP), b_err2 = L.add<double>(n);
  const auto b_obs_keep = L.add<int32_t>(n), b_point_keep = L.add<int32_t>(nP);
  const auto b_point_fail = L.add<int32_t>(nP), b_hyp = L.add<int32_t>(nP);
  HIP_TRY(hipSetDevice(c->device));
  st = L.bind(c, 256, L.total() + 256);
  if (st) return st;
  std::memcpy(b_cams.host(), cams, b_cams.bytes);
  std::memcpy(b_uv.host(), uv, b_uv.bytes);
  std::memcpy(b_ov.host(), obs_view, b_ov.bytes);
  std::memcpy(b_pt_off.host(), pt_off.data(), b_pt_off.bytes);
  {
    int32_t *pt_obs = b_pt_obs.host(), *list = b_list.host();
    std::vector<int32_t> w(pt_off.begin(), pt_off.end() - 1);
    for (int64_t i = 0; i < n; ++i) pt_obs[w[obs_point[i]]++] = static_cast<int32_t>(i);
    int fill[kClasses] = {cls_off[0], cls_off[1], cls_off[2]};
    for (int64_t p = 0; p < nP; ++p) list[fill[cls[p]]++] = static_cast<int32_t>(p);
  }
  std::memcpy(b_pts.host(), pts, b_pts.bytes);

  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(L.dev(), L.host(), L.upto(b_err2), hipMemcpyHostToDevice, s));
  rsd::WashArgs A;
  A.cams = b_cams.dev();
  A.uv = b_uv.dev();
  A.ov = b_ov.dev();
  A.pt_off = b_pt_off.dev();
  A.pt_obs = b_pt_obs.dev();
  A.mode = mode;
  A.t2 = thresh * thresh;
  A.min_views = min_views;
  A.depth_sign = depth_sign;
  A.pts = b_pts.dev();
  A.err2 = b_err2.dev();
  A.obs_keep = b_obs_keep.dev();
  A.point_keep = b_point_keep.dev();
  A.point_fail = b_point_fail.dev();
  A.hyp = b_hyp.dev();
  A.list = b_list.dev();
  unsigned grid = 0;
  for (int k = 0; k < kClasses; ++k) {
    A.cls_off[k] = cls_off[k];
    A.cls_blocks[k] = (cls_count[k] + kClassTeams[k] - 1) / kClassTeams[k];
    grid += static_cast<unsigned>(A.cls_blocks[k]);
  }
  A.cls_off[kClasses] = cls_off[kClasses];
  if (grid > 0) hipLaunchKernelGGL(rsd::k_wash, dim3(grid), dim3(64), 0, s, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(b_pts.host(), b_pts.dev(), L.from(b_pts), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));

  std::memcpy(pts, b_pts.host(), b_pts.bytes);
  std::memcpy(point_keep, b_point_keep.host(), b_point_keep.bytes);
  if (mode == 0) {
    std::memcpy(err2, b_err2.host(), b_err2.bytes);
    std::memcpy(obs_keep, b_obs_keep.host(), b_obs_keep.bytes);
    const int32_t *pf = b_point_fail.host(), *hy = b_hyp.host();
    rs_wash_info r = {0, 0, 0, 0, 0};
    for (int64_t p = 0; p < nP; ++p) {
      r.hypotheses += hy[p];
      r.points_failed += pf[p];
      r.points_removed += point_keep[p] ? 0 : 1;
    }
    for (int64_t i = 0; i < n; ++i) r.obs_removed += obs_keep[i] ? 0 : 1;
    *info = r;
  }
  return RS_OK;
}

}  // namespace

extern "C" int rs_triangulate_nview(rs_ctx *c, const double *cams, int64_t nC, double *pts,
                                    int64_t nP, const int32_t *obs_view,
                                    const int32_t *obs_point, const double *uv, int64_t n,
                                    int32_t *ok) {
  if (!c || !cams || !pts || !obs_view || !obs_point || !uv || !ok)
    return fail(RS_EINVAL, "null pointer");
  return wash_run(c, 1, cams, nC, pts, nP, obs_view, obs_point, uv, n, 1.0, 2, 0, nullptr, ok,
                  nullptr, nullptr);
}

extern "C" int rs_wash_points(rs_ctx *c, const double *cams, int64_t nC, double *pts, int64_t nP,
                              const int32_t *obs_view, const int32_t *obs_point, const double *uv,
                              int64_t n, double thresh, int32_t min_views, int32_t depth_sign,
                              int32_t *obs_keep, int32_t *point_keep, double *err2,
                              rs_wash_info *info) {
  if (!c || !cams || !pts || !obs_view || !obs_point || !uv || !obs_keep || !point_keep ||
      !err2 || !info)
    return fail(RS_EINVAL, "null pointer");
  if (!std::isfinite(thresh) || !(thresh > 0.0))
    return fail(RS_EINVAL, "thresh must be finite and positive");
  if (min_views < 2) return fail(RS_EINVAL, "min_views must be at least 2");
  if (depth_sign < -1 || depth_sign > 1) return fail(RS_EINVAL, "depth_sign must be -1, 0 or 1");
  return wash_run(c, 0, cams, nC, pts, nP, obs_view, obs_point, uv, n, thresh, min_views,
                  depth_sign, obs_keep, point_keep, err2, info);
}
