// Bundle adjustment on the GPU: Tables.BundleAdjustment2 (tables.py:260-338) minimised by the
// Levenberg-Marquardt of oracle/tables_ref.bundle_adjust_lm -- Marquardt diagonal damping,
// Nielsen update, points eliminated by a Schur complement, camera 0 fixed.  All fp64.
//
// The problem is uploaded once and stays on the device for the whole call; the host runs the LM
// loop and reads one small record (trial cost, predicted reduction, failure flag) from pinned
// host memory per trial.  Every sum is taken in a fixed order over a CSR row or by a fixed tree,
// no floating-point atomics: the same inputs give bitwise the same outputs.
//
// per linearisation
//   k_ba_linearize   lane per observation: r, the Jacobian blocks and W_i = Jc^T Jp (12x3).
//                    Jc is stored as its 6 generators (xh / w, a / w, b / w), not 2x12 dense
//   k_ba_camera      workgroup per free camera: U_c (12x12), g_c over its CSR row
//   k_ba_pointsum    lane per point: V_p (3x3 symmetric), g_p over its CSR row
// per trial (U, V, W, g are reused across rejected trials, as the oracle reuses them)
//   k_ba_point       lane per observation: (V + lam diag V)^-1 of its point, Y_i = W_i V*^-1
//   k_ba_schur       workgroup per camera block pair a <= b (free cameras):
//                    S_ab = [a == b] U*_a - sum_p Y_{a,p} W_{b,p}^T, and the right-hand side
//   k_ba_chol        one workgroup: left-looking blocked Cholesky of S, 12-wide block columns,
//                    the matrix in global memory / L2 and a tile of the panel in LDS; the
//                    right-hand side rides along as one more row (forward solve), then the
//                    backward solve.  Raises the flag on a non-positive pivot
//   k_ba_step        lane per point: dx_p by back-substitution, trial points and cameras, the
//                    point's share of the predicted reduction
//   k_ba_cost        lane per observation: squared trial residual
//   k_ba_final       one workgroup: cost and predicted reduction by fixed-order reductions,
//                    the status record into pinned host memory
//
// Rigid cameras (rs_bundle_adjust_rigid).  The same loop over 6 local coordinates per camera,
// delta = (omega, tau) with R+ = Exp(omega) R, t+ = Exp(omega) t + tau.  The camera block width
// is the template parameter D of k_ba_camera, k_ba_point, k_ba_schur, k_ba_chol, k_ba_step and
// k_ba_final: D = 12 is the code above, unchanged; D = 6 linearises with k_ba_linearize_rigid
// (3 generators a, b, 1/z per observation), runs k_ba_camera and k_ba_schur in one wave per
// block (36 + 6 workers), pads the reduced system to whole 12-wide block columns with an
// identity diagonal and a zero right-hand side, and retracts in k_ba_step.
//
// Robust losses (rs_bundle_adjust_robust).  The same loop on the re-weighted problem: with
// w_i = rho'(z_i) at the accepted state, k_ba_linearize<true> / k_ba_linearize_rigid<true> scale
// r, Jp, W (and, D = 12, the generators of Jc) by sqrt(w_i), k_ba_camera<6, true> scales the
// rigid Jc while staging it, k_ba_cost<true> writes C^2 rho(z_i), and k_ba_weights writes the
// final w_i.  Everything from k_ba_pointsum to k_ba_final is shared with the linear path, whose
// <false> instantiations are the code it had.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "host.h"

namespace rsd {

constexpr int kBaCamTile = 256;        // observations of a camera row per LDS tile (16 KiB)
constexpr int kBaSchurTile = 32;       // observation pairs per LDS tile (2 x 9 KiB)
constexpr int kBaCholThreads = 512;
constexpr int kBaCholRows = 2;         // rows of the panel a thread updates per pass
constexpr int kBaCholBatch = 12;       // columns whose L entries are in flight together
constexpr int kBaCholTile = 240;        // columns of the panel tile in LDS (x 12 rows); a multiple of 12
constexpr int kBaMaxFree = RS_BA_MAX_CAMERAS;  // ys[] of k_ba_chol: 12 * kBaMaxFree doubles
constexpr int kBaFinalThreads = 1024;

// Row `row` (0: u, 1: v) of Jc at camera entry k, from g = xh / w (4), aw = a / w, bw = b / w:
// Jc[0] = [-g, 0, g aw], Jc[1] = [0, -g, g bw].
__device__ __forceinline__ double ba_jc(const double *j6, int row, int k) {
  const int grp = k >> 2;
  const double g = j6[k & 3];
  if (grp == 2) return g * j6[4 + row];
  return grp == row ? -g : 0.0;
}

// Rigid cameras: entry f = 6 row + k of the 2 x 6 Jc = d r / d (omega, tau) at delta = 0, from
// j3 = (a, b, iz) of Xc = R X + t = (x, y, z), a = x / z, b = y / z, iz = 1 / z:
// Jc[0] = [ab, -(1 + a^2), b, -iz, 0, a iz], Jc[1] = [1 + b^2, -ab, -a, 0, -iz, b iz].
__device__ __forceinline__ double ba_jc6(const double *j3, int f) {
  const double a = j3[0], b = j3[1], iz = j3[2];
  switch (f) {
    case 0: return a * b;
    case 1: return -(1.0 + a * a);
    case 2: return b;
    case 3: return -iz;
    case 5: return a * iz;
    case 6: return 1.0 + b * b;
    case 7: return -(a * b);
    case 8: return -a;
    case 10: return -iz;
    case 11: return b * iz;
    default: return 0.0;
  }
}

// E = Exp(w) = I + A K + B K^2 of K = [w]x: A = sin t / t, B = (sin(t/2) / (t/2))^2 / 2 (no
// 1 - cos cancellation), by their series below t^2 = 1e-12.  K^2 = w w^T - t^2 I.
__device__ __forceinline__ void ba_exp_so3(const double *w, double *E) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double A, B;
  if (t2 < 1e-12) {
    A = 1.0 - t2 / 6.0;
    B = 0.5 - t2 / 24.0;
  } else {
    const double t = sqrt(t2), h = 0.5 * t, sh = sin(h) / h;
    A = sin(t) / t;
    B = 0.5 * sh * sh;
  }
  E[0] = 1.0 + B * (w[0] * w[0] - t2);
  E[1] = B * (w[0] * w[1]) - A * w[2];
  E[2] = B * (w[0] * w[2]) + A * w[1];
  E[3] = B * (w[0] * w[1]) + A * w[2];
  E[4] = 1.0 + B * (w[1] * w[1] - t2);
  E[5] = B * (w[1] * w[2]) - A * w[0];
  E[6] = B * (w[0] * w[2]) - A * w[1];
  E[7] = B * (w[1] * w[2]) + A * w[0];
  E[8] = 1.0 + B * (w[2] * w[2] - t2);
}

// Threads of a k_ba_camera / k_ba_schur workgroup: D * D + D workers, in whole waves.
constexpr int ba_block_threads(int D) { return D == 12 ? 192 : 64; }

// v of lane `lane` (wave-uniform) in every lane.
__device__ __forceinline__ double ba_bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Inverse of the damped V* = V + lam diag(V) (V symmetric as 00 01 02 11 12 22) through its
// Cholesky factor.  False on a non-positive (or NaN) pivot.
__device__ __forceinline__ bool ba_inv3(const double *V, double lam, double *Vi) {
  const double a00 = V[0] + lam * V[0], a11 = V[3] + lam * V[3], a22 = V[5] + lam * V[5];
  const double a10 = V[1], a20 = V[2], a21 = V[4];
  bool ok = a00 > 0.0;
  const double l00 = sqrt(a00);
  const double l10 = a10 / l00, l20 = a20 / l00;
  const double d1 = a11 - l10 * l10;
  ok = ok && d1 > 0.0;
  const double l11 = sqrt(d1);
  const double l21 = (a21 - l20 * l10) / l11;
  const double d2 = a22 - l20 * l20 - l21 * l21;
  ok = ok && d2 > 0.0;
  const double l22 = sqrt(d2);
  // M = L^-1 (lower), V*^-1 = M^T M
  const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
  const double m10 = -l10 * m00 * m11;
  const double m21 = -l21 * m11 * m22;
  const double m20 = -(l20 * m00 + l21 * m10) * m22;
  Vi[0] = m00 * m00 + m10 * m10 + m20 * m20;
  Vi[1] = m10 * m11 + m20 * m21;
  Vi[2] = m20 * m22;
  Vi[3] = m11 * m11 + m21 * m21;
  Vi[4] = m21 * m22;
  Vi[5] = m22 * m22;
  return ok;
}

// Robust losses (rs_bundle_adjust_robust; scipy's names and forms) of z = (ru^2 + rv^2) / C^2:
// 1 soft_l1, 2 huber, 3 cauchy.  `loss` is uniform over a launch.  A NaN z gives NaN.
__device__ __forceinline__ double ba_rho(int loss, double z) {
  if (loss == 1) return 2.0 * z / (sqrt(1.0 + z) + 1.0);
  if (loss == 2) return z <= 1.0 ? z : 2.0 * sqrt(z) - 1.0;
  return log1p(z);
}

// w = rho'(z)
__device__ __forceinline__ double ba_weight(int loss, double z) {
  if (loss == 1) return 1.0 / sqrt(1.0 + z);
  if (loss == 2) return z <= 1.0 ? 1.0 : 1.0 / sqrt(z);
  return 1.0 / (1.0 + z);
}

// ROB: the re-weighted problem of one IRLS round.  sq = sqrt(w) of the observation's residual at
// this state scales r, Jp and the 4 generators xh / w (Jc is linear in them), so W comes out as
// w Jc^T Jp and every kernel downstream runs unchanged.  ic2 = 1 / C^2.
template <bool ROB>
__global__ __launch_bounds__(256) void k_ba_linearize(
    const double *__restrict__ cams, const double *__restrict__ pts,
    const int32_t *__restrict__ ov, const int32_t *__restrict__ op,
    const double *__restrict__ uv, int n, double *__restrict__ r, double *__restrict__ jcs,
    double *__restrict__ Jp, double *__restrict__ W, int loss, double ic2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double *c = cams + 12 * ov[i];
  const double *p = pts + 3 * op[i];
  const double xh[4] = {p[0], p[1], p[2], 1.0};
  const double a = c[0] * xh[0] + c[1] * xh[1] + c[2] * xh[2] + c[3];
  const double b = c[4] * xh[0] + c[5] * xh[1] + c[6] * xh[2] + c[7];
  const double w = c[8] * xh[0] + c[9] * xh[1] + c[10] * xh[2] + c[11];
  const double iw = 1.0 / w, iw2 = iw * iw;
  const double aw = a / w, bw = b / w;
  double r0 = uv[2 * i] - aw, r1 = uv[2 * i + 1] - bw;
  double sq = 1.0;
  if constexpr (ROB) {
    sq = sqrt(ba_weight(loss, (r0 * r0 + r1 * r1) * ic2));
    r0 *= sq;
    r1 *= sq;
  }
  r[2 * i] = r0;
  r[2 * i + 1] = r1;
  double g[4], j0[3], j1[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g[k] = xh[k] / w;
    if constexpr (ROB) g[k] *= sq;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    j0[k] = -(c[k] * w - a * c[8 + k]) * iw2;
    j1[k] = -(c[4 + k] * w - b * c[8 + k]) * iw2;
    if constexpr (ROB) {
      j0[k] *= sq;
      j1[k] *= sq;
    }
  }
  double *j6 = jcs + 6 * static_cast<int64_t>(i);
#pragma unroll
  for (int k = 0; k < 4; ++k) j6[k] = g[k];
  j6[4] = aw;
  j6[5] = bw;
  double *jp = Jp + 6 * static_cast<int64_t>(i);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    jp[k] = j0[k];
    jp[3 + k] = j1[k];
  }
  // W = Jc^T Jp: rows 0-3 = -g_k Jp[0], rows 4-7 = -g_k Jp[1], rows 8-11 = g_k (aw Jp[0] + bw Jp[1])
  double *wi = W + 36 * static_cast<int64_t>(i);
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      wi[3 * k + q] = -g[k] * j0[q];
      wi[3 * (4 + k) + q] = -g[k] * j1[q];
      wi[3 * (8 + k) + q] = (g[k] * aw) * j0[q] + (g[k] * bw) * j1[q];
    }
}

// Rigid cameras: r, the 3 generators (a, b, iz), Jp = -Pi R (the arithmetic of k_ba_linearize:
// with nC == 1 both paths give the same bits) and W = Jc^T Jp (6 x 3).
// ROB: r, Jp and W are scaled as in k_ba_linearize.  Jc is not linear in (a, b, iz), so the
// generators stay as they are and sq goes to sw[i] for k_ba_camera<6, true>.
template <bool ROB>
__global__ __launch_bounds__(256) void k_ba_linearize_rigid(
    const double *__restrict__ cams, const double *__restrict__ pts,
    const int32_t *__restrict__ ov, const int32_t *__restrict__ op,
    const double *__restrict__ uv, int n, double *__restrict__ r, double *__restrict__ jcs,
    double *__restrict__ Jp, double *__restrict__ W, int loss, double ic2,
    double *__restrict__ sw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double *c = cams + 12 * ov[i];
  const double *p = pts + 3 * op[i];
  const double xh[4] = {p[0], p[1], p[2], 1.0};
  const double a = c[0] * xh[0] + c[1] * xh[1] + c[2] * xh[2] + c[3];
  const double b = c[4] * xh[0] + c[5] * xh[1] + c[6] * xh[2] + c[7];
  const double w = c[8] * xh[0] + c[9] * xh[1] + c[10] * xh[2] + c[11];
  const double iw = 1.0 / w, iw2 = iw * iw;
  const double aw = a / w, bw = b / w;
  double r0 = uv[2 * i] - aw, r1 = uv[2 * i + 1] - bw;
  double sq = 1.0;
  if constexpr (ROB) {
    sq = sqrt(ba_weight(loss, (r0 * r0 + r1 * r1) * ic2));
    r0 *= sq;
    r1 *= sq;
    sw[i] = sq;
  }
  r[2 * i] = r0;
  r[2 * i + 1] = r1;
  double j0[3], j1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    j0[k] = -(c[k] * w - a * c[8 + k]) * iw2;
    j1[k] = -(c[4 + k] * w - b * c[8 + k]) * iw2;
    if constexpr (ROB) {
      j0[k] *= sq;
      j1[k] *= sq;
    }
  }
  double *j3 = jcs + 3 * static_cast<int64_t>(i);
  j3[0] = aw;
  j3[1] = bw;
  j3[2] = iw;
  double *jp = Jp + 6 * static_cast<int64_t>(i);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    jp[k] = j0[k];
    jp[3 + k] = j1[k];
  }
  const double g[3] = {aw, bw, iw};
  double *wi = W + 18 * static_cast<int64_t>(i);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double c0 = ba_jc6(g, k), c1 = ba_jc6(g, 6 + k);
    if constexpr (ROB) {
      c0 *= sq;
      c1 *= sq;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) wi[3 * k + q] = c0 * j0[q] + c1 * j1[q];
  }
}

// U_c = sum Jc^T Jc and g_c = sum Jc^T r over the camera's observations, in CSR order.  The
// row is staged through LDS in tiles (generators and residual of each observation, gathered
// by all threads); every thread then walks the tile in order for its own entry.  D = 6 stages
// the 2 x 6 Jc itself (each entry formed once from the 3 generators) and runs in one wave.
// ROB (D = 6 only; the D = 12 generators arrive scaled): every staged Jc entry of observation i
// is multiplied by sw[i] = sqrt(w_i).
template <int D, bool ROB>
__global__ __launch_bounds__(ba_block_threads(D)) void k_ba_camera(
    const int32_t *__restrict__ cam_of_slot, const int32_t *__restrict__ cam_off,
    const int32_t *__restrict__ cam_obs, const double *__restrict__ jcs,
    const double *__restrict__ r, double *__restrict__ U, double *__restrict__ gc,
    const double *__restrict__ sw) {
  static_assert(!ROB || D == 6, "the 12-parameter generators are scaled by k_ba_linearize");
  constexpr int DD = D * D, NT = ba_block_threads(D), F = D == 12 ? 8 : 14;
  __shared__ double sj[kBaCamTile * F];
  const int slot = blockIdx.x, tid = threadIdx.x;
  const int cam = cam_of_slot[slot];
  const int lo = cam_off[slot], hi = cam_off[slot + 1];
  const int rr = tid < DD ? tid / D : tid - DD, cc = tid % D;
  double s = 0.0;
  for (int base = lo; base < hi; base += kBaCamTile) {
    const int cnt = min(kBaCamTile, hi - base);
    __syncthreads();
    for (int idx = tid; idx < cnt * F; idx += NT) {
      const int64_t i = cam_obs[base + idx / F];
      const int f = idx % F;
      if constexpr (D == 12)
        sj[idx] = f < 6 ? jcs[6 * i + f] : r[2 * i + f - 6];
      else if constexpr (ROB)
        sj[idx] = f < 12 ? ba_jc6(jcs + 3 * i, f) * sw[i] : r[2 * i + f - 12];
      else
        sj[idx] = f < 12 ? ba_jc6(jcs + 3 * i, f) : r[2 * i + f - 12];
    }
    __syncthreads();
    if (tid < DD) {
      for (int o = 0; o < cnt; ++o) {
        if constexpr (D == 12) {
          const double *j6 = sj + 8 * o;
          s += ba_jc(j6, 0, rr) * ba_jc(j6, 0, cc) + ba_jc(j6, 1, rr) * ba_jc(j6, 1, cc);
        } else {
          const double *j = sj + 14 * o;
          s += j[rr] * j[cc] + j[6 + rr] * j[6 + cc];
        }
      }
    } else if (tid < DD + D) {
      for (int o = 0; o < cnt; ++o) {
        if constexpr (D == 12) {
          const double *j6 = sj + 8 * o;
          s += ba_jc(j6, 0, rr) * j6[6] + ba_jc(j6, 1, rr) * j6[7];
        } else {
          const double *j = sj + 14 * o;
          s += j[rr] * j[12] + j[6 + rr] * j[13];
        }
      }
    }
  }
  if (tid < DD)
    U[DD * cam + tid] = s;
  else if (tid < DD + D)
    gc[D * cam + rr] = s;
}

// V_p = sum Jp^T Jp (00 01 02 11 12 22) and g_p = sum Jp^T r over the point's observations.
__global__ __launch_bounds__(256) void k_ba_pointsum(
    const int32_t *__restrict__ pt_off, const int32_t *__restrict__ pt_obs, int nP,
    const double *__restrict__ Jp, const double *__restrict__ r, double *__restrict__ V,
    double *__restrict__ gp) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nP) return;
  double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  for (int o = pt_off[p]; o < pt_off[p + 1]; ++o) {
    const int64_t i = pt_obs[o];
    const double *j = Jp + 6 * i;
    const double r0 = r[2 * i], r1 = r[2 * i + 1];
    v[0] += j[0] * j[0] + j[3] * j[3];
    v[1] += j[0] * j[1] + j[3] * j[4];
    v[2] += j[0] * j[2] + j[3] * j[5];
    v[3] += j[1] * j[1] + j[4] * j[4];
    v[4] += j[1] * j[2] + j[4] * j[5];
    v[5] += j[2] * j[2] + j[5] * j[5];
#pragma unroll
    for (int q = 0; q < 3; ++q) g[q] += j[q] * r0 + j[3 + q] * r1;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) V[6 * static_cast<int64_t>(p) + q] = v[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) gp[3 * static_cast<int64_t>(p) + q] = g[q];
}

// Y_i = W_i V*^-1 of the observation's point; the first observation of each point also keeps
// V*^-1 for k_ba_step and reports a non-positive pivot.  W_i and Y_i are D x 3.
template <int D>
__global__ __launch_bounds__(256) void k_ba_point(
    const int32_t *__restrict__ op, const int32_t *__restrict__ pt_off,
    const int32_t *__restrict__ pt_obs, int n, const double *__restrict__ V, double lam,
    const double *__restrict__ W, double *__restrict__ Y, double *__restrict__ Vinv,
    int32_t *__restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t p = op[i];
  double vi[6];
  const bool ok = ba_inv3(V + 6 * p, lam, vi);
  if (pt_obs[pt_off[p]] == i) {
#pragma unroll
    for (int q = 0; q < 6; ++q) Vinv[6 * p + q] = vi[q];
    if (!ok) flag[0] = 1;
  }
  const double *w = W + 3 * D * static_cast<int64_t>(i);
  double *y = Y + 3 * D * static_cast<int64_t>(i);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double w0 = w[3 * k], w1 = w[3 * k + 1], w2 = w[3 * k + 2];
    y[3 * k] = w0 * vi[0] + w1 * vi[1] + w2 * vi[2];
    y[3 * k + 1] = w0 * vi[1] + w1 * vi[3] + w2 * vi[4];
    y[3 * k + 2] = w0 * vi[2] + w1 * vi[4] + w2 * vi[5];
  }
}

// The reduced system, lower triangle, element (i, m), i >= m, at S[m * ld + i]; row N (ld =
// N + 1) is the right-hand side -g_c + sum_i Y_i g_p.  Block pair `blockIdx.x` in the order
// (0,0) (0,1) .. (0,nf-1) (1,1) ..; its (i, j) observation pairs ent[pair_off[.] ..] are sorted
// by point.  D = 6 runs in one wave; ld - 1 may then exceed 6 nf (the system padded to whole
// block columns of k_ba_chol): the first workgroup writes the pad, an identity diagonal and a
// zero right-hand side.
template <int D>
__global__ __launch_bounds__(ba_block_threads(D)) void k_ba_schur(
    int nf, const int64_t *__restrict__ pair_off, const int32_t *__restrict__ ent,
    const double *__restrict__ Y, const double *__restrict__ W, const double *__restrict__ U,
    const double *__restrict__ gc, const double *__restrict__ gp,
    const int32_t *__restrict__ op, const int32_t *__restrict__ cam_of_slot,
    const int32_t *__restrict__ cam_off, const int32_t *__restrict__ cam_obs, double lam,
    double *__restrict__ S, int ld) {
  int a = 0, rest = blockIdx.x;
  while (rest >= nf - a) {
    rest -= nf - a;
    ++a;
  }
  const int b = a + rest, tid = threadIdx.x;
  const int N = ld - 1;
  constexpr int DD = D * D, D3 = 3 * D, NT = ba_block_threads(D);
  __shared__ double sy[kBaSchurTile * D3], sw[kBaSchurTile * D3];
  const int rr = tid / D, cc = tid % D;
  if constexpr (D != 12) {
    if (blockIdx.x == 0)
      for (int i = D * nf; i < N; ++i) {
        // row and column i of the symmetric matrix, and its right-hand side (column N)
        for (int m = tid; m <= N; m += NT) S[static_cast<int64_t>(i) * ld + m] = m == i ? 1.0 : 0.0;
        for (int m = tid; m < i; m += NT) S[static_cast<int64_t>(m) * ld + i] = 0.0;
      }
  }
  double s = 0.0;
  const int64_t lo = pair_off[blockIdx.x], hi = pair_off[blockIdx.x + 1];
  for (int64_t e0 = lo; e0 < hi; e0 += kBaSchurTile) {
    const int cnt = static_cast<int>(hi - e0 < kBaSchurTile ? hi - e0 : kBaSchurTile);
    __syncthreads();
    for (int idx = tid; idx < cnt * D3; idx += NT) {
      const int64_t e = e0 + idx / D3;
      const int f = idx % D3;
      sy[idx] = Y[D3 * static_cast<int64_t>(ent[2 * e]) + f];
      sw[idx] = W[D3 * static_cast<int64_t>(ent[2 * e + 1]) + f];
    }
    __syncthreads();
    if (tid < DD) {
      for (int e = 0; e < cnt; ++e) {
        const double *y = sy + D3 * e + 3 * rr;
        const double *w = sw + D3 * e + 3 * cc;
        s += y[0] * w[0] + y[1] * w[1] + y[2] * w[2];
      }
    }
  }
  if (tid < DD) {
    double u = 0.0;
    if (a == b) {
      u = U[DD * cam_of_slot[a] + tid];
      if (rr == cc) u += lam * u;
    }
    // element (D a + rr, D b + cc) = element (D b + cc, D a + rr) of the lower triangle
    S[static_cast<int64_t>(D * a + rr) * ld + D * b + cc] = u - s;
  }
  if (a != b) return;
  // right-hand side of block row a: the camera's row staged the same way (Y_i, g_p of its point)
  const int k = tid - DD;
  double t = tid >= DD && tid < DD + D ? -gc[D * cam_of_slot[a] + k] : 0.0;
  for (int o0 = cam_off[a]; o0 < cam_off[a + 1]; o0 += kBaSchurTile) {
    const int cnt = min(kBaSchurTile, cam_off[a + 1] - o0);
    __syncthreads();
    for (int idx = tid; idx < cnt * D3; idx += NT)
      sy[idx] = Y[D3 * static_cast<int64_t>(cam_obs[o0 + idx / D3]) + idx % D3];
    for (int idx = tid; idx < cnt * 3; idx += NT)
      sw[idx] = gp[3 * static_cast<int64_t>(op[cam_obs[o0 + idx / 3]]) + idx % 3];
    __syncthreads();
    if (tid >= DD && tid < DD + D) {
      for (int o = 0; o < cnt; ++o) {
        const double *y = sy + D3 * o + 3 * k;
        const double *g = sw + 3 * o;
        t += y[0] * g[0] + y[1] * g[1] + y[2] * g[2];
      }
    }
  }
  if (tid >= DD && tid < DD + D) S[static_cast<int64_t>(D * a + k) * ld + N] = t;
}

// Cholesky of S (N = 12 nf) and both triangular solves in one workgroup.  Left-looking by 12-wide
// block columns: for block column k every row i >= 12k gets A[i, 12k..] -= L[i, :12k] L[12k.., :12k]^T
// with the 12 x 12k factor rows in an LDS tile and kBaCholRows rows of the panel per thread, the
// L entries of kBaCholBatch columns requested together (DESIGN.md section 10 has the measured
// alternatives); then the diagonal block is
// factorised in the first wave's registers and the rows below are solved against it.  The right-hand
// side is row N of the matrix, so the factorisation leaves y = L^-1 rhs there.  dc (nC, 12) gets
// the camera steps (rows of cameras outside the system stay zero); on a non-positive pivot it
// gets zeros and the flag.
// Template: DC is the camera block width of dc, BW the block-column width (every 12 of the text
// above).  N is a multiple of BW; rows [nreal, N) are an identity pad (k_ba_schur) whose solution
// is zero and is not written anywhere.  A pad row has zeros left of its diagonal, so it changes
// no sum of a real row.
template <int DC, int BW>
__global__ __launch_bounds__(kBaCholThreads) void k_ba_chol(
    double *__restrict__ S, int N, int nreal, const int32_t *__restrict__ cam_of_slot,
    double *__restrict__ dc, int32_t *__restrict__ flag) {
  constexpr int BB = BW * BW, NB = BW == 12 ? kBaCholBatch : BW;
  static_assert(kBaCholTile % BW == 0 && kBaCholTile % NB == 0 && BW % NB == 0, "tile shapes");
  __shared__ double Ts[kBaCholTile * BW];
  __shared__ double D[BB];
  __shared__ double ys[12 * kBaMaxFree];
  __shared__ int bad;
  const int tid = threadIdx.x, ld = N + 1, R = N + 1, nb = N / BW;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int k = 0; k < nb; ++k) {
    const int c0 = BW * k;
    for (int m0 = 0; m0 < c0; m0 += kBaCholTile) {
      const int mc = min(kBaCholTile, c0 - m0);
      __syncthreads();
      for (int idx = tid; idx < mc * BW; idx += kBaCholThreads)
        Ts[idx] = S[static_cast<int64_t>(m0 + idx / BW) * ld + c0 + idx % BW];
      __syncthreads();
      for (int base = c0; base < R; base += kBaCholThreads * kBaCholRows) {
        // rows base + q * blockDim + tid, q < nq (uniform); a lane past the last row works on
        // row R - 1 and stores nothing
        const int nq = min(kBaCholRows, (R - base + kBaCholThreads - 1) / kBaCholThreads);
        double acc[kBaCholRows][BW];
        int row[kBaCholRows];
#pragma unroll
        for (int q = 0; q < kBaCholRows; ++q) {
          row[q] = min(base + q * kBaCholThreads + tid, R - 1);
          if (q < nq) {
#pragma unroll
            for (int c = 0; c < BW; ++c) acc[q][c] = S[static_cast<int64_t>(c0 + c) * ld + row[q]];
          }
        }
        // NB columns at a time: their L entries are all requested before the first is
        // used (one memory latency per batch, not per column); mc is a multiple of BW
        for (int m = 0; m < mc; m += NB) {
          double l[NB][kBaCholRows];
#pragma unroll
          for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int q = 0; q < kBaCholRows; ++q)
              l[j][q] = q < nq ? S[static_cast<int64_t>(m0 + m + j) * ld + row[q]] : 0.0;
#pragma unroll
          for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int c = 0; c < BW; ++c) {
              const double t = Ts[BW * (m + j) + c];
#pragma unroll
              for (int q = 0; q < kBaCholRows; ++q)
                if (q < nq) acc[q][c] -= l[j][q] * t;
            }
        }
#pragma unroll
        for (int q = 0; q < kBaCholRows; ++q)
          if (q < nq && base + q * kBaCholThreads + tid < R) {
#pragma unroll
            for (int c = 0; c < BW; ++c) S[static_cast<int64_t>(c0 + c) * ld + row[q]] = acc[q][c];
          }
      }
    }
    __syncthreads();
    if (tid < BB) D[tid] = S[static_cast<int64_t>(c0 + tid % BW) * ld + c0 + tid / BW];
    __syncthreads();
    if (tid < 64) {
      // the BW x BW factor in the first wave, lane i holding row i in registers (right-looking;
      // L[c][j] travels from lane c by v_readlane).  A bad pivot poisons the rest with NaN and
      // is reported, not branched on
      double a[BW];
#pragma unroll
      for (int c = 0; c < BW; ++c) a[c] = tid < BW ? D[BW * tid + c] : 1.0;
      bool ok = true;
#pragma unroll
      for (int j = 0; j < BW; ++j) {
        const double d = ba_bcast(a[j], j);
        ok = ok && d > 0.0;
        const double root = sqrt(d), inv = 1.0 / root;
        a[j] = tid == j ? root : a[j] * inv;
#pragma unroll
        for (int c = j + 1; c < BW; ++c) a[c] -= a[j] * ba_bcast(a[j], c);
      }
      if (tid < BW) {
#pragma unroll
        for (int c = 0; c < BW; ++c)
          if (c <= tid) D[BW * tid + c] = a[c];
      }
      if (tid == 0 && !ok) bad = 1;
    }
    __syncthreads();
    if (bad) break;
    for (int i = c0 + BW + tid; i < R; i += kBaCholThreads) {
      // keep the 78 reads of D inside the loop: hoisted, they would sit in 156 VGPRs
      asm volatile("" ::: "memory");
      double x[BW];
#pragma unroll
      for (int c = 0; c < BW; ++c) {
        double s = S[static_cast<int64_t>(c0 + c) * ld + i];
#pragma unroll
        for (int t = 0; t < c; ++t) s -= x[t] * D[BW * c + t];
        x[c] = s / D[(BW + 1) * c];
      }
#pragma unroll
      for (int c = 0; c < BW; ++c) S[static_cast<int64_t>(c0 + c) * ld + i] = x[c];
    }
    if (tid < BB && tid % BW <= tid / BW)
      S[static_cast<int64_t>(c0 + tid % BW) * ld + c0 + tid / BW] = D[tid];
  }
  __syncthreads();
  if (bad) {
    for (int idx = tid; idx < nreal; idx += kBaCholThreads)
      dc[DC * cam_of_slot[idx / DC] + idx % DC] = 0.0;
    if (tid == 0) flag[0] = 1;
    return;
  }
  // backward solve L^T x = y, block rows from the last
  for (int idx = tid; idx < N; idx += kBaCholThreads)
    ys[idx] = S[static_cast<int64_t>(idx) * ld + N];
  for (int k = nb - 1; k >= 0; --k) {
    const int c0 = BW * k;
    if (tid < BB && tid % BW <= tid / BW)
      D[tid] = S[static_cast<int64_t>(c0 + tid % BW) * ld + c0 + tid / BW];
    __syncthreads();
    if (tid == 0) {
      for (int c = BW - 1; c >= 0; --c) {
        double s = ys[c0 + c];
        for (int t = c + 1; t < BW; ++t) s -= D[BW * t + c] * ys[c0 + t];
        ys[c0 + c] = s / D[(BW + 1) * c];
      }
    }
    __syncthreads();
    for (int i = tid; i < c0; i += kBaCholThreads) {
      const double *l = S + static_cast<int64_t>(i) * ld + c0;
      double s = ys[i];
#pragma unroll
      for (int c = 0; c < BW; ++c) s -= l[c] * ys[c0 + c];
      ys[i] = s;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < nreal; idx += kBaCholThreads)
    dc[DC * cam_of_slot[idx / DC] + idx % DC] = ys[idx];
}

// Lanes [0, nP): dx_p = -V*^-1 (g_p + sum_i W_i^T dc_cam(i)), the trial point, and the point's
// share lam dx^T diag(V) dx - dx^T g_p of the predicted reduction.  Lanes [0, 12 nC) also form
// the trial cameras.  A point without observations and a camera outside the system are copied.
// D = 6: lanes [0, nC) retract, one camera each: [R | t] <- Exp(omega) [R | t] + [0 | tau].
template <int D>
__global__ __launch_bounds__(256) void k_ba_step(
    const int32_t *__restrict__ pt_off, const int32_t *__restrict__ pt_obs,
    const int32_t *__restrict__ ov, int nP, int nC, const int32_t *__restrict__ slot_of_cam,
    const double *__restrict__ W, const double *__restrict__ V, const double *__restrict__ Vinv,
    const double *__restrict__ gp, const double *__restrict__ dc, double lam,
    const double *__restrict__ cams, const double *__restrict__ pts,
    double *__restrict__ cams_n, double *__restrict__ pts_n, double *__restrict__ ppred) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (D == 12) {
    if (t < 12 * nC) cams_n[t] = slot_of_cam[t / 12] >= 0 ? cams[t] + dc[t] : cams[t];
  } else {
    if (t < nC) {
      const double *c = cams + 12 * t;
      double *cn = cams_n + 12 * t;
      if (slot_of_cam[t] >= 0) {
        const double *d = dc + 6 * t;
        double E[9];
        ba_exp_so3(d, E);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double v = E[3 * i] * c[j] + E[3 * i + 1] * c[4 + j] + E[3 * i + 2] * c[8 + j];
            cn[4 * i + j] = j == 3 ? v + d[3 + i] : v;
          }
      } else {
#pragma unroll
        for (int q = 0; q < 12; ++q) cn[q] = c[q];
      }
    }
  }
  if (t >= nP) return;
  const int64_t p = t;
  const int lo = pt_off[p], hi = pt_off[p + 1];
  if (lo == hi) {
#pragma unroll
    for (int q = 0; q < 3; ++q) pts_n[3 * p + q] = pts[3 * p + q];
    ppred[p] = 0.0;
    return;
  }
  double g[3] = {gp[3 * p], gp[3 * p + 1], gp[3 * p + 2]};
  for (int o = lo; o < hi; ++o) {
    const int64_t i = pt_obs[o];
    const double *w = W + 3 * D * i;
    const double *d = dc + D * ov[i];
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int q = 0; q < 3; ++q) g[q] += w[3 * k + q] * d[k];
  }
  const double *vi = Vinv + 6 * p;
  const double dx[3] = {-(vi[0] * g[0] + vi[1] * g[1] + vi[2] * g[2]),
                        -(vi[1] * g[0] + vi[3] * g[1] + vi[4] * g[2]),
                        -(vi[2] * g[0] + vi[4] * g[1] + vi[5] * g[2])};
  const double dv[3] = {V[6 * p], V[6 * p + 3], V[6 * p + 5]};
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    pts_n[3 * p + q] = pts[3 * p + q] + dx[q];
    s += lam * dx[q] * dv[q] * dx[q] - dx[q] * gp[3 * p + q];
  }
  ppred[p] = s;
}

// ru^2 + rv^2 of observation i.
__device__ __forceinline__ double ba_sqres(const double *__restrict__ cams,
                                           const double *__restrict__ pts,
                                           const int32_t *__restrict__ ov,
                                           const int32_t *__restrict__ op,
                                           const double *__restrict__ uv, int i) {
  const double *c = cams + 12 * ov[i];
  const double *p = pts + 3 * static_cast<int64_t>(op[i]);
  const double x0 = p[0], x1 = p[1], x2 = p[2];
  const double a = c[0] * x0 + c[1] * x1 + c[2] * x2 + c[3];
  const double b = c[4] * x0 + c[5] * x1 + c[6] * x2 + c[7];
  const double w = c[8] * x0 + c[9] * x1 + c[10] * x2 + c[11];
  const double ru = uv[2 * i] - a / w, rv = uv[2 * i + 1] - b / w;
  return ru * ru + rv * rv;
}

// e_i = s_i, the squared residual; ROB: C^2 rho(s_i / C^2), so that k_ba_final's 0.5 sum e is
// the robust cost.
template <bool ROB>
__global__ __launch_bounds__(256) void k_ba_cost(
    const double *__restrict__ cams, const double *__restrict__ pts,
    const int32_t *__restrict__ ov, const int32_t *__restrict__ op,
    const double *__restrict__ uv, int n, double *__restrict__ e, int loss, double c2,
    double ic2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s = ba_sqres(cams, pts, ov, op, uv, i);
  if constexpr (ROB)
    e[i] = c2 * ba_rho(loss, s * ic2);
  else
    e[i] = s;
}

// The weights w_i = rho'(s_i / C^2) at the returned state.
__global__ __launch_bounds__(256) void k_ba_weights(
    const double *__restrict__ cams, const double *__restrict__ pts,
    const int32_t *__restrict__ ov, const int32_t *__restrict__ op,
    const double *__restrict__ uv, int n, double *__restrict__ wout, int loss, double ic2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  wout[i] = ba_weight(loss, ba_sqres(cams, pts, ov, op, uv, i) * ic2);
}

// Sum over the workgroup in a fixed order: each thread's strided partial, then a binary tree.
__device__ __forceinline__ double ba_block_sum(double v, double *sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = kBaFinalThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

// rec (pinned host memory): [0] cost = 0.5 sum e, [1] predicted reduction
// 0.5 (lam (dc^T diag(U) dc + dx^T diag(V) dx) - dc^T g_c - dx^T g_p), [2] the failure flag
// (cleared here for the next trial), [3] the trial's serial number.  nP = nC = 0: cost only.
template <int D>
__global__ __launch_bounds__(kBaFinalThreads) void k_ba_final(
    const double *__restrict__ e, int n, const double *__restrict__ ppred, int nP,
    const double *__restrict__ dc, const double *__restrict__ U, const double *__restrict__ gc,
    int nC, double lam, int32_t *__restrict__ flag, double serial, double *__restrict__ rec) {
  __shared__ double sh[kBaFinalThreads];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n; i += kBaFinalThreads) s += e[i];
  const double cost = 0.5 * ba_block_sum(s, sh);
  s = 0.0;
  for (int p = tid; p < nP; p += kBaFinalThreads) s += ppred[p];
  const double pp = ba_block_sum(s, sh);
  s = 0.0;
  for (int t = tid; t < D * nC; t += kBaFinalThreads) {
    const double d = dc[t];
    s += lam * d * U[D * D * (t / D) + (D + 1) * (t % D)] * d - d * gc[t];
  }
  const double pc = ba_block_sum(s, sh);
  if (tid == 0) {
    rec[0] = cost;
    rec[1] = 0.5 * (pp + pc);
    rec[2] = flag[0] ? 1.0 : 0.0;
    rec[3] = serial;
    flag[0] = 0;
    __threadfence_system();
  }
}

}  // namespace rsd

namespace {

enum { T_LIN, T_CAM, T_PSUM, T_POINT, T_SCHUR, T_CHOL, T_STEP, T_COST, T_SLOTS };
static_assert(T_SLOTS == RS_BA_TIMING_SLOTS, "rs_ba_timing slots");

// The context's BA timer over one batch of kernels (up to the next host wait): event k closes
// the kernel whose slot is slot[k], and collect() adds the batch to the sums per kernel.
struct BaMarks {
  rs_ctx *c;
  int used = 0;
  int slot[RS_BA_EVENTS] = {};
  int begin() {
    used = 0;
    return mark(-1);
  }
  int mark(int s) {
    if (!c->ba.on || used >= RS_BA_EVENTS) return RS_OK;
    slot[used] = s;
    return c->ba.mark(used++, c->stream);
  }
  int collect() {  // after the stream has been waited for
    for (int k = 1; k < used; ++k)
      if (int st = c->ba.add(slot[k], k - 1, k)) return st;
    used = 0;
    return RS_OK;
  }
};

using rs::blocks;

}  // namespace

extern "C" int rs_ba_timing(rs_ctx *c, int32_t enable, double *ms, int64_t *trials) {
  if (!c) return fail(RS_EINVAL, "null context");
  if (ms) c->ba.copy_out(ms);
  if (trials) *trials = c->ba_trials;
  c->ba.on = enable ? 1 : 0;  // no device call here: the events are created by the first marks
  return RS_OK;
}

namespace {

// Block-column width of the rigid (D = 6) reduced system: 12 pads 6 nf up to a multiple of 12
// with an identity diagonal, 6 factorises 6-wide block columns (DESIGN.md section 10 has the
// measurement behind the default).
#ifndef RS_BA_RIGID_BW
#define RS_BA_RIGID_BW 12
#endif

// R of a free rigid camera must be a rotation: max |R^T R - I| <= 1e-6 and det R > 0.
bool ba_is_rotation(const double *c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = c[i] * c[j] + c[4 + i] * c[4 + j] + c[8 + i] * c[8 + j] - (i == j ? 1.0 : 0.0);
      if (!(std::fabs(g) <= 1e-6)) return false;  // NaN too
    }
  const double det = c[0] * (c[5] * c[10] - c[6] * c[9]) - c[1] * (c[4] * c[10] - c[6] * c[8]) +
                     c[2] * (c[4] * c[9] - c[5] * c[8]);
  return det > 0.0;
}

// The LM loop of all entry points; D = 12: cameras as 12 free entries, D = 6: rigid.  ROB: the
// robust loss `loss` (1..3) at scale f_scale, every linearisation re-weighted from the residuals
// of the accepted state (the linear instantiation launches what it launched before the robust
// loss existed).  weights (n) may be NULL; it gets w_i at the returned state, ones without ROB.
template <int D, bool ROB>
int ba_run(rs_ctx *c, double *cams, int64_t nC, double *pts, int64_t nP, const int32_t *obs_view,
           const int32_t *obs_point, const double *uv, int64_t n, int32_t max_iter, double ftol,
           int32_t loss, double f_scale, double *weights, rs_ba_info *info) {
  constexpr int BW = D == 12 ? 12 : RS_BA_RIGID_BW, DD = D * D, D3 = 3 * D, NG = D / 2;
  constexpr int NT = rsd::ba_block_threads(D);
  static_assert(BW == 12 || BW == 6, "block-column width");
  if (!c || !cams || !pts || !obs_view || !obs_point || !uv || !info)
    return fail(RS_EINVAL, "null pointer");
  if (n <= 0) return fail(RS_EINVAL, "bundle adjustment needs at least one observation");
  if (nC > RS_BA_MAX_CAMERAS) return fail(RS_EINVAL, "more cameras than RS_BA_MAX_CAMERAS");
  if (n > (1 << 24) || max_iter < 0) return fail(RS_EINVAL, "bad sizes");
  int st = rs::ba_check(nC, nP, obs_view, obs_point, n);
  if (st) return st;

  // ---- host, once: CSR by point and by camera (counting sort, stable), the free cameras
  // (1.. with an observation) and the observation pairs of every camera block pair
  std::vector<int32_t> pt_off(nP + 1, 0), pt_obs(n), cnt_cam(nC, 0), slot_of_cam(nC, -1);
  for (int64_t i = 0; i < n; ++i) {
    ++pt_off[obs_point[i] + 1];
    ++cnt_cam[obs_view[i]];
  }
  for (int64_t p = 0; p < nP; ++p) pt_off[p + 1] += pt_off[p];
  {
    std::vector<int32_t> at(pt_off.begin(), pt_off.end() - 1);
    for (int64_t i = 0; i < n; ++i) pt_obs[at[obs_point[i]]++] = static_cast<int32_t>(i);
  }
  std::vector<int32_t> cam_of_slot;
  for (int64_t k = 1; k < nC; ++k)
    if (cnt_cam[k] > 0) {
      slot_of_cam[k] = static_cast<int32_t>(cam_of_slot.size());
      cam_of_slot.push_back(static_cast<int32_t>(k));
    }
  const int nf = static_cast<int>(cam_of_slot.size());
  if constexpr (D == 6) {
    for (int32_t k : cam_of_slot)
      if (!ba_is_rotation(cams + 12 * k)) {
        rs::set_error("camera %d is not a rigid pose: max |R^T R - I| > 1e-6 or det R <= 0", k);
        return RS_EINVAL;
      }
  }
  // N: the reduced system with its pad to whole block columns
  const int nreal = D * nf, N = (nreal + BW - 1) / BW * BW, ld = N + 1;
  std::vector<int32_t> cam_off(nf + 1, 0), cam_obs;
  for (int s = 0; s < nf; ++s) cam_off[s + 1] = cam_off[s] + cnt_cam[cam_of_slot[s]];
  cam_obs.resize(cam_off[nf] > 0 ? cam_off[nf] : 1);
  {
    std::vector<int32_t> at(cam_off.begin(), cam_off.end() - 1);
    for (int64_t i = 0; i < n; ++i) {
      const int s = slot_of_cam[obs_view[i]];
      if (s >= 0) cam_obs[at[s]++] = static_cast<int32_t>(i);
    }
  }
  const int64_t npair = static_cast<int64_t>(nf) * (nf + 1) / 2;
  auto pair_index = [nf](int a, int b) {
    return static_cast<int64_t>(a) * nf - static_cast<int64_t>(a) * (a - 1) / 2 + (b - a);
  };
  std::vector<int64_t> pair_off(npair + 1, 0);
  std::vector<int32_t> ent;
  if (nf > 0) {
    for (int pass = 0; pass < 2; ++pass) {
      std::vector<int64_t> at;
      if (pass == 1) {
        for (int64_t q = 0; q < npair; ++q) pair_off[q + 1] += pair_off[q];
        if (pair_off[npair] > (int64_t(1) << 27))
          return fail(RS_EINVAL, "too many co-visible observation pairs");
        ent.resize(2 * static_cast<size_t>(pair_off[npair]) + 2);
        at.assign(pair_off.begin(), pair_off.end() - 1);
      }
      for (int64_t p = 0; p < nP; ++p)
        for (int oi = pt_off[p]; oi < pt_off[p + 1]; ++oi) {
          const int i = pt_obs[oi], a = slot_of_cam[obs_view[i]];
          if (a < 0) continue;
          for (int oj = pt_off[p]; oj < pt_off[p + 1]; ++oj) {
            const int j = pt_obs[oj], b = slot_of_cam[obs_view[j]];
            if (b < a) continue;
            const int64_t q = pair_index(a, b);
            if (pass == 0) {
              ++pair_off[q + 1];
            } else {
              ent[2 * at[q]] = i;
              ent[2 * at[q] + 1] = j;
              ++at[q];
            }
          }
        }
    }
  } else {
    ent.resize(2);
  }

  // ---- device buffers, one carve of the context scratch
  HIP_TRY(hipSetDevice(c->device));
  const size_t F8 = sizeof(double), I = sizeof(int32_t);
  const int64_t pp = nP > 0 ? nP : 1;
  rs::Layout L;
  // the state and its trial copy
  const auto b_cams = L.add<double>(12 * nC), b_cams_n = L.add<double>(12 * nC);
  const auto b_pts = L.add<double>(3 * pp), b_pts_n = L.add<double>(3 * pp);
  // the observations
  const auto b_ov = L.add<int32_t>(n), b_op = L.add<int32_t>(n);
  const auto b_uv = L.add<double>(2 * n);
  // CSR by point and by free camera
  const auto b_pt_off = L.add<int32_t>(nP + 1), b_pt_obs = L.add<int32_t>(n);
  const auto b_cam_off = L.add<int32_t>(nf + 1), b_cam_obs = L.add<int32_t>(cam_obs.size());
  // camera -> slot, slot -> camera, the observation pairs of every camera block pair
  const auto b_slot = L.add<int32_t>(nC), b_cos = L.add<int32_t>(nf + 1);
  const auto b_pair_off = L.add<int64_t>(npair + 1);
  const auto b_ent = L.add<int32_t>(ent.size());
  // r, jcs, Jp, W, Y per observation
  const auto b_r = L.add<double>(2 * n), b_jcs = L.add<double>(NG * n), b_Jp = L.add<double>(6 * n);
  const auto b_W = L.add<double>(D3 * n), b_Y = L.add<double>(D3 * n);
  // U, gc, dc per camera
  const auto b_U = L.add<double>(DD * nC), b_gc = L.add<double>(D * nC), b_dc = L.add<double>(D * nC);
  // V, Vinv, gp, ppred per point
  const auto b_V = L.add<double>(6 * pp), b_Vinv = L.add<double>(6 * pp);
  const auto b_gp = L.add<double>(3 * pp), b_ppred = L.add<double>(pp);
  // e per observation, the reduced system S, the failure flag
  const auto b_e = L.add<double>(n), b_S = L.add<double>(static_cast<size_t>(ld) * ld);
  const auto b_flag = L.add<int32_t>(64);
  const auto b_sw = L.add<double>(ROB && D == 6 ? n : 0);  // robust rigid only
  st = L.bind(c, 256, 256);  // pinned: the status record alone
  if (st) return st;
  double *d_cams = b_cams.dev(), *d_cams_n = b_cams_n.dev();
  double *d_pts = b_pts.dev(), *d_pts_n = b_pts_n.dev();
  int32_t *d_ov = b_ov.dev(), *d_op = b_op.dev();
  double *d_uv = b_uv.dev();
  int32_t *d_pt_off = b_pt_off.dev(), *d_pt_obs = b_pt_obs.dev();
  int32_t *d_cam_off = b_cam_off.dev(), *d_cam_obs = b_cam_obs.dev();
  int32_t *d_slot = b_slot.dev(), *d_cos = b_cos.dev();
  int64_t *d_pair_off = b_pair_off.dev();
  int32_t *d_ent = b_ent.dev();
  double *d_r = b_r.dev(), *d_jcs = b_jcs.dev(), *d_Jp = b_Jp.dev(), *d_W = b_W.dev();
  double *d_Y = b_Y.dev(), *d_U = b_U.dev(), *d_gc = b_gc.dev(), *d_dc = b_dc.dev();
  double *d_V = b_V.dev(), *d_Vinv = b_Vinv.dev(), *d_gp = b_gp.dev(), *d_ppred = b_ppred.dev();
  double *d_e = b_e.dev(), *d_S = b_S.dev();
  int32_t *d_flag = b_flag.dev();
  double *d_sw = b_sw.dev();
  const double c2 = ROB ? f_scale * f_scale : 1.0, ic2 = 1.0 / c2;
  volatile double *rec = static_cast<volatile double *>(c->pinned);

  hipStream_t s = c->stream;
  auto up = [s](void *dst, const void *src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  };
  HIP_TRY(up(d_cams, cams, F8 * 12 * nC));
  HIP_TRY(up(d_pts, pts, F8 * 3 * nP));
  HIP_TRY(up(d_ov, obs_view, I * n));
  HIP_TRY(up(d_op, obs_point, I * n));
  HIP_TRY(up(d_uv, uv, F8 * 2 * n));
  HIP_TRY(up(d_pt_off, pt_off.data(), I * (nP + 1)));
  HIP_TRY(up(d_pt_obs, pt_obs.data(), I * n));
  HIP_TRY(up(d_cam_off, cam_off.data(), I * (nf + 1)));
  HIP_TRY(up(d_cam_obs, cam_obs.data(), I * cam_obs.size()));
  HIP_TRY(up(d_slot, slot_of_cam.data(), I * nC));
  HIP_TRY(up(d_cos, cam_of_slot.data(), I * nf));
  HIP_TRY(up(d_pair_off, pair_off.data(), sizeof(int64_t) * (npair + 1)));
  HIP_TRY(up(d_ent, ent.data(), I * ent.size()));
  // cameras outside the system keep zero U, g_c and step for the whole call
  HIP_TRY(hipMemsetAsync(d_U, 0, F8 * DD * nC, s));
  HIP_TRY(hipMemsetAsync(d_gc, 0, F8 * D * nC, s));
  HIP_TRY(hipMemsetAsync(d_dc, 0, F8 * D * nC, s));
  HIP_TRY(hipMemsetAsync(d_flag, 0, b_flag.bytes, s));

  BaMarks mk{c};
  if (c->ba.on) {
    for (double &v : c->ba.ms) v = 0.0;
    c->ba_trials = 0;
  }
  const int ni = static_cast<int>(n), nPi = static_cast<int>(nP), nCi = static_cast<int>(nC);
  double serial = 0.0;
  // the cost at (cm, pt) into the record; waits for it
  auto cost_at = [&](const double *cm, const double *pt, bool trial, double lam) -> int {
    hipLaunchKernelGGL(rsd::k_ba_cost<ROB>, dim3(blocks(n, 256)), dim3(256), 0, s, cm, pt, d_ov,
                       d_op, d_uv, ni, d_e, loss, c2, ic2);
    serial += 1.0;
    hipLaunchKernelGGL(rsd::k_ba_final<D>, dim3(1), dim3(rsd::kBaFinalThreads), 0, s, d_e, ni,
                       d_ppred, trial ? nPi : 0, d_dc, d_U, d_gc, trial ? nCi : 0, lam, d_flag,
                       serial, const_cast<double *>(rec));
    HIP_TRY(hipGetLastError());
    if (int e = mk.mark(T_COST)) return e;
    HIP_TRY(hipStreamSynchronize(s));
    if (int e = mk.collect()) return e;
    if (rec[3] != serial) return fail(RS_EDEVICE, "bundle adjustment: status record not written");
    return RS_OK;
  };

  if ((st = mk.begin())) return st;
  st = cost_at(d_cams, d_pts, false, 0.0);
  if (st) return st;
  double cost = rec[0];
  if (!std::isfinite(cost)) return fail(RS_EINVAL, "non-finite initial cost");
  const double cost0 = cost;
  double lam = 1e-3, nu = 2.0;
  int32_t it = 0, rejected = 0, status = 0;
  bool done = false;
  for (it = 1; it <= max_iter && !done; ++it) {
    if ((st = mk.begin())) return st;
    if constexpr (D == 12)
      hipLaunchKernelGGL(rsd::k_ba_linearize<ROB>, dim3(blocks(n, 256)), dim3(256), 0, s, d_cams,
                         d_pts, d_ov, d_op, d_uv, ni, d_r, d_jcs, d_Jp, d_W, loss, ic2);
    else
      hipLaunchKernelGGL(rsd::k_ba_linearize_rigid<ROB>, dim3(blocks(n, 256)), dim3(256), 0, s,
                         d_cams, d_pts, d_ov, d_op, d_uv, ni, d_r, d_jcs, d_Jp, d_W, loss, ic2,
                         d_sw);
    if ((st = mk.mark(T_LIN))) return st;
    if (nf > 0) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(rsd::k_ba_camera<D, ROB && D == 6>), dim3(nf), dim3(NT), 0,
                         s, d_cos, d_cam_off, d_cam_obs, d_jcs, d_r, d_U, d_gc, d_sw);
      if ((st = mk.mark(T_CAM))) return st;
    }
    hipLaunchKernelGGL(rsd::k_ba_pointsum, dim3(blocks(pp, 256)), dim3(256), 0, s, d_pt_off,
                       d_pt_obs, nPi, d_Jp, d_r, d_V, d_gp);
    if ((st = mk.mark(T_PSUM))) return st;
    for (;;) {
      hipLaunchKernelGGL(rsd::k_ba_point<D>, dim3(blocks(n, 256)), dim3(256), 0, s, d_op, d_pt_off,
                         d_pt_obs, ni, d_V, lam, d_W, d_Y, d_Vinv, d_flag);
      if ((st = mk.mark(T_POINT))) return st;
      if (nf > 0) {
        hipLaunchKernelGGL(rsd::k_ba_schur<D>, dim3(static_cast<unsigned>(npair)), dim3(NT), 0, s,
                           nf, d_pair_off, d_ent, d_Y, d_W, d_U, d_gc, d_gp, d_op, d_cos,
                           d_cam_off, d_cam_obs, lam, d_S, ld);
        if ((st = mk.mark(T_SCHUR))) return st;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(rsd::k_ba_chol<D, BW>), dim3(1),
                           dim3(rsd::kBaCholThreads), 0, s, d_S, N, nreal, d_cos, d_dc, d_flag);
        if ((st = mk.mark(T_CHOL))) return st;
      }
      const int64_t clanes = D == 12 ? 12 * nC : nC, lanes = nP > clanes ? nP : clanes;
      hipLaunchKernelGGL(rsd::k_ba_step<D>, dim3(blocks(lanes, 256)), dim3(256), 0, s, d_pt_off,
                         d_pt_obs, d_ov, nPi, nCi, d_slot, d_W, d_V, d_Vinv, d_gp, d_dc, lam,
                         d_cams, d_pts, d_cams_n, d_pts_n, d_ppred);
      if ((st = mk.mark(T_STEP))) return st;
      st = cost_at(d_cams_n, d_pts_n, true, lam);
      if (st) return st;
      if (c->ba.on) ++c->ba_trials;
      const double cost_n = rec[0], pred = rec[1];
      const bool failed = rec[2] != 0.0 || !std::isfinite(cost_n);
      if (!failed && cost_n < cost && pred > 0.0) {
        const double rho = (cost - cost_n) / pred;
        const bool small = (cost - cost_n) <= ftol * cost;
        std::swap(d_cams, d_cams_n);
        std::swap(d_pts, d_pts_n);
        cost = cost_n;
        const double t = 2.0 * rho - 1.0;
        lam *= std::fmax(1.0 / 3.0, 1.0 - t * t * t);
        nu = 2.0;
        if (small) {
          status = 1;
          done = true;
        }
        break;
      }
      ++rejected;
      lam *= nu;
      nu *= 2.0;
      if (lam > 1e32) {
        status = 2;
        done = true;
        break;
      }
      if ((st = mk.begin())) return st;
    }
  }
  it = done ? it - 1 : max_iter;

  if constexpr (ROB) {
    if (weights) {
      if ((st = mk.begin())) return st;
      hipLaunchKernelGGL(rsd::k_ba_weights, dim3(blocks(n, 256)), dim3(256), 0, s, d_cams, d_pts,
                         d_ov, d_op, d_uv, ni, d_e, loss, ic2);
      HIP_TRY(hipGetLastError());
      if ((st = mk.mark(T_COST))) return st;
      HIP_TRY(hipMemcpyAsync(weights, d_e, F8 * n, hipMemcpyDeviceToHost, s));
    }
  } else if (weights) {
    for (int64_t i = 0; i < n; ++i) weights[i] = 1.0;
  }
  HIP_TRY(hipMemcpyAsync(cams, d_cams, F8 * 12 * nC, hipMemcpyDeviceToHost, s));
  if (nP > 0) HIP_TRY(hipMemcpyAsync(pts, d_pts, F8 * 3 * nP, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((st = mk.collect())) return st;
  info->cost_init = cost0;
  info->cost = cost;
  info->lambda = lam;
  info->iterations = it;
  info->rejected = rejected;
  info->status = status;
  info->reserved = 0;
  return RS_OK;
}

}  // namespace

extern "C" int rs_bundle_adjust(rs_ctx *c, double *cams, int64_t nC, double *pts, int64_t nP,
                                const int32_t *obs_view, const int32_t *obs_point,
                                const double *uv, int64_t n, int32_t max_iter, double ftol,
                                rs_ba_info *info) {
  return ba_run<12, false>(c, cams, nC, pts, nP, obs_view, obs_point, uv, n, max_iter, ftol, 0,
                           1.0, nullptr, info);
}

extern "C" int rs_bundle_adjust_rigid(rs_ctx *c, double *cams, int64_t nC, double *pts,
                                      int64_t nP, const int32_t *obs_view,
                                      const int32_t *obs_point, const double *uv, int64_t n,
                                      int32_t max_iter, double ftol, rs_ba_info *info) {
  return ba_run<6, false>(c, cams, nC, pts, nP, obs_view, obs_point, uv, n, max_iter, ftol, 0,
                          1.0, nullptr, info);
}

extern "C" int rs_bundle_adjust_robust(rs_ctx *c, double *cams, int64_t nC, double *pts,
                                       int64_t nP, const int32_t *obs_view,
                                       const int32_t *obs_point, const double *uv, int64_t n,
                                       int32_t max_iter, double ftol, int32_t rigid, int32_t loss,
                                       double f_scale, double *weights, rs_ba_info *info) {
  if (loss < 0 || loss > 3) return fail(RS_EINVAL, "loss must be 0 (linear) .. 3 (cauchy)");
  if (!std::isfinite(f_scale) || f_scale <= 0.0)
    return fail(RS_EINVAL, "f_scale must be finite and > 0");
  if (loss == 0) {
    if (rigid)
      return ba_run<6, false>(c, cams, nC, pts, nP, obs_view, obs_point, uv, n, max_iter, ftol, 0,
                              1.0, weights, info);
    return ba_run<12, false>(c, cams, nC, pts, nP, obs_view, obs_point, uv, n, max_iter, ftol, 0,
                             1.0, weights, info);
  }
  if (rigid)
    return ba_run<6, true>(c, cams, nC, pts, nP, obs_view, obs_point, uv, n, max_iter, ftol, loss,
                           f_scale, weights, info);
  return ba_run<12, true>(c, cams, nC, pts, nP, obs_view, obs_point, uv, n, max_iter, ftol, loss,
                          f_scale, weights, info);
}
