// gel_kernels_exact_aero.hip -- the exact gradients of the aero path constraints (GEL_FLAG_EXACT_AERO_JAC): every entry the aero
// kinds write (angle of attack, dynamic pressure, q-alpha; lib/con_aero.py:311-471) as the analytic derivative of
// con = 1 - f / limit, formed in fp64 forward mode (gel_exact.h).  Constraint values are not formed here: the host launches the
// values-only aero launch first (launch_aero without gradient outputs), so they stay bit-identical to a handle without the flag.
//
// One lane = one (decision vector, constrained AeroNodeDev) (64-bit addressing), every kind that constrains the node served by the
// one chain.  The value chain is aero_kernel's centre (pos_part<CENTRE> without gravity, wind in ECI, aero_vair2, thrust_dir,
// aero_cos); the position directions pass through the geopotential altitude and the Bowring / longitude tangents of
// gel_exact.h (geodetic_tangent, atmosphere_tangent, wind_eci_tangent) as in exact_jac_kernel.  With the air velocity a
// (s = |a|, u = a / s), the body axis d = thrust_dir(q) (e = d / |d|), c = u.e and the density rho:
//   dq       = rho a.da + drho s^2 / 2
//   dalpha   = -(da.e_perp / s + dd.u_perp / |d|),   e_perp = (e - c u) / |e - c u|,  u_perp = (u - c e) / |u - c e|
//              (the perpendicular form: its error grows like eps / alpha; -dc / sqrt(1 - c^2) would grow like eps / alpha^2)
//   d(q alpha) = q dalpha + alpha dq
// Conventions: alpha's entries are 0 where its value is clamped to 0 (c > 1 or |a|^2 < 1e-12) and where |e - c u| = 0 exactly;
// the table-interval, atmosphere-layer, polar-axis and zero-air-speed conventions are those of gel_exact.h.  The t0 / tf columns
// are exact zeros (the air-relative velocity does not depend on the Earth angle).
//
// Outputs: the addressing of aero_body (gel_aero_body.h) for all three forms -- the dense per-kind arrays (ld = 0), the per-vector
// records' part B (ld != 0, gel_eval_aero_all's block layout) and part A (ld != 0, sm: spec-major, no t columns).
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_launch.h"
#include "gel_exact.h"

namespace gel {

constexpr int kExactAeroBlock = 256;

__global__ __launch_bounds__(kExactAeroBlock) void exact_aero_kernel(ProblemDev P, int nnodes, const AeroNodeDev* __restrict__ nodes,
                                                                      int B, const double* __restrict__ x, AeroLaunchOut O,
                                                                      long long ld, int sm) {
  extern __shared__ double lds[];
  const Tables tb = stage_tables(P, lds, true);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * nnodes) return;
  const int b = (int)(t / nnodes), ni = (int)(t - (long long)b * nnodes);
  const AeroNodeDev Nd = nodes[ni];
  const PhaseDev ph = P.phases[Nd.phase];
  const int M = P.M, N = P.N, xi = ph.xa + Nd.k;
  const double* xb = x + (size_t)b * P.nvars;
  const double r[3] = {xb[M + 3 * xi] * P.up, xb[M + 3 * xi + 1] * P.up, xb[M + 3 * xi + 2] * P.up};
  const double v[3] = {xb[4 * M + 3 * xi] * P.uv, xb[4 * M + 3 * xi + 1] * P.uv, xb[4 * M + 3 * xi + 2] * P.uv};
  const double q[4] = {xb[7 * M + 4 * xi], xb[7 * M + 4 * xi + 1], xb[7 * M + 4 * xi + 2], xb[7 * M + 4 * xi + 3]};

  // ---- values (aero_body's centre): air-relative velocity, body axis, alpha, q
  PosCentre pc;
  PosCentreTail tail;
  PosPart pp = pos_part<true, PosCentreSink, false>(r, tb, 0.0, nullptr, PosCentreSink{&pc}, &tail);
  pos_centre_tail(tail, pp.rho, pp.P, tb, pc, pp.wn, pp.we);
  const double to = xb[11 * M + 2 * N + Nd.phase], tf = xb[11 * M + 2 * N + Nd.phase + 1];
  const double tau = (Nd.k == 0) ? 0.0 : P.tau[ph.toff + Nd.k - 1];
  // PSparams.time_nodes (SectionParameters.py:77-81): node 0 is t0 itself; t in seconds here (con_aero.py:45)
  const EarthAngle ea = earth_angle(((Nd.k == 0) ? to : (tau * (tf - to) / 2 + (tf + to) / 2)) * P.ut);
  double w[3], a[3], dir[3];
  wind_eci_or_calm(r, ea, pp.sl, pp.cl, pp.inv_p, pp.wn, pp.we, w);
  const double nv2 = aero_vair2(r, v, w, a);
  thrust_dir(q, dir);
  const double ind = frsqrt(fmax(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2], 1.0e-300));
  const double cc = aero_cos(a, nv2, dir, ind);
  const double alpha = aero_acos(cc, nv2);
  const double qdyn = 0.5 * pp.rho * nv2;

  // ---- tangent pieces: position -> altitude -> density, wind; the perpendicular unit vectors of alpha
  double dsl[3], dcl[3], dalt[3], dh[3];
  geodetic_tangent(r, pp.inv_p, pc, dsl, dcl, dalt);
#pragma unroll
  for (int k = 0; k < 3; k++) dh[k] = (pc.G * pc.G) * dalt[k];
  const double Tk = pp.P / (pp.rho * tb.atm[33 + tail.k]);   // temperature at the node (rho = P / (R T))
  const AirTangent at = atmosphere_tangent(tail.h, Tk, pp.P, pp.rho, pp.inv_a, tb.atm);
  const bool in = tail.piece >= 0;
  const double s0 = in ? tb.winds[2 * tail.piece] : 0.0, s1 = in ? tb.winds[2 * tail.piece + 1] : 0.0;
  const double clon = (pp.inv_p > 0.0) ? r[0] * pp.inv_p : ea.c, slon = (pp.inv_p > 0.0) ? r[1] * pp.inv_p : ea.s;
  double dw[3][3];
  wind_eci_tangent(r, pp.inv_p, clon, slon, pc.sl, pc.cl, pp.wn, pp.we, s0, s1, dh, dsl, dcl, dw);
  const double is = frsqrt(fmax(nv2, 1.0e-300));               // 1 / |a|
  const double u[3] = {a[0] * is, a[1] * is, a[2] * is}, e[3] = {dir[0] * ind, dir[1] * ind, dir[2] * ind};
  double ep[3], upp[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { ep[c] = e[c] - cc * u[c]; upp[c] = u[c] - cc * e[c]; }
  const double ne2 = ep[0] * ep[0] + ep[1] * ep[1] + ep[2] * ep[2], nu2 = upp[0] * upp[0] + upp[1] * upp[1] + upp[2] * upp[2];
  // alpha's entries are 0 where its value is clamped (aero_acos: c > 1, |a|^2 < 1e-12) and where |e - c u| = 0 exactly
  const bool has_da = (cc <= 1.0) && (nv2 >= 1.0e-12) && ne2 > 0.0 && nu2 > 0.0;
  const double kep = has_da ? frsqrt(ne2) * is : 0.0;          // e_perp / s
  const double kup = has_da ? frsqrt(nu2) * ind : 0.0;         // u_perp / |d|
#pragma unroll
  for (int c = 0; c < 3; c++) { ep[c] *= kep; upp[c] *= kup; }

  // ---- outputs: aero_body's addressing (gel_aero_body.h AeroOut)
  double* base[3];
  int32_t rowst[3];   // distance between a block's columns (doubles)
#pragma unroll
  for (int kind = 0; kind < 3; kind++) {
    const int nq = (kind == 1) ? 0 : 4;
    const bool has = O.jac[kind] && Nd.row[kind] >= 0;
    const long long vs = ld ? ld : (long long)O.nrows[kind] * (8 + nq);
    base[kind] = has ? O.jac[kind] + (size_t)b * vs + (sm ? (size_t)Nd.row0[kind] : 0) + Nd.ko : nullptr;
    rowst[kind] = Nd.nk[kind];
  }
  const double il[3] = {frcp(Nd.limit[0]), frcp(Nd.limit[1]), frcp(Nd.limit[2])};
  bool bad = false;
  // one column of every kind that has this node: block bo (0 position, 3 velocity, 6 quaternion, -1 t) of width wd, column col;
  // sm: spec-major part A, column (1 | 4 | 7) + col of the spec's block
#define EXPUT(bo, wd, col, dal, dq_)                                                                                   \
  do {                                                                                                                 \
    const double da_ = (dal), dqv_ = (dq_);                                                                            \
    _Pragma("unroll") for (int kind = 0; kind < 3; kind++) {                                                           \
      if (!base[kind] || ((bo) == 6 && kind == 1) || (sm && (bo) < 0)) continue;                                      \
      const double df_ = (kind == 0) ? da_ : ((kind == 1) ? dqv_ : qdyn * da_ + alpha * dqv_);                        \
      const double gv_ = ((bo) < 0) ? 0.0 : -(df_ * il[kind]);                                                       \
      const int nq_ = (kind == 1) ? 0 : 4, b_ = ((bo) < 0) ? 6 + nq_ : (bo);                                           \
      const size_t o_ = sm ? (size_t)(((bo) == 0 ? 1 : ((bo) == 3 ? 4 : 7)) + (col)) * rowst[kind]                     \
                           : (size_t)b_ * O.nrows[kind] + (size_t)(wd) * Nd.row0[kind] + (size_t)(col) * rowst[kind];  \
      base[kind][o_] = gv_;                                                                                            \
      bad = bad || !(fabs(gv_) <= 1.79769313486231570815e308);                                                         \
    }                                                                                                                  \
  } while (0)

  // position columns: da = omega x (aero_vair2's sign) - dw, drho along the altitude; x_pos = r / unit_p
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double da[3] = {((k == 1) ? kOmega : 0.0) - dw[k][0], ((k == 0) ? -kOmega : 0.0) - dw[k][1], -dw[k][2]};
    const double ada = a[0] * da[0] + a[1] * da[1] + a[2] * da[2];
    const double dq = pp.rho * ada + 0.5 * (at.drho * dh[k]) * nv2;
    const double dal = -(da[0] * ep[0] + da[1] * ep[1] + da[2] * ep[2]);
    EXPUT(0, 3, k, P.up * dal, P.up * dq);
  }
  // velocity columns: da = e_k unit_v
#pragma unroll
  for (int k = 0; k < 3; k++) EXPUT(3, 3, k, P.uv * -ep[k], P.uv * (pp.rho * a[k]));
  // quaternion columns: the body axis quatrot(conj(q), e1) is a quadratic form of q (thrust_dir(); exact_jac_kernel)
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double dd[3] = {(k < 2) ? 2.0 * q[k] : -2.0 * q[k], 2.0 * q[3 - k], 2.0 * ((k & 1) ? q[k ^ 2] : -q[k ^ 2])};
    EXPUT(6, 4, k, -(dd[0] * upp[0] + dd[1] * upp[1] + dd[2] * upp[2]), 0.0);
  }
  // t0 / tf columns: exact zeros (not stored in spec-major records)
  EXPUT(-1, 2, 0, 0.0, 0.0);
  EXPUT(-1, 2, 1, 0.0, 0.0);
#undef EXPUT
  if (bad) *(volatile int32_t*)P.flag = 1;
}

hipError_t launch_aero_exact(const ProblemDev& P, int nnodes, const AeroNodeDev* nodes, int B, const double* d_x,
                             const AeroLaunchOut& out, hipStream_t s, long long ld, bool spec_major) {
  if (B <= 0 || nnodes <= 0) return hipSuccess;
  if (P.fd_recompute) return hipErrorInvalidValue;   // the default layout only (t columns as exact zeros, blocks of 11 n in part A)
  const long long threads = (long long)B * nnodes;
  const unsigned grid = (unsigned)((threads + kExactAeroBlock - 1) / kExactAeroBlock);
  const size_t lds = table_lds_bytes(P.Kw, P.Kc);
  hipLaunchKernelGGL(exact_aero_kernel, dim3(grid), dim3(kExactAeroBlock), lds, s, P, nnodes, nodes, B, d_x, out, ld,
                     (ld > 0 && spec_major) ? 1 : 0);
  return hipGetLastError();
}

}  // namespace gel
