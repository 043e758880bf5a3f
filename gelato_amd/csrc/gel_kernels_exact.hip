// gel_kernels_exact.hip -- the exact Jacobian of the defect groups (GEL_FLAG_EXACT_DEFECT_JAC): every x-dependent compact slot
// the fused kernel writes for an evaluation with derivatives, as the analytic derivative of the residual, formed in fp64 forward
// mode (gel_exact.h).  Residuals are not formed here: the host launches the fused kernel's residual-only form first.
//
// One lane = one collocation node of one decision vector (grid B x N, node-major inside a vector); no D.X product (the D
// entries of the pattern are constants, D[j][j+1] on the velocity diagonal is read from Dt).  Position and velocity columns
// are three tangent directions each, carried side by side (a dual<3> written out): the chain position -> altitude ->
// atmosphere / wind collapses to ONE scalar (geopotential altitude), so the three position directions share d/dh of every
// atmospheric quantity and only the geodetic, longitude, gravity and force tangents are per direction.  Three dual<1> passes
// would run the value chain three times; the three directions at once take 162 VGPRs, no scratch, 3 waves per SIMD
// (make resource-usage).
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_eval_kernel.h"   // the compact slot numbers (kSlotPT ...)
#include "gel_exact.h"

namespace gel {

constexpr int kExactBlock = 256;

__global__ __launch_bounds__(kExactBlock) void exact_jac_kernel(ProblemDev P, int B, const double* __restrict__ x,
                                                                double* __restrict__ jvar) {
  extern __shared__ double lds[];
  const Tables tb = stage_tables(P, lds, true);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * P.N) return;
  const int N = P.N, M = P.M;
  const int b = (int)(t / N), g = (int)(t - (long long)b * N);
  const int sec = P.node_phase[g];
  const PhaseDev ph = P.phases[sec];
  const int n = ph.n, j = g - ph.ua;
  const int xj = ph.xa + 1 + j;
  const double* xb = x + (size_t)b * P.nvars;
  const double me = xb[xj];
  const double re[3] = {xb[M + 3 * xj], xb[M + 3 * xj + 1], xb[M + 3 * xj + 2]};
  const double ve[3] = {xb[4 * M + 3 * xj], xb[4 * M + 3 * xj + 1], xb[4 * M + 3 * xj + 2]};
  const double q[4] = {xb[7 * M + 4 * xj], xb[7 * M + 4 * xj + 1], xb[7 * M + 4 * xj + 2], xb[7 * M + 4 * xj + 3]};
  const double u0 = ph.hold ? 0.0 : xb[11 * M + 2 * g], u1 = ph.hold ? 0.0 : xb[11 * M + 2 * g + 1];
  const double to = xb[11 * M + 2 * N + sec], tf = xb[11 * M + 2 * N + sec + 1];
  const double tau = P.tau[ph.toff + j];
  const double djj = P.Dt[ph.doff + (size_t)(j + 1) * n + j];   // D[j][j+1]
  const double ut = P.ut, hT = P.hT;
  const double S = (tf - to) * ut / 2.0;                        // d(residual)/d(rhs) = -S
  const double inv_uv = P.inv_uv;

  // compact layout of the phase: [64-node chunk][slot][node of the chunk], the phase scalar behind (gel_host.hip compact_index)
  const int j0 = j & ~63, w = min(64, n - j0);
  double* const out = jvar + (size_t)b * P.V + ph.voff + (size_t)j0 * ph.K + (j - j0);
  bool bad = false;
#define XPUT(slot, val)                                        \
  do {                                                         \
    const double v_ = (val);                                   \
    out[(size_t)(slot) * w] = v_;                              \
    bad = bad || !(fabs(v_) <= 1.79769313486231570815e308);    \
  } while (0)

  // ---- position group (:155-213): t0 column (tf = its negative); the pos/velocity diagonal scalar of the phase ----
#pragma unroll
  for (int c = 0; c < 3; c++) XPUT(kSlotPT + c, ve[c] * P.kpt);
  if (j == 0) {
    const double sc = -(P.kpt * (tf - to));
    jvar[(size_t)b * P.V + ph.voff + (size_t)ph.K * n] = sc;
    bad = bad || !(fabs(sc) <= 1.79769313486231570815e308);
  }

  // ---- quaternion group (:499-632): dq = q (x) (0, 0, omega_y, omega_z) / 2 is linear in q and u (closed form) ----
  if (!ph.hold) {
    const double hS = (tf - to) * ut / 2.0;
    const double d2r = 0.017453292519943295769;
    XPUT(ph.s_qq + 0, 0.5 * ((u0 * P.uu) * d2r) * hS);
    XPUT(ph.s_qq + 1, 0.5 * ((u1 * P.uu) * d2r) * hS);
    const double kq = 0.5 * (P.uu * d2r) * hS;
    XPUT(ph.s_qq + 2, -(kq * q[0]));
    XPUT(ph.s_qq + 3, kq * q[1]);
    XPUT(ph.s_qq + 4, kq * q[2]);
    XPUT(ph.s_qq + 5, kq * q[3]);
    double fq[4];
    quat_rate(q, u0, u1, P.uu, fq);
#pragma unroll
    for (int c = 0; c < 4; c++) XPUT(ph.s_qq + 6 + c, fq[c] * hT);
  }

  // ---- velocity group (:216-496) ----
  const double tn = tau * (tf - to) / 2 + (tf + to) / 2;   // PSparams.time_nodes
  const double inv_m = frcp(me * P.um);
  const double r[3] = {re[0] * P.up, re[1] * P.up, re[2] * P.up};
  double dir[3];
  thrust_dir(q, dir);
  double T, fc[3], tm[3];
  double dfr[3][3];   // d(acc / unit_v)_c / d r_k (SI position): dfr[k][c]
  if (ph.air) {
    PosCentre pc;
    PosCentreTail tail;
    const PosPart pp = pos_part<true, PosCentreSink>(r, tb, P.barC20, nullptr, PosCentreSink{&pc}, &tail);
    const EarthAngle ea = earth_angle(tn);
    double wv[3], F[3];
    wind_eci_or_calm(r, ea, pp.sl, pp.cl, pp.inv_p, pp.wn, pp.we, wv);
    const double v[3] = {ve[0] * P.uv, ve[1] * P.uv, ve[2] * P.uv};
    aero_force(r, v, pp.rho, pp.inv_a, wv, ph.area, tb, F);
    T = ph.thrust - ph.nozzle * pp.P;
    {
      const double Td[3] = {T * dir[0], T * dir[1], T * dir[2]};
      accel_parts(Td, F, inv_m, pp.g, inv_uv, tm, fc);
    }
    // the air-relative velocity and the force's factors, as aero_force() forms them
    const double a[3] = {(v[0] + kOmega * r[1]) - wv[0], (v[1] - kOmega * r[0]) - wv[1], v[2] - wv[2]};
    const double s2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    const double s = fsqrt(fmax(s2, 1.0e-200));
    const double mach = s * pp.inv_a;
    const double ca = interp_tab(mach, tb.ca, tb.cas, tb.Kc, 2, 1);
    const double cas = interp_tab_slope(mach, tb.ca, tb.cas, tb.Kc, 2);
    const double kk = (s2 > 0.0) ? 0.5 * pp.rho * ph.area * ca * s : 0.0;
    // velocity columns (air_fd phases: reference_area > 0): da = e_k unit_v
    if (ph.air_fd) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double da[3] = {(k == 0) ? 1.0 : 0.0, (k == 1) ? 1.0 : 0.0, (k == 2) ? 1.0 : 0.0};
        double dF[3];
        aero_force_tangent(a, s2, s, pp.rho, pp.inv_a, ph.area, ca, cas, kk, da, 0.0, 0.0, dF);
#pragma unroll
        for (int c = 0; c < 3; c++) XPUT(ph.s_vv + 3 * k + c, ((c == k) ? djj : 0.0) - S * ((dF[c] * P.uv) * inv_m * inv_uv));
      }
    }
    // position columns: altitude -> atmosphere, wind; latitude / longitude -> wind axes; gravity; omega x r
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
    double dg[3][3];
    gravity_tangent(r, P.barC20, dg);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double da[3] = {((k == 1) ? kOmega : 0.0) - dw[k][0], ((k == 0) ? -kOmega : 0.0) - dw[k][1], -dw[k][2]};
      double dF[3];
      aero_force_tangent(a, s2, s, pp.rho, pp.inv_a, ph.area, ca, cas, kk, da, at.drho * dh[k], at.dinv_a * dh[k], dF);
      const double dT = -ph.nozzle * (at.dP * dh[k]);
#pragma unroll
      for (int c = 0; c < 3; c++) dfr[k][c] = ((dT * dir[c] + dF[c]) * inv_m + dg[k][c]) * inv_uv;
    }
  } else {
    // NoAir (reference_area == 0): thrust + gravity (src/pybind_dynamics.cpp:73-92)
    T = ph.thrust;
    double gc[3];
    gravity_eci(r, P.barC20, gc);
#pragma unroll
    for (int c = 0; c < 3; c++) { tm[c] = (T * dir[c]) * inv_m; fc[c] = (tm[c] + gc[c]) * inv_uv; }
    double dg[3][3];
    gravity_tangent(r, P.barC20, dg);
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) dfr[k][c] = dg[k][c] * inv_uv;
  }
  // position columns: x_pos = r / unit_p
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) XPUT(kSlotVP + 3 * k + c, -S * (P.up * dfr[k][c]));
  // mass column: d((T d + F) / m) / d m = -(T d + F) / m^2
  {
    const double km = (P.um * inv_m) * (inv_uv * S);
#pragma unroll
    for (int c = 0; c < 3; c++) XPUT(kSlotVM + c, tm[c] * km);
  }
  // quaternion columns: the thrust direction quatrot(conj(q), e1) is a quadratic form of q (thrust_dir())
  {
    const double kqe = (T * inv_m) * (inv_uv * S);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double a_ = (k < 2) ? -kqe : kqe;   // d dir_x / d q_k = +-2 q_k
      const double b_ = -2.0 * kqe;
      XPUT(ph.s_vq + 3 * k + 0, (2.0 * q[k]) * a_);
      XPUT(ph.s_vq + 3 * k + 1, q[3 - k] * b_);                            // d dir_y / d q = 2 (q3, q2, q1, q0)
      XPUT(ph.s_vq + 3 * k + 2, ((k & 1) ? q[k ^ 2] : -q[k ^ 2]) * b_);    // d dir_z / d q = 2 (-q2, q3, -q0, q1)
    }
  }
  // t0 column (tf = its negative): the RHS does not depend on t (the Earth angle's rotations cancel)
#pragma unroll
  for (int c = 0; c < 3; c++) XPUT(ph.s_vt + c, fc[c] * hT);
#undef XPUT
  if (bad) *(volatile int32_t*)P.flag = 1;
}

hipError_t launch_eval_exact(const ProblemDev& P, int B, const double* d_x, double* d_jvar, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (P.fd_recompute || !d_jvar) return hipErrorInvalidValue;   // the default compact layout only (t0 / tf, quaternion slots)
  const long long threads = (long long)B * P.N;
  const unsigned grid = (unsigned)((threads + kExactBlock - 1) / kExactBlock);
  const size_t lds = table_lds_bytes(P.Kw, P.Kc);
  hipLaunchKernelGGL(exact_jac_kernel, dim3(grid), dim3(kExactBlock), lds, s, P, B, d_x, d_jvar);
  return hipGetLastError();
}

}  // namespace gel
