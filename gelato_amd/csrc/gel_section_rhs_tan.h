// gel_section_rhs_tan.h -- the right-hand side F of gel_section_rhs.h together with its tangent dF along ONE direction, for the
// tangent-linear propagation (gel_kernels_proptan.hip).
//
// Values: the functions section_rhs<true> calls, on the same arguments in the same order, so F has section_rhs<true>'s bits; the air
// branch's are linearise_air's (gel_section_rhs_lin.h), which also forms the partials -- gel_exact.h's helpers, written for the
// three unit position directions.  Here they are contracted with the direction's position part.
//
// The direction (everything in the units of the value call):
//   dxt [11]   the state: mass | position 3 | velocity 3 | quaternion 4, normalised
//   du0, du1   the controls (not read by a hold phase)
//   dthrust, dmf, darea   the tangents of ph.thrust, ph.mf_um and ph.area AS THE VALUE CALL HOLDS THEM: the caller scaled the
//              handle's thrust by its factor f0, so its tangent is (the handle's thrust) df0; likewise mf_um df1 and area df2
//   dfw        the tangent of the wind factor: d(wn fw) = fw dwn + wn dfw, the same for we
// THE TIME: F reads the time only through the Earth angle, which wind_eci reads only exactly on the polar axis.  Its tangent is
// taken as gel_kernels_exact.hip takes it for the t columns of the velocity rows: zero (the rotations by the Earth angle cancel
// off the axis, and on it the longitude is held, like the partials of p and of the longitude there).  The knot times therefore
// enter a flight's tangent through the step S h alone.
//
// kWind (gel_propagate_tangent_wind*): the direction also moves the VALUES of the wind table, by the seed dwl [Kw][2]
// (north, east per row; the altitudes stay).  The seed is looked up on the piece the value lookup took (gel_wind_rows.h), times fw,
// and added to dwn / dwe beside the factor's term; where that product is zero the sum is not formed, so a zero seed leaves the
// bits of the instantiation without it.  kWind = false reads none of this and is the function it was.
#pragma once
#include "gel_section_rhs_lin.h"
#include "gel_wind_rows.h"

namespace gel {

struct RhsDirection {
  double du0, du1;
  double dthrust, dmf, darea, dfw;
};

template <bool kWind = false>
GEL_DEV void section_rhs_tangent(const ProblemDev& P, const PhaseDev& ph, const Tables& tb, double vp, double sig, double to,
                                 double tf, const double xt[11], double u0, double u1, double fw, const double dxt[11],
                                 const RhsDirection& d, double F[11], double dF[11], const double* dwl = nullptr) {
  F[0] = ph.engine_on ? ph.mf_um : 0.0;
  dF[0] = ph.engine_on ? d.dmf : 0.0;
#pragma unroll
  for (int c = 0; c < 3; c++) { F[1 + c] = xt[4 + c] * vp; dF[1 + c] = dxt[4 + c] * vp; }
  const double m = xt[0] * P.um;
  const double r[3] = {xt[1] * P.up, xt[2] * P.up, xt[3] * P.up};
  const double q[4] = {xt[7], xt[8], xt[9], xt[10]};
  const double dm = dxt[0] * P.um;
  const double dr[3] = {dxt[1] * P.up, dxt[2] * P.up, dxt[3] * P.up};
  const double dq[4] = {dxt[7], dxt[8], dxt[9], dxt[10]};
  double dir[3], f[3], df[3];
  thrust_dir(q, dir);
  // the thrust direction is a quadratic form of q (thrust_dir())
  const double ddir[3] = {2.0 * (q[0] * dq[0] + q[1] * dq[1] - q[2] * dq[2] - q[3] * dq[3]),
                          2.0 * (q[0] * dq[3] + q[3] * dq[0] + q[1] * dq[2] + q[2] * dq[1]),
                          2.0 * (q[1] * dq[3] + q[3] * dq[1] - q[0] * dq[2] - q[2] * dq[0])};
  const double inv_m = 1.0 / m;
  double dg[3][3];
  gravity_tangent(r, P.barC20, dg);
  if (ph.air) {
    AirLinearisation L;
    linearise_air(P, ph, tb, sig, to, tf, xt, r, dir, inv_m, fw, L, f);
    // ---- the contraction with the direction ----
    const double dhd = L.dh[0] * dr[0] + L.dh[1] * dr[1] + L.dh[2] * dr[2];
    // the wind factor's direction: (wn N + we E) dfw with the value's axes
    double dwn = L.pp.wn * d.dfw, dwe = L.pp.we * d.dfw;
    if constexpr (kWind) {   // the table's own direction: the seed on the value's piece, times the factor
      const WindRows wr = wind_rows(L.tail.h, L.tail.piece, tb.wind, tb.Kw);
      const double sn = wind_rows_seed(wr, dwl, 0) * fw, se = wind_rows_seed(wr, dwl, 1) * fw;
      dwn = (sn == 0.0) ? dwn : dwn + sn;
      dwe = (se == 0.0) ? dwe : dwe + se;
    }
    const double dw[3] = {L.dw3[0][0] * dr[0] + L.dw3[1][0] * dr[1] + L.dw3[2][0] * dr[2] + (dwn * (-L.pc.sl * L.clon) + dwe * (-L.slon)),
                          L.dw3[0][1] * dr[0] + L.dw3[1][1] * dr[1] + L.dw3[2][1] * dr[2] + (dwn * (-L.pc.sl * L.slon) + dwe * L.clon),
                          L.dw3[0][2] * dr[0] + L.dw3[1][2] * dr[1] + L.dw3[2][2] * dr[2] + dwn * L.pc.cl};
    const double da[3] = {(dxt[4] * P.uv + kOmega * dr[1]) - dw[0], (dxt[5] * P.uv - kOmega * dr[0]) - dw[1], dxt[6] * P.uv - dw[2]};
    double dFa[3];
    aero_force_tangent(L.a, L.s2, L.s, L.pp.rho, L.pp.inv_a, ph.area, L.ca, L.cas, L.kk, da, L.at.drho * dhd, L.at.dinv_a * dhd, dFa);
    // the reference area enters k = rho area CA |a| / 2 linearly
    const double dka = (L.s2 > 0.0) ? 0.5 * L.pp.rho * d.darea * L.ca * L.s : 0.0;
    const double dT = d.dthrust - ph.nozzle * (L.at.dP * dhd);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double tm = (L.Td[c] + L.Fa[c]) * inv_m;   // (thrust + aero) / m, whose mass derivative is -tm / m
      const double dgc = dg[0][c] * dr[0] + dg[1][c] * dr[1] + dg[2][c] * dr[2];
      df[c] = (((dT * dir[c] + L.T * ddir[c]) + (dFa[c] - dka * L.a[c])) * inv_m - (tm * inv_m) * dm + dgc) * P.inv_uv;
    }
  } else {
    double g[3];
    gravity_eci(r, P.barC20, g);
    const double Td[3] = {ph.thrust * dir[0], ph.thrust * dir[1], ph.thrust * dir[2]};
    accel_noair(Td, inv_m, g, P.inv_uv, f);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double tm = Td[c] * inv_m;
      const double dgc = dg[0][c] * dr[0] + dg[1][c] * dr[1] + dg[2][c] * dr[2];
      df[c] = ((d.dthrust * dir[c] + ph.thrust * ddir[c]) * inv_m - (tm * inv_m) * dm + dgc) * P.inv_uv;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) { F[4 + c] = f[c]; dF[4 + c] = df[c]; }
  double fq[4] = {0.0, 0.0, 0.0, 0.0}, dfq[4] = {0.0, 0.0, 0.0, 0.0};
  if (!ph.hold) {
    quat_rate(q, u0, u1, P.uu, fq);
    // bilinear in (q, u): the rate of dq under u plus the rate of q under du
    double t1[4], t2[4];
    quat_rate(dq, u0, u1, P.uu, t1);
    quat_rate(q, d.du0, d.du1, P.uu, t2);
#pragma unroll
    for (int c = 0; c < 4; c++) dfq[c] = t1[c] + t2[c];
  }
#pragma unroll
  for (int c = 0; c < 4; c++) { F[7 + c] = fq[c]; dF[7 + c] = dfq[c]; }
}

}  // namespace gel
