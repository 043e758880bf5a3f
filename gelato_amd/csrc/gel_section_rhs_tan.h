// gel_section_rhs_tan.h -- the right-hand side F of gel_section_rhs.h together with its tangent dF along ONE direction, for the
// tangent-linear propagation (gel_kernels_proptan.hip).
//
// Values: the functions section_rhs<true> calls, on the same arguments in the same order (pos_part's CENTRE form and
// wind_ned2_centre are the same value expressions), so F has section_rhs<true>'s bits.  Tangents: gel_exact.h's helpers -- written
// for the three unit position directions -- contracted with the direction's position part; their conventions at kinks (table
// knots, clamps, atmosphere layers, r < b, |v_air| = 0, the polar axis) are gel_exact.h's and are not restated here.
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
#include "gel_exact.h"
#include "gel_section_rhs.h"
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
    const double v3[3] = {xt[4] * P.uv, xt[5] * P.uv, xt[6] * P.uv};
    PosCentre pc;
    PosCentreTail tail;
    const PosPart pp = pos_part<true, PosCentreSink>(r, tb, P.barC20, nullptr, PosCentreSink{&pc}, &tail);
    const EarthAngle ea = earth_angle(sig * (tf - to) / 2 + (tf + to) / 2);
    double w[3], Fa[3];
    const double wn = pp.wn * fw, we = pp.we * fw;
    wind_eci_or_calm(r, ea, pp.shp, pp.chp, pp.inv_p, wn, we, w);
    aero_force(r, v3, pp.rho, pp.inv_a, w, ph.area, tb, Fa);
    const double T = ph.thrust - ph.nozzle * pp.P;
    const double Td[3] = {T * dir[0], T * dir[1], T * dir[2]};
    accel(Td, Fa, inv_m, pp.g, P.inv_uv, f);
    // ---- the tangent ----
    // the air-relative velocity and the force's factors, as aero_force() forms them
    const double a[3] = {(v3[0] + kOmega * r[1]) - w[0], (v3[1] - kOmega * r[0]) - w[1], v3[2] - w[2]};
    const double s2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    const double s = fsqrt(fmax(s2, 1.0e-200));
    const double mach = s * pp.inv_a;
    const double ca = interp_tab(mach, tb.ca, tb.cas, tb.Kc, 2, 1);
    const double cas = interp_tab_slope(mach, tb.ca, tb.cas, tb.Kc, 2);
    const double kk = (s2 > 0.0) ? 0.5 * pp.rho * ph.area * ca * s : 0.0;
    // altitude -> atmosphere, wind; latitude / longitude -> wind axes (the three unit directions, then the contraction)
    double dsl[3], dcl[3], dalt[3], dh[3];
    geodetic_tangent(r, pp.inv_p, pc, dsl, dcl, dalt);
#pragma unroll
    for (int k = 0; k < 3; k++) dh[k] = (pc.G * pc.G) * dalt[k];
    const double Tk = pp.P / (pp.rho * tb.atm[33 + tail.k]);
    const AirTangent at = atmosphere_tangent(tail.h, Tk, pp.P, pp.rho, pp.inv_a, tb.atm);
    const bool in = tail.piece >= 0;
    const double s0 = in ? tb.winds[2 * tail.piece] * fw : 0.0, s1 = in ? tb.winds[2 * tail.piece + 1] * fw : 0.0;
    const double clon = (pp.inv_p > 0.0) ? r[0] * pp.inv_p : ea.c, slon = (pp.inv_p > 0.0) ? r[1] * pp.inv_p : ea.s;
    double dw3[3][3];
    wind_eci_tangent(r, pp.inv_p, clon, slon, pc.sl, pc.cl, wn, we, s0, s1, dh, dsl, dcl, dw3);
    const double dhd = dh[0] * dr[0] + dh[1] * dr[1] + dh[2] * dr[2];
    // the wind factor's direction: (wn N + we E) dfw with the value's axes
    double dwn = pp.wn * d.dfw, dwe = pp.we * d.dfw;
    if constexpr (kWind) {   // the table's own direction: the seed on the value's piece, times the factor
      const WindRows wr = wind_rows(tail.h, tail.piece, tb.wind, tb.Kw);
      const double sn = wind_rows_seed(wr, dwl, 0) * fw, se = wind_rows_seed(wr, dwl, 1) * fw;
      dwn = (sn == 0.0) ? dwn : dwn + sn;
      dwe = (se == 0.0) ? dwe : dwe + se;
    }
    const double dw[3] = {dw3[0][0] * dr[0] + dw3[1][0] * dr[1] + dw3[2][0] * dr[2] + (dwn * (-pc.sl * clon) + dwe * (-slon)),
                          dw3[0][1] * dr[0] + dw3[1][1] * dr[1] + dw3[2][1] * dr[2] + (dwn * (-pc.sl * slon) + dwe * clon),
                          dw3[0][2] * dr[0] + dw3[1][2] * dr[1] + dw3[2][2] * dr[2] + dwn * pc.cl};
    const double da[3] = {(dxt[4] * P.uv + kOmega * dr[1]) - dw[0], (dxt[5] * P.uv - kOmega * dr[0]) - dw[1], dxt[6] * P.uv - dw[2]};
    double dFa[3];
    aero_force_tangent(a, s2, s, pp.rho, pp.inv_a, ph.area, ca, cas, kk, da, at.drho * dhd, at.dinv_a * dhd, dFa);
    // the reference area enters k = rho area CA |a| / 2 linearly
    const double dka = (s2 > 0.0) ? 0.5 * pp.rho * d.darea * ca * s : 0.0;
    const double dT = d.dthrust - ph.nozzle * (at.dP * dhd);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double tm = (Td[c] + Fa[c]) * inv_m;   // (thrust + aero) / m, whose mass derivative is -tm / m
      const double dgc = dg[0][c] * dr[0] + dg[1][c] * dr[1] + dg[2][c] * dr[2];
      df[c] = (((dT * dir[c] + T * ddir[c]) + (dFa[c] - dka * a[c])) * inv_m - (tm * inv_m) * dm + dgc) * P.inv_uv;
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
