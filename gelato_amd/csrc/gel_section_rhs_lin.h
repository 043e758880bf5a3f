// gel_section_rhs_lin.h -- the air branch of the right-hand side linearised at one point, once: the value lines of section_rhs<true>
// (pos_part's CENTRE form and wind_ned2_centre: the same value expressions, hence its bits) and every partial that
// section_rhs_tangent contracts with a direction (gel_section_rhs_tan.h) and section_rhs_adjoint with a multiplier
// (gel_section_rhs_adj.h).  The adjoint is the tangent's transpose only while both read the SAME partials: these.
// gel_exact.h's conventions at kinks (table knots, clamps, atmosphere layers, r < b, |v_air| = 0, the polar axis) hold.
#pragma once
#include "gel_exact.h"
#include "gel_section_rhs.h"

namespace gel {

struct AirLinearisation {
  PosPart pp;            // the position part, its centre terms and the layer / wind piece the lookups took
  PosCentre pc;
  PosCentreTail tail;
  EarthAngle ea;
  AirTangent at;         // the atmosphere by altitude
  double wn, we;         // the wind as F reads it: interpolated, times fw
  double T, Td[3], Fa[3];   // thrust less the nozzle's back pressure, along the thrust direction; the aerodynamic force
  double a[3], s2, s;    // the air-relative velocity as aero_force() forms it, |a|^2, |a| (floored)
  double ca, cas, kk;    // CA at the Mach number, its slope, k = rho area CA |a| / 2 (0 where |a| = 0)
  double dh[3], clon, slon, dw3[3][3];   // altitude by position; cos / sin of the longitude; dw3[k][i]: wind i (ECI) by position k
};

// xt: the stage's state; r = its position, dir = its thrust direction, inv_m = 1 / mass, as the caller formed them.  Out: f [3], the
// acceleration rows of F.
GEL_DEV void linearise_air(const ProblemDev& P, const PhaseDev& ph, const Tables& tb, double sig, double to, double tf, const double xt[11],
                           const double r[3], const double dir[3], double inv_m, double fw, AirLinearisation& L, double f[3]) {
  const double v3[3] = {xt[4] * P.uv, xt[5] * P.uv, xt[6] * P.uv};
  L.pp = pos_part<true, PosCentreSink>(r, tb, P.barC20, nullptr, PosCentreSink{&L.pc}, &L.tail);
  const PosPart& pp = L.pp;
  const PosCentre& pc = L.pc;
  L.ea = earth_angle(sig * (tf - to) / 2 + (tf + to) / 2);
  double w[3];
  L.wn = pp.wn * fw;
  L.we = pp.we * fw;
  wind_eci_or_calm(r, L.ea, pp.sl, pp.cl, pp.inv_p, L.wn, L.we, w);
  aero_force(r, v3, pp.rho, pp.inv_a, w, ph.area, tb, L.Fa);
  L.T = ph.thrust - ph.nozzle * pp.P;
#pragma unroll
  for (int c = 0; c < 3; c++) L.Td[c] = L.T * dir[c];
  accel(L.Td, L.Fa, inv_m, pp.g, P.inv_uv, f);
  // the air-relative velocity and the force's factors, as aero_force() forms them
  L.a[0] = (v3[0] + kOmega * r[1]) - w[0];
  L.a[1] = (v3[1] - kOmega * r[0]) - w[1];
  L.a[2] = v3[2] - w[2];
  L.s2 = L.a[0] * L.a[0] + L.a[1] * L.a[1] + L.a[2] * L.a[2];
  L.s = fsqrt(fmax(L.s2, 1.0e-200));
  const double mach = L.s * pp.inv_a;
  L.ca = interp_tab(mach, tb.ca, tb.cas, tb.Kc, 2, 1);
  L.cas = interp_tab_slope(mach, tb.ca, tb.cas, tb.Kc, 2);
  L.kk = (L.s2 > 0.0) ? 0.5 * pp.rho * ph.area * L.ca * L.s : 0.0;
  // altitude -> atmosphere, wind; latitude / longitude -> wind axes (the three unit directions)
  double dsl[3], dcl[3], dalt[3];
  geodetic_tangent(r, pp.inv_p, pc, dsl, dcl, dalt);
#pragma unroll
  for (int k = 0; k < 3; k++) L.dh[k] = (pc.G * pc.G) * dalt[k];
  const double Tk = pp.P / (pp.rho * tb.atm[33 + L.tail.k]);
  L.at = atmosphere_tangent(L.tail.h, Tk, pp.P, pp.rho, pp.inv_a, tb.atm);
  const bool in = L.tail.piece >= 0;
  const double s0 = in ? tb.winds[2 * L.tail.piece] * fw : 0.0, s1 = in ? tb.winds[2 * L.tail.piece + 1] * fw : 0.0;
  L.clon = (pp.inv_p > 0.0) ? r[0] * pp.inv_p : L.ea.c;
  L.slon = (pp.inv_p > 0.0) ? r[1] * pp.inv_p : L.ea.s;
  wind_eci_tangent(r, pp.inv_p, L.clon, L.slon, pc.sl, pc.cl, L.wn, L.we, s0, s1, L.dh, dsl, dcl, L.dw3);
}

}  // namespace gel
