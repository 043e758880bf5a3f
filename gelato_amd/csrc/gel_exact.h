// gel_exact.h -- tangent forms of the defect RHS chain for the exact-Jacobian kernel (gel_kernels_exact.hip,
// GEL_FLAG_EXACT_DEFECT_JAC).
//
// Forward mode: every value is produced by the functions the fused kernel uses (gel_physics.h, gel_rhs_parts.h); what is
// added here is the TANGENT of each step, formed from those values.  The chain from the position to the atmosphere and the
// wind runs through one scalar (the geopotential altitude h), so it is carried as d/dh of each quantity times dh/dr_k; the
// geodetic latitude, the longitude, gravity and the air-relative velocity carry the three position directions explicitly.
//
// Conventions at the points where the value computation is not differentiable: the derivative of the branch the value took.
//   interp (wind, CA)   the slope of the table interval used (x == a knot: the interval it closes, as lower_count picks it);
//                       0 where the value is clamped, including x <= xp[0] (np.interp's value there);
//   atmosphere          the US-1976 layer used (us76_layer) and the temperature law of that altitude band; the 86 km switch of
//                       the geopotential altitude: dh/dalt = (r0 / (r0 + alt))^2 below, 1 at and above;
//   gravity             r < b: the clamped magnitude terms (mu / r^2, a / r) are constant, the direction terms still vary;
//   |v_air| = 0         d|v_air| = 0 and the force's tangent is 0 (|v| v CA(|v|/a) is C^1 with derivative 0 there);
//   polar axis p = 0    the partials of p = sqrt(x^2 + y^2) and of the longitude are 0; the longitude is the value code's
//                       (Earth angle of the node's time); the altitude there is the reference's -N, constant along the axis
//                       (its tangent is 0).  Every tangent is finite wherever the value is.
#pragma once
#include "gel_rhs_parts.h"

namespace gel {

// d/dx of interp_tab(x, ...) on the branch its value took
GEL_DEV double interp_tab_slope(double x, const double* tab, const double* slope, int n, int stride) {
  const int idx = min(max(lower_count(x, tab, n, stride) - 1, 0), n - 2);
  return (x <= tab[0] || x > tab[(n - 1) * stride]) ? 0.0 : slope[idx];
}

// d/dh of pressure, density and 1 / speed of sound at geopotential altitude h (atmosphere(), src/Air.cpp:71-111), from its
// values P, rho, inv_a and the temperature T
struct AirTangent { double dP, drho, dinv_a; };
GEL_DEV AirTangent atmosphere_tangent(double h, double T, double P, double rho, double inv_a, const double* atm) {
  const int k = us76_layer(h);
  const double Hb = atm[66 + k], Lmb = atm[k], Tmb = atm[11 + k], R = atm[33 + k];
  double dT;
  if (h <= 91000.0) {
    dT = Lmb;
  } else if (h <= 110000.0) {   // T = Tc + A sqrt(1 - y^2), y = (h - 91000) / a
    const double a = -19942.9, y = (h - 91000.0) / a;
    dT = -76.3232 * (-(y / a)) / sqrt(1.0 - y * y);
  } else if (h <= 120000.0) {
    dT = Lmb;
  } else {                      // T = Tinf - (Tinf - Tmb) exp(-l xi), dxi/dh = ((r0 + Hb) / (r0 + h))^2
    const double r0 = 6356766.0, q = (r0 + Hb) / (r0 + h);
    dT = 0.01875e-3 * (1000.0 - T) * (q * q);
  }
  AirTangent o;
  // the pressure law follows the layer's linear temperature profile in every band (src/Air.cpp:90-98)
  o.dP = (fabs(Lmb) > 1.0e-6) ? P * atm[44 + k] * Lmb / (Tmb + Lmb * (h - Hb)) : -P * (atm[55 + k] * atm[77 + k]);
  o.drho = o.dP / (R * T) - rho * dT / T;
  o.dinv_a = -0.5 * inv_a * dT / T;
  return o;
}

// Tangents of the geodetic chain (Bowring, src/Earth.cpp:49-61) along the three ECI position directions, from the centre's
// exported intermediates (PosCentre: p, 1/hypot(z Ra, p Rb), 1/hypot(zz, pp), sin / cos / 1/cos of the latitude, N):
// dsl, dcl (sin / cos latitude) and dalt per direction k.
GEL_DEV void geodetic_tangent(const double r[3], double inv_p, const PosCentre& pc, double dsl[3], double dcl[3], double dalt[3]) {
  const double a = r[2] * kRa, b = pc.p * kRb;
  const double st = a * pc.ih, ct = b * pc.ih;
  const double K1 = 3.0 * kEp2 * kRb, K2 = 3.0 * kE2 * kRa;
  const double kN = pc.N * pc.N * pc.N * (kE2 / (kRa * kRa));   // dN = N^3 e^2 / Ra^2 sin(lat) dsl
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double dp = (k < 2) ? r[k] * inv_p : 0.0;   // inv_p = 0 on the polar axis
    const double dz = (k == 2) ? 1.0 : 0.0;
    const double da = dz * kRa, db = dp * kRb;
    const double dH = st * da + ct * db;               // d hypot(a, b) / hypot(a, b)
    const double dst = pc.ih * (da - st * dH), dct = pc.ih * (db - ct * dH);
    const double dzz = dz + K1 * (st * st) * dst, dpp = dp - K2 * (ct * ct) * dct;
    const double dY = pc.sl * dzz + pc.cl * dpp;
    dsl[k] = pc.ihy * (dzz - pc.sl * dY);
    dcl[k] = pc.ihy * (dpp - pc.cl * dY);
    // alt = p / cos(lat) - N; icl = (p / cl) / p is 0 on the polar axis, where the value is -N
    dalt[k] = (dp - pc.p * pc.icl * dcl[k]) * pc.icl - kN * pc.sl * dsl[k];
  }
}

// d g_i / d r_k of the J2 gravity (gravity_eci(), src/gravity.cpp:11-57): dg[k][i]
GEL_DEV void gravity_tangent(const double r3[3], double barC20, double dg[3][3]) {
  const double a = 6378137.0, mu = kMu;
  const double b = a * (1.0 - 1.0 / 298.257223563);
  double r, inv_r;
  fsqrt_rsqrt(fmax(r3[0] * r3[0] + r3[1] * r3[1] + r3[2] * r3[2], 1.0e-300), r, inv_r);
  const bool on = r > 1.0e-150;
  const double ir[3] = {on ? r3[0] * inv_r : 0.0, on ? r3[1] * inv_r : 0.0, on ? r3[2] * inv_r : 0.0};
  const double irv = on ? inv_r : 0.0;
  const bool clamp = r < b;
  const double irm = clamp ? 1.0 / b : inv_r;
  const double s5 = 2.23606797749978969641;
  const double irz = ir[2];
  const double P20 = s5 * (3.0 * irz * irz - 1.0) * 0.5, P20d = s5 * 3.0 * irz;
  const double mur2 = mu * (irm * irm), ar = a * irm;
  const double X = 3.0 * P20 + irz * P20d;
  const double Q = 1.0 + barC20 * ar * ar * X;
  const double g_ir = -mur2 * Q;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double dir[3];
#pragma unroll
    for (int i = 0; i < 3; i++) dir[i] = (((i == k) ? 1.0 : 0.0) - ir[i] * ir[k]) * irv;
    const double drm = clamp ? 0.0 : ir[k];
    const double dmur2 = -2.0 * mur2 * drm * irm, dar = -ar * drm * irm;
    const double dP20 = s5 * 3.0 * irz * dir[2], dP20d = s5 * 3.0 * dir[2];
    const double dX = 3.0 * dP20 + dir[2] * P20d + irz * dP20d;
    const double dQ = barC20 * (2.0 * ar * dar * X + ar * ar * dX);
    const double dgir = -(dmur2 * Q + mur2 * dQ);
    const double dgiz = barC20 * (dmur2 * ar * ar * P20d + 2.0 * mur2 * ar * dar * P20d + mur2 * ar * ar * dP20d);
#pragma unroll
    for (int i = 0; i < 3; i++) dg[k][i] = dgir * ir[i] + g_ir * dir[i] + ((i == 2) ? dgiz : 0.0);
  }
}

// The wind in ECI is wn N + we E with the local north / east axes N = (-sin lat cos lon, -sin lat sin lon, cos lat),
// E = (-sin lon, cos lon, 0) at the ECI longitude lon (what wind_eci()'s quaternion chain composes to: the rotations by the
// Earth angle cancel).  Its tangent along r_k from the altitude's (dh), the latitude's (dsl, dcl) and the longitude's.
// (clon, slon): cos / sin of the ECI longitude the value took.
GEL_DEV void wind_eci_tangent(const double r[3], double inv_p, double clon, double slon, double sl, double cl, double wn, double we,
                              double s0, double s1, const double dh[3], const double dsl[3], const double dcl[3], double dw[3][3]) {
  const double Nh[3] = {-sl * clon, -sl * slon, cl}, Eh[3] = {-slon, clon, 0.0};
  const double ip2 = inv_p * inv_p;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double dlon = (k == 0) ? -r[1] * ip2 : ((k == 1) ? r[0] * ip2 : 0.0);
    const double dN[3] = {-dsl[k] * clon + sl * slon * dlon, -dsl[k] * slon - sl * clon * dlon, dcl[k]};
    const double dE[3] = {-clon * dlon, -slon * dlon, 0.0};
    const double dwn = s0 * dh[k], dwe = s1 * dh[k];
#pragma unroll
    for (int i = 0; i < 3; i++) dw[k][i] = dwn * Nh[i] + wn * dN[i] + dwe * Eh[i] + we * dE[i];
  }
}

// Tangent of the axial aerodynamic force F = -k a, k = rho area CA(|a| / a_s) |a| / 2 (aero_force()) along one direction:
// da (air-relative velocity), drho, dinv_a.  kk = k of the value (0 where |a| = 0), s = |a|, ca / cas = CA and its slope.
GEL_DEV void aero_force_tangent(const double a[3], double s2, double s, double rho, double inv_a, double area, double ca, double cas,
                                double kk, const double da[3], double drho, double dinv_a, double dF[3]) {
  const double ds = (s2 > 0.0) ? (a[0] * da[0] + a[1] * da[1] + a[2] * da[2]) / s : 0.0;
  const double dM = ds * inv_a + s * dinv_a;
  const double dk = (s2 > 0.0) ? 0.5 * area * (drho * ca * s + rho * (cas * dM) * s + rho * ca * ds) : 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) dF[i] = -(dk * a[i] + kk * da[i]);
}

}  // namespace gel
