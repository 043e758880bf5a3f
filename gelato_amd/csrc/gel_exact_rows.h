// gel_exact_rows.h -- forward-mode (value, tangent) forms of the node functions of the row table (gel_rows_body.h node_fn,
// iip_faa, distance_vincenty) for the exact row Jacobian (gel_kernels_exact_rows.hip, GEL_FLAG_EXACT_ROWS_JAC).
//
// Every function is restated statement for statement on a scalar fp64 dual number (value, tangent along ONE direction).  The
// value part of each step is the expression the value code rounds (the geodetic chain calls the very helpers of geodetic_full;
// elsewhere a product-sum the value code's compiler fuses may round once more here), and every branch and every loop exit is
// decided by the value part alone, as in the value computation: IIP's five steps and
// early returns, Vincenty's |d lambda| < 1e-12 break.  The tangent never decides anything.  All lanes of one row carry the same
// value part, so they take the same branches and leave Vincenty's loop together.
//
// Conventions where the value is not differentiable -- the derivative of the branch the value took:
//   IIP without a solution   (below the surface, not elliptic, positive perigee, no intersection, not converged: the (0, 0)
//                            fill) every tangent is 0;
//   inclination              c_z / |c| = +-1 exactly (equatorial orbit): acos' tangent is 0 (as is asin's at +-1);
//   norms at exactly 0       (|c|, e, |r|, |v|, the IIP norms): the root's tangent is 0;
//   polar axis p = 0         the partials of p = sqrt(x^2 + y^2) and of the longitude are 0 (gel_exact.h); the latitude and the
//                            altitude (-N there) then have tangent 0 as well;
//   Vincenty                 lon2 - lon1 == 0 exactly (the value 0 by that branch): 0; otherwise the tangent carried through
//                            the loop (it converges with lambda: the iteration contracts by about the flattening per trip);
//   atan2(0, 0)              tangent 0.
#pragma once
#include "gel_physics.h"

namespace gel {

struct Dual { double v, d; };

GEL_DEV Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
GEL_DEV Dual operator+(Dual a, double b) { return {a.v + b, a.d}; }
GEL_DEV Dual operator+(double a, Dual b) { return {a + b.v, b.d}; }
GEL_DEV Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
GEL_DEV Dual operator-(Dual a, double b) { return {a.v - b, a.d}; }
GEL_DEV Dual operator-(double a, Dual b) { return {a - b.v, -b.d}; }
GEL_DEV Dual operator-(Dual a) { return {-a.v, -a.d}; }
GEL_DEV Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
GEL_DEV Dual operator*(Dual a, double b) { return {a.v * b, a.d * b}; }
GEL_DEV Dual operator*(double a, Dual b) { return {a * b.v, a * b.d}; }
GEL_DEV Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
GEL_DEV Dual operator/(Dual a, double b) { return {a.v / b, a.d / b}; }
GEL_DEV Dual operator/(double a, Dual b) {
  const double q = a / b.v;
  return {q, -(q * b.d) / b.v};
}
GEL_DEV Dual dsqrt(Dual a) {
  const double s = sqrt(a.v);
  return {s, (s > 0.0) ? a.d / (2.0 * s) : 0.0};   // a norm at exactly 0: tangent 0
}
GEL_DEV Dual dsin(Dual a) { return {sin(a.v), cos(a.v) * a.d}; }
GEL_DEV Dual dcos(Dual a) { return {cos(a.v), -sin(a.v) * a.d}; }
GEL_DEV void dsincos(Dual a, Dual& sn, Dual& cs) {
  double s, c;
  sincos(a.v, &s, &c);
  sn = {s, c * a.d};
  cs = {c, -s * a.d};
}
GEL_DEV Dual dtan(Dual a) {
  const double t = tan(a.v);
  return {t, (1.0 + t * t) * a.d};
}
GEL_DEV Dual dasin(Dual a) {
  const double w = 1.0 - a.v * a.v;
  return {asin(a.v), (w > 0.0) ? a.d / sqrt(w) : 0.0};
}
GEL_DEV Dual dacos(Dual a) {
  const double w = 1.0 - a.v * a.v;
  return {acos(a.v), (w > 0.0) ? -a.d / sqrt(w) : 0.0};   // c_z / |c| = +-1 exactly: 0
}
GEL_DEV Dual datan(Dual a) { return {atan(a.v), a.d / (1.0 + a.v * a.v)}; }
GEL_DEV Dual datan2(Dual y, Dual x) {
  const double r2 = x.v * x.v + y.v * y.v;
  return {atan2(y.v, x.v), (r2 > 0.0) ? (x.v * y.d - y.v * x.d) / r2 : 0.0};
}

// geodetic_full (gel_physics.h, Bowring one step) with tangents: the values by the same helper calls, hence the same bits
GEL_DEV void geodetic_full_dual(Dual x, Dual y, Dual z, Dual& lat, Dual& lon, Dual& alt) {
  double latv, p, ip, ih, ihy;
  geodetic_lat_p(x.v, y.v, z.v, latv, p, ip, &ih, &ihy);
  const double lonv = atan2(y.v, x.v);
  double sl, cl;
  fsincos(latv, &sl, &cl);
  const double N = fdiv(kRa, fsqrt(1.0 - kE2 * sl * sl));
  const double altv = fdiv(p, cl) - N;
  // tangents: p (0 on the polar axis, where ip = 0), theta = atan2(z Ra, p Rb) through (st, ct), lat = atan2(zz, pp)
  const double dp = (x.v * x.d + y.v * y.d) * ip;
  const double a = z.v * kRa, b = p * kRb, da = z.d * kRa, db = dp * kRb;
  const bool h = a * a + b * b > 0.0;
  const double st = h ? a * ih : 0.0, ct = h ? b * ih : 1.0;
  const double dH = st * da + ct * db;
  const double dst = h ? ih * (da - st * dH) : 0.0, dct = h ? ih * (db - ct * dH) : 0.0;
  const double zz = z.v + kEp2 * kRb * (st * st * st), pp = p - kE2 * kRa * (ct * ct * ct);
  const double dzz = z.d + 3.0 * kEp2 * kRb * (st * st) * dst, dpp = dp - 3.0 * kE2 * kRa * (ct * ct) * dct;
  const double dlat = (pp * dzz - zz * dpp) * (ihy * ihy);
  const double dlon = (x.v * y.d - y.v * x.d) * (ip * ip);
  const double dsl = cl * dlat, dcl = -sl * dlat;
  const double dN = N * N * N * (kE2 / (kRa * kRa)) * sl * dsl;
  const double icl = 1.0 / cl;
  lat = {latv, dlat};
  lon = {lonv, dlon};
  alt = {altv, (dp - p * icl * dcl) * icl - dN};
}

// iip_faa (gel_output_row.h) on duals: the (0, 0) fill returns zero tangents
GEL_DEV void iip_faa_dual(const Dual pe[3], const Dual ve[3], Dual& lat_deg, Dual& lon_deg) {
  const double a = 6378137.0, f = 1.0 / 298.257223563, b = a * (1.0 - f), e2 = 2.0 * f - f * f;
  lat_deg = {0.0, 0.0}; lon_deg = {0.0, 0.0};
  Dual r_k1 = {b, 0.0};
  const Dual r0 = dsqrt(pe[0] * pe[0] + pe[1] * pe[1] + pe[2] * pe[2]);
  if (r0.v < r_k1.v) return;                                        // below the surface
  const Dual vi[3] = {ve[0] - kOmega * pe[1], ve[1] + kOmega * pe[0], ve[2]};
  const Dual v0 = dsqrt(vi[0] * vi[0] + vi[1] * vi[1] + vi[2] * vi[2]);
  const Dual eps_cos = (r0 * (v0 * v0) / kMu) - 1.0;
  if (eps_cos.v >= 1.0) return;                                     // not elliptical
  const Dual a_t = r0 / (1.0 - eps_cos);
  const Dual eps_sin = (pe[0] * vi[0] + pe[1] * vi[1] + pe[2] * vi[2]) / dsqrt(kMu * a_t);
  const Dual eps2 = eps_cos * eps_cos + eps_sin * eps_sin;
  const Dual se2 = dsqrt(eps2);
  if (se2.v <= 1.0 && (a_t * (1.0 - se2) - a).v >= 0.0) return;     // positive perigee height
  Dual Ek = {0.0, 0.0}, Fk = Ek, Gk = Ek, r_k2 = Ek, r_prev = Ek, eps_k_sin = Ek, dcos = Ek, dsin = Ek;
  const Dual root = dsqrt((a_t * a_t * a_t) / kMu);
  for (int it = 0; it < 5; it++) {
    const Dual eps_k_cos = (a_t - r_k1) / a_t;
    const Dual w = eps2 - eps_k_cos * eps_k_cos;
    if (w.v < 0.0) return;                                          // no intersection with the surface
    eps_k_sin = -dsqrt(w);
    dcos = (eps_k_cos * eps_cos + eps_k_sin * eps_sin) / eps2;
    dsin = (eps_k_sin * eps_cos - eps_k_cos * eps_sin) / eps2;
    const Dual fs = (dcos - eps_cos) / (1.0 - eps_cos);
    const Dual gs = (dsin + eps_sin - eps_k_sin) * root;
    Ek = fs * pe[0] + gs * vi[0]; Fk = fs * pe[1] + gs * vi[1]; Gk = fs * pe[2] + gs * vi[2];
    const Dual q = Gk / r_k1;
    r_k2 = a / dsqrt((e2 / (1.0 - e2)) * (q * q) + 1.0);
    r_prev = r_k1;
    r_k1 = r_k2;
  }
  if (fabs(r_prev.v - r_k2.v) > 1.0) return;                        // not converged
  const Dual delta = datan2(dsin, dcos);
  const Dual time_sec = (delta + eps_sin - eps_k_sin) * root;
  const Dual phi = datan2(dtan(dasin(Gk / r_k2)), Dual{1.0 - e2, 0.0});
  const Dual lam = datan2(Fk, Ek) - kOmega * time_sec;
  lat_deg = phi * 180.0 / kPi;
  lon_deg = lam * 180.0 / kPi;
}

// distance_vincenty (gel_output_row.h) from a fixed origin to a dual target; the loop runs on the value part
GEL_DEV Dual distance_vincenty_dual(double lat_o, double lon_o, Dual lat_t, Dual lon_t) {
  const double Ra = 6378137.0, f = 1.0 / 298.257223563, Rb = Ra * (1.0 - f);
  const double lat1 = lat_o * kPi / 180.0, lon1 = lon_o * kPi / 180.0;
  const Dual lat2 = lat_t * kPi / 180.0, lon2 = lon_t * kPi / 180.0;
  if (lon2.v - lon1 == 0.0) return {0.0, 0.0};
  const double U1 = atan((1.0 - f) * tan(lat1));
  const Dual U2 = datan((1.0 - f) * dtan(lat2)), dl = lon2 - lon1;
  const double sU1 = sin(U1), cU1 = cos(U1);
  const Dual sU2 = dsin(U2), cU2 = dcos(U2);
  Dual lam = dl, sin_sigma = {0.0, 0.0}, cos_sigma = sin_sigma, sigma = sin_sigma, cos_alpha = sin_sigma, cos_2sm = sin_sigma;
  for (int it = 0; it < 5000; it++) {
    Dual sl, cl;
    dsincos(lam, sl, cl);
    const Dual t1 = cU2 * sl, t2 = cU1 * sU2 - sU1 * cU2 * cl;
    sin_sigma = dsqrt(t1 * t1 + t2 * t2);
    cos_sigma = sU1 * sU2 + cU1 * cU2 * cl;
    sigma = datan2(sin_sigma, cos_sigma);
    const Dual sin_alpha = cU1 * cU2 * sl / sin_sigma;
    cos_alpha = dsqrt(1.0 - sin_alpha * sin_alpha);
    cos_2sm = cos_sigma - 2.0 * sU1 * sU2 / (cos_alpha * cos_alpha);
    const Dual ca2 = cos_alpha * cos_alpha;
    const Dual coeff = f / 16.0 * ca2 * (4.0 + f * (4.0 - 3.0 * ca2));
    const double prev = lam.v;
    lam = dl + (1.0 - coeff) * f * sin_alpha * (sigma + coeff * sin_sigma * (cos_2sm + coeff * cos_sigma * (-1.0 + 2.0 * cos_2sm)));
    if (fabs(lam.v - prev) < 1e-12) break;
  }
  const Dual u2 = (cos_alpha * cos_alpha) * (Ra * Ra - Rb * Rb) / (Rb * Rb);
  const Dual A = 1.0 + u2 / 16384.0 * (4096.0 + u2 * (-768.0 + u2 * (320.0 - 175.0 * u2)));
  const Dual Bc = u2 / 1024.0 * (256.0 + u2 * (-128.0 + u2 * (74.0 - 47.0 * u2)));
  const Dual ds = Bc * sin_sigma * (cos_2sm + 0.25 * Bc * (cos_sigma * (-1.0 + 2.0 * (cos_2sm * cos_2sm)) -
                  (1.0 / 6.0) * Bc * cos_2sm * (-3.0 + 4.0 * (sin_sigma * sin_sigma)) * (-3.0 + 4.0 * (cos_2sm * cos_2sm))));
  return Rb * A * (sigma - ds);
}

// node_fn (gel_rows_body.h) on duals: functions 0 .. 15 of one knot state
GEL_DEV Dual node_fn_dual(int fn, const Dual r[3], const Dual v[3], Dual t, const double* p) {
  if (fn >= 9) {
    Dual sn, cs;
    dsincos(kOmega * t, sn, cs);
    const Dual pe[3] = {r[0] * cs + r[1] * sn, -r[0] * sn + r[1] * cs, r[2]};   // eci2ecef
    if (fn <= 11 || fn == 15) {
      Dual lat, lon, alt;
      geodetic_full_dual(pe[0], pe[1], pe[2], lat, lon, alt);
      if (fn == 15) return distance_vincenty_dual(p[2], p[3], lat * (180.0 / kPi), lon * (180.0 / kPi));
      return (fn == 9) ? lat * (180.0 / kPi) : (fn == 10) ? lon * (180.0 / kPi) : alt;
    }
    if (fn <= 13) {
      const Dual d0 = v[0] + kOmega * r[1], d1 = v[1] - kOmega * r[0];           // vel_eci2ecef
      const Dual ve[3] = {d0 * cs + d1 * sn, -d0 * sn + d1 * cs, v[2]};
      Dual la, lo;
      iip_faa_dual(pe, ve, la, lo);
      return (fn == 12) ? la : lo;
    }
    const Dual d[3] = {pe[0] - p[2], pe[1] - p[3], pe[2] - p[4]};
    const Dual dn = dsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    return (d[0] / dn) * p[5] + (d[1] / dn) * p[6] + (d[2] / dn) * p[7];
  }
  const Dual rn = dsqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  const Dual vn = dsqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (fn == 0) return 0.5 * vn * vn - kMu / rn;
  if (fn == 7) return rn;
  if (fn == 8) return vn;
  const Dual c[3] = {r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]};   // r x v
  const Dual c2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  if (fn == 1) return dsqrt(c2);
  if (fn == 2) return dacos(c[2] / dsqrt(c2));
  const Dual f[3] = {v[1] * c[2] - v[2] * c[1] - kMu * (r[0] / rn), v[2] * c[0] - v[0] * c[2] - kMu * (r[1] / rn),
                     v[0] * c[1] - v[1] * c[0] - kMu * (r[2] / rn)};          // Laplace vector v x c - mu r / |r|
  const Dual e = dsqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]) / kMu;
  if (fn == 4) return e;
  const Dual a = (c2 / kMu) / (1.0 - e * e);
  if (fn == 3) return a;
  return (fn == 5) ? a * (1.0 - e) : a * (1.0 + e);
}

}  // namespace gel
