// gel_rows_body.h -- the knot / terminal / user rows as a device function of a (virtual) workgroup index: node_fn and rows_body, which
// rows_kernel (gel_kernels_rows.hip) and callback_kernel (gel_kernels.hip) run.
#pragma once
#include "gel_tables.h"
#include "gel_output_row.h"

namespace gel {

// ---------------------------------------------------------------------------
// Knot / terminal / user rows.
//
// Linear rows: (coef0 x[idx0] + coef1 x[idx1]) + c0 -- equality_init, equality_time, inequality_time and
// equality_knot_LGR (lib/con_init_terminal_knot.py:39-52,118-141,174-252,422-436) are differences of single decision
// variables plus a constant; with coefficients +-1 the expression rounds exactly like the reference's
// (a - b) - c.  Their Jacobians are the coefficients (constant COO, laid out by the caller).
//
// Node-function rows: g = f(r, v) / p0 - p1 at ONE state node, r = position * unit, v = velocity * unit, and the forward
// difference (g(x + dx e_c) - g(x)) / dx over exactly the six columns the row can see (lib/con_init_terminal_knot.py:
// 378-405 perturbs the last node's six columns; lib/jac_fd.py:29-62 perturbs every column of x, and every column but
// these six returns an exact zero).  Eight lanes per row: lane 0 the centre, lanes 1..6 one perturbed state column each,
// lane 7 the knot time of rows that read it (the waypoint rows of lib/con_waypoint.py), formed in the kernel -- no
// perturbed copies of x exist anywhere.  Functions: see node_fn(); iip_faa and distance_vincenty, which the output table's row
// shares, are in gel_output_row.h.
// ---------------------------------------------------------------------------
// functions of ONE knot state (r, v in SI units, t in seconds, row parameters p):
//   0 orbit energy (src/wrapper_coordinate.hpp:246-250)   1 |angular momentum| (:222-228)   2 inclination [rad] (:229-236)
//   3 a   4 e   5 a (1 - e)   6 a (1 + e)   (src/Coordinate.cpp:197-245)   7 |r|   8 |v|
//   9 / 10 / 11 geodetic latitude [deg] / longitude [deg] / altitude [m] of the ECEF position at time t
//       (eci2geodetic, lib/coordinate.py; lib/con_waypoint.py:507-560)
//   12 / 13 latitude / longitude [deg] of the instantaneous impact point (lib/con_waypoint.py:164-207, lib/IIP.py)
//   14 sine of the elevation above an antenna's horizon, p[2..4] = antenna ECEF, p[5..7] = its local vertical
//       (lib/con_waypoint.py:45-51)
//   15 downrange [m]: Vincenty distance from the launch point p[2] = latitude, p[3] = longitude [deg] to the geodetic
//       latitude / longitude of the position (lib/con_waypoint.py:531-534,590-598; lib/downrange.py:32-111)
GEL_DEV double node_fn(int fn, const double r[3], const double v[3], double t, const double* p) {
  if (fn >= 9) {
    double sn, cs;
    sincos(kOmega * t, &sn, &cs);
    const double pe[3] = {r[0] * cs + r[1] * sn, -r[0] * sn + r[1] * cs, r[2]};      // eci2ecef (src/Coordinate.cpp:51-59)
    if (fn <= 11) {
      double lat, lon, alt;
      geodetic_full(pe[0], pe[1], pe[2], lat, lon, alt);
      return (fn == 9) ? lat * (180.0 / kPi) : (fn == 10) ? lon * (180.0 / kPi) : alt;   // math.degrees
    }
    if (fn == 15) {
      double lat, lon, alt;
      geodetic_full(pe[0], pe[1], pe[2], lat, lon, alt);
      return distance_vincenty(p[2], p[3], lat * (180.0 / kPi), lon * (180.0 / kPi));
    }
    if (fn <= 13) {
      const double d0 = v[0] + kOmega * r[1], d1 = v[1] - kOmega * r[0];             // vel_eci2ecef (:69-73)
      const double ve[3] = {d0 * cs + d1 * sn, -d0 * sn + d1 * cs, v[2]};
      double la, lo;
      iip_faa(pe, ve, la, lo);
      return (fn == 12) ? la : lo;
    }
    const double d[3] = {pe[0] - p[2], pe[1] - p[3], pe[2] - p[4]};
    const double dn = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    return (d[0] / dn) * p[5] + (d[1] / dn) * p[6] + (d[2] / dn) * p[7];
  }
  const double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (fn == 0) return 0.5 * vn * vn - kMu / rn;
  if (fn == 7) return rn;
  if (fn == 8) return vn;
  const double c[3] = {r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]};  // r x v
  const double c2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  if (fn == 1) return sqrt(c2);
  if (fn == 2) return acos(c[2] / sqrt(c2));
  // Laplace vector f = v x c - mu r/|r|
  const double f[3] = {v[1] * c[2] - v[2] * c[1] - kMu * (r[0] / rn), v[2] * c[0] - v[0] * c[2] - kMu * (r[1] / rn),
                       v[0] * c[1] - v[1] * c[0] - kMu * (r[2] / rn)};
  const double e = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]) / kMu;
  if (fn == 4) return e;
  const double a = (c2 / kMu) / (1.0 - e * e);
  if (fn == 3) return a;
  return (fn == 5) ? a * (1.0 - e) : a * (1.0 + e);
}

__device__ __forceinline__ void rows_body(const ProblemDev P, int nlin, const LinRowDev* __restrict__ lin, int nfn,
                                          const FnRowDev* __restrict__ fr, int B, int lin_blocks, const double* __restrict__ x,
                                          double* __restrict__ con, double* __restrict__ jfn, const unsigned vblk) {
  const int R = nlin + nfn;
  double chk = 0.0;
  if ((int)vblk < lin_blocks) {
    const long long t = (long long)vblk * blockDim.x + threadIdx.x;
    if (t >= (long long)B * nlin) return;
    const int b = (int)(t / nlin), r = (int)(t - (long long)b * nlin);
    const LinRowDev L = lin[r];
    const double* xb = x + (size_t)b * P.nvars;
    double s = L.coef0 * xb[L.idx0];
    if (L.idx1 >= 0) s += L.coef1 * xb[L.idx1];
    chk = con[(size_t)b * R + r] = s + L.c0;
  } else {
    const long long t = (long long)(vblk - lin_blocks) * blockDim.x + threadIdx.x;
    const long long grp = t >> 3;
    const int sw = (int)(t & 7);                       // 0 centre, 1..3 position xyz + dx, 4..6 velocity xyz + dx, 7 knot time + dx
    const bool live = grp < (long long)B * nfn;
    const long long g2 = live ? grp : 0;
    const int b = (int)(g2 / nfn), row = (int)(g2 - (long long)b * nfn);
    const FnRowDev F = fr[row];
    const double* xb = x + (size_t)b * P.nvars;
    double r[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      // xdict[key][j] += dx, then * unit (con_init_terminal_knot.py:340-341,392-394; con_waypoint.py:219-232,565-577)
      const double pe = xb[P.M + 3 * F.node + c], ve = xb[4 * P.M + 3 * F.node + c];
      r[c] = ((sw == 1 + c) ? pe + P.dx : pe) * P.up;
      v[c] = ((sw == 4 + c) ? ve + P.dx : ve) * P.uv;
    }
    double tk = 0.0;
    if (F.tcol >= 0) {
      const double te = xb[11 * P.M + 2 * P.N + F.tcol];
      tk = ((sw == 7) ? te + P.dx : te) * P.ut;
    }
    const double f = node_fn(F.fn, r, v, tk, F.p);
    const int vm = F.mode & 3;
    double g = (vm == 0) ? f / F.p[0] - F.p[1] : (f - F.p[1]) / F.p[0];
    if (F.mode & 8) g = -g;
    const int lane0 = (int)(threadIdx.x & 63 & ~7);
    const double gc = __shfl(g, lane0, 64), fc = __shfl(f, lane0, 64);   // the centre values of this row's lane group
    if (!live) return;
    if (sw == 0) chk = con[(size_t)b * R + nlin + row] = g;
    else if (jfn) {
      double d;
      if (F.mode & 4) { d = ((f - fc) / P.dx) / F.p[0]; if (F.mode & 8) d = -d; }   // the reference scales the raw difference
      else d = (g - gc) / P.dx;                                                       // difference of the row's own value
      chk = jfn[((size_t)b * nfn + row) * 7 + (sw - 1)] = d;
    }
  }
  if (!(fabs(chk) <= 1.79769313486231570815e308)) *(volatile int32_t*)P.flag = 1;  // every writer stores the same 1
}

}  // namespace gel
