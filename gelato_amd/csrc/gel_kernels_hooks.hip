// gel_kernels_hooks.hip -- the test hooks: the node-batched right-hand sides (rhs_vel_air_kernel, rhs_vel_noair_kernel,
// rhs_quat_kernel: gel_dynamics_velocity / gel_dynamics_quaternion) and the point functions (point_kernel: gel_point_eval), which
// put single device functions of the hot path beside the reference's or the library's.
#include "gel_tables.h"

namespace gel {

// ---------------------------------------------------------------------------
// node-batched RHS hooks (dynamics_c replacements, src/pybind_dynamics.cpp:30-106)
// ---------------------------------------------------------------------------
struct RhsArgs {
  int n, Kw, Kc;
  const double *mass_e, *pos_e, *vel_e, *quat, *t, *tables;
  double thrust, area, nozzle, um, up, uv, barC20;
  double* out;
};

__global__ void rhs_vel_air_kernel(RhsArgs A) {
  extern __shared__ double lds[];
  ProblemDev P{};
  P.Kw = A.Kw; P.Kc = A.Kc; P.tables = A.tables;
  const Tables tb = stage_tables(P, lds);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const double m = A.mass_e[i] * A.um;
  const double r[3] = {A.pos_e[3 * i] * A.up, A.pos_e[3 * i + 1] * A.up, A.pos_e[3 * i + 2] * A.up};
  const double v[3] = {A.vel_e[3 * i] * A.uv, A.vel_e[3 * i + 1] * A.uv, A.vel_e[3 * i + 2] * A.uv};
  const double q[4] = {A.quat[4 * i], A.quat[4 * i + 1], A.quat[4 * i + 2], A.quat[4 * i + 3]};
  const PosPart pp = pos_part(r, tb, A.barC20);
  const EarthAngle ea = earth_angle(A.t[i]);
  double w[3], F[3], dir[3], f[3];
  wind_eci(r, ea, pp.sl, pp.cl, pp.inv_p, pp.wn, pp.we, w);
  aero_force(r, v, pp.rho, pp.inv_a, w, A.area, tb, F);
  thrust_dir(q, dir);
  const double T = A.thrust - A.nozzle * pp.P;
  const double Td[3] = {T * dir[0], T * dir[1], T * dir[2]};
  accel(Td, F, 1.0 / m, pp.g, 1.0 / A.uv, f);
  for (int c = 0; c < 3; c++) A.out[3 * i + c] = f[c];
}

__global__ void rhs_vel_noair_kernel(RhsArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const double m = A.mass_e[i] * A.um;
  const double r[3] = {A.pos_e[3 * i] * A.up, A.pos_e[3 * i + 1] * A.up, A.pos_e[3 * i + 2] * A.up};
  const double q[4] = {A.quat[4 * i], A.quat[4 * i + 1], A.quat[4 * i + 2], A.quat[4 * i + 3]};
  double dir[3], g[3], f[3];
  thrust_dir(q, dir);
  gravity_eci(r, A.barC20, g);
  const double Td[3] = {A.thrust * dir[0], A.thrust * dir[1], A.thrust * dir[2]};
  accel_noair(Td, 1.0 / m, g, 1.0 / A.uv, f);
  for (int c = 0; c < 3; c++) A.out[3 * i + c] = f[c];
}

__global__ void rhs_quat_kernel(int n, const double* quat, const double* u_e, double unit_u, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double q[4] = {quat[4 * i], quat[4 * i + 1], quat[4 * i + 2], quat[4 * i + 3]};
  double dq[4];
  quat_rate(q, u_e[2 * i], u_e[2 * i + 1], unit_u, dq);
  for (int c = 0; c < 4; c++) out[4 * i + c] = dq[c];
}

__global__ void point_kernel(int kind, int n, const double* in, const double* aux, int aux_rows, double* out) {
  extern __shared__ double lds[];
  // aux table (wind [K][3] or generic [K][2]) and the atmosphere table are staged in LDS
  // kinds 5 / 6: rows followed by the per-interval slopes (built by the host entry point)
  const int naux = (kind == 5 || kind == 10) ? 3 * aux_rows + 2 * (aux_rows - 1)
                   : (kind == 6 || kind == 9) ? 2 * aux_rows + (aux_rows - 1)
                   : (kind == 15 || kind == 16) ? kAtmDoubles + 3 * aux_rows + 2 * (aux_rows - 1) : (kind == 0 ? kAtmDoubles : 0);
  for (int i = threadIdx.x; i < naux; i += blockDim.x) lds[i] = aux[i];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  switch (kind) {
    case 0: {
      const double h = geopotential_altitude(in[i]);
      const Air a = atmosphere(h, lds);
      out[5 * i] = h; out[5 * i + 1] = a.T; out[5 * i + 2] = a.P; out[5 * i + 3] = a.rho; out[5 * i + 4] = a.a;
    } break;
    case 1: {
      // latitude / longitude in degrees (atan2, as the reference reports them); the altitude exactly as pos_part forms it
      // (from the algebraic sine / cosine pair of the latitude)
      double lat, sl, cl, p, ip;
      geodetic_lat_p(in[3 * i], in[3 * i + 1], in[3 * i + 2], lat, p, ip);
      geodetic_sincos_p(in[3 * i], in[3 * i + 1], in[3 * i + 2], sl, cl, p, ip);
      const double lon = atan2(in[3 * i + 1], in[3 * i]);
      out[3 * i] = lat * 180.0 / kPi; out[3 * i + 1] = lon * 180.0 / kPi;
      out[3 * i + 2] = geodetic_alt_from(p, sl, cl);
    } break;
    case 2: {
      const double r[3] = {in[3 * i], in[3 * i + 1], in[3 * i + 2]};
      double g[3];
      gravity_eci(r, aux[0], g);
      out[3 * i] = g[0]; out[3 * i + 1] = g[1]; out[3 * i + 2] = g[2];
    } break;
    case 3: {
      // wind vector NED -> ECI exactly as the hot path does it: in = pos[3], t, wn, we
      const double* a = in + 6 * i;
      const double r[3] = {a[0], a[1], a[2]};
      double sl, cl, p, ip, w[3];
      geodetic_sincos_p(r[0], r[1], r[2], sl, cl, p, ip);
      const EarthAngle ea = earth_angle(a[3]);
      wind_eci(r, ea, sl, cl, ip, a[4], a[5], w);
      out[3 * i] = w[0]; out[3 * i + 1] = w[1]; out[3 * i + 2] = w[2];
    } break;
    case 4: {
      const double* a = in + 7 * i;  // vel[3], pos[3], t
      double s, c;
      sincos(kOmega * a[6], &s, &c);
      const double d0 = a[0] - (0.0 * a[5] - kOmega * a[4]);
      const double d1 = a[1] - (kOmega * a[3] - 0.0 * a[5]);
      const double d2 = a[2] - (0.0 * a[4] - 0.0 * a[3]);
      out[3 * i] = d0 * c + d1 * s; out[3 * i + 1] = -d0 * s + d1 * c; out[3 * i + 2] = d2;
    } break;
    case 5: {
      double wn, we;
      wind_ned2(in[i], lds, lds + 3 * aux_rows, aux_rows, wn, we);
      out[3 * i] = wn; out[3 * i + 1] = we; out[3 * i + 2] = 0.0;
    } break;
    case 6: out[i] = interp_tab(in[i], lds, lds + 2 * aux_rows, aux_rows, 2, 1); break;
    case 7: {  // the path's guard-free sqrt / division beside the compiler's, for the bit-identity test
      const double a = in[2 * i], b = in[2 * i + 1];
      out[4 * i] = fsqrt(a); out[4 * i + 1] = sqrt(a); out[4 * i + 2] = fdiv(a, b); out[4 * i + 3] = a / b;
    } break;
    case 8: {  // the path's sincos / log beside the library's, for the accuracy test
      double s1, c1, s2, c2;
      fsincos(in[2 * i], &s1, &c1);
      sincos(in[2 * i], &s2, &c2);
      out[6 * i] = s1; out[6 * i + 1] = c1; out[6 * i + 2] = s2; out[6 * i + 3] = c2;
      out[6 * i + 4] = flog_ratio(in[2 * i + 1]); out[6 * i + 5] = log(in[2 * i + 1]);
    } break;
    case 9: {  // eight lookups in a row through the interval kept from the previous one (the fused kernel's CA lookups)
      Bracket br = no_bracket();
      for (int k = 0; k < 8; k++) out[8 * i + k] = interp_tab_cached(in[8 * i + k], lds, lds + 2 * aux_rows, aux_rows, 2, 1, br);
    } break;
    case 10: {  // likewise the wind lookups of a node's position evaluations
      Bracket2 br = no_bracket2();
      for (int k = 0; k < 8; k++) {
        double wn, we;
        wind_ned2_cached(in[8 * i + k], lds, lds + 3 * aux_rows, aux_rows, wn, we, br);
        out[16 * i + 2 * k] = wn; out[16 * i + 2 * k + 1] = we;
      }
    } break;
    case 11: {  // quatmult (src/wrapper_coordinate.hpp:50-57): in = q[4], p[4]
      double o[4];
      quatmult(in + 8 * i, in + 8 * i + 4, o);
      for (int c = 0; c < 4; c++) out[4 * i + c] = o[c];
    } break;
    case 12: {  // quatrot (:70-78) = vec(conj(q) (0, v) q): in = q[4], v[3]
      double o[3];
      quatrot(in + 7 * i, in + 7 * i + 4, o);
      for (int c = 0; c < 3; c++) out[3 * i + c] = o[c];
    } break;
    case 13: {  // conj (:59-61) and the thrust direction quatrot(conj(q), (1, 0, 0)) the hot path forms without the zero terms: in = q[4]
      const double* q = in + 4 * i;
      out[7 * i] = q[0]; out[7 * i + 1] = -q[1]; out[7 * i + 2] = -q[2]; out[7 * i + 3] = -q[3];
      double d[3];
      thrust_dir(q, d);
      for (int c = 0; c < 3; c++) out[7 * i + 4 + c] = d[c];
    } break;
    case 14: out[2 * i] = fexp(in[i]); out[2 * i + 1] = exp(in[i]); break;   // the path's exp beside the library's, for the bit-identity test
    case 15: {  // a position sweep in exact-difference form as the fused kernel chains it: in = r[3] (m), kk, dlt; the atmosphere table,
                // the wind rows and their slopes in LDS
      Tables tb;
      tb.atm = lds; tb.wind = lds + kAtmDoubles; tb.winds = tb.wind + 3 * aux_rows; tb.ca = nullptr; tb.cas = nullptr;
      tb.Kw = aux_rows; tb.Kc = 0;
      const double* a = in + 5 * i;
      const double r[3] = {a[0], a[1], a[2]};
      const int kk = min(max((int)a[3], 0), 2);
      PosCentre pc;
      PosCentreTail pt;
      PosPart pp = pos_part<true, PosCentreSink, false>(r, tb, 0.0, nullptr, PosCentreSink{&pc}, &pt);
      pos_centre_tail(pt, pp.rho, pp.P, tb, pc, pp.wn, pp.we);
      PosPart pq;
      double dlat;
      const bool ok = pos_delta(r, kk, a[4], pp, pc, tb, pq, &dlat);
      // the half-latitude pair of the centre and of the perturbed point, which the position part no longer carries (the wind takes
      // sin / cos of the latitude itself): formed here as pos_part() and pos_delta() used to
      double shp, chp, shq, chq;
      half_lat_pair(pp.sl, pp.cl, shp, chp);
      half_lat_step(shp, chp, dlat, shq, chq);
      double* o = out + 18 * i;
      o[0] = pp.rho; o[1] = pp.P; o[2] = pp.inv_a; o[3] = pp.wn; o[4] = pp.we; o[5] = shp; o[6] = chp; o[7] = pp.inv_p;
      o[8] = pq.rho; o[9] = pq.P; o[10] = pq.inv_a; o[11] = pq.wn; o[12] = pq.we; o[13] = shq; o[14] = chq; o[15] = pq.inv_p;
      o[16] = ok ? 1.0 : 0.0; o[17] = pc.margin;
    } break;
    case 16: {  // kind 15's 18 outputs for kk = 0, 1, 2 from ONE centre, chained as the fused kernel chains its three position sweeps:
                // 1/T and the margin taken once (pos_centre_tail) and kept, each sweep re-deriving only the wind slopes and the
                // centre's wind (pos_centre_tail_kept); in = r[3] (m), (unused), dlt; out = [kk][18]
      Tables tb;
      tb.atm = lds; tb.wind = lds + kAtmDoubles; tb.winds = tb.wind + 3 * aux_rows; tb.ca = nullptr; tb.cas = nullptr;
      tb.Kw = aux_rows; tb.Kc = 0;
      const double* a = in + 5 * i;
      const double r[3] = {a[0], a[1], a[2]};
      PosCentre pc0;
      PosCentreTail pt;
      const PosPart pp = pos_part<true, PosCentreSink, false>(r, tb, 0.0, nullptr, PosCentreSink{&pc0}, &pt);
      double iT, margin;
      {
        PosCentre pcx;
        double wn_, we_;
        pos_centre_tail(pt, pp.rho, pp.P, tb, pcx, wn_, we_);
        iT = pcx.air.iT; margin = pcx.margin;
      }
      double shp, chp;
      half_lat_pair(pp.sl, pp.cl, shp, chp);
#pragma unroll 1
      for (int kk = 0; kk < 3; kk++) {
        PosCentre pc = pc0;
        PosPart pcv = pp;
        pos_centre_tail_kept(pt, iT, margin, tb, pc, pcv.wn, pcv.we);
        PosPart pq;
        double dlat, shq, chq;
        const bool ok = pos_delta(r, kk, a[4], pcv, pc, tb, pq, &dlat);
        half_lat_step(shp, chp, dlat, shq, chq);
        double* o = out + 54 * i + 18 * kk;
        o[0] = pcv.rho; o[1] = pcv.P; o[2] = pcv.inv_a; o[3] = pcv.wn; o[4] = pcv.we; o[5] = shp; o[6] = chp; o[7] = pcv.inv_p;
        o[8] = pq.rho; o[9] = pq.P; o[10] = pq.inv_a; o[11] = pq.wn; o[12] = pq.we; o[13] = shq; o[14] = chq; o[15] = pq.inv_p;
        o[16] = ok ? 1.0 : 0.0; o[17] = pc.margin;
      }
    } break;
    default: break;
  }
}

hipError_t launch_rhs_vel(bool air, int n, const double* mass_e, const double* pos_e, const double* vel_e,
                          const double* quat, const double* t, const double* tables, int Kw, int Kc, double thrust,
                          double area, double nozzle, double um, double up, double uv, double barC20, double* out,
                          hipStream_t s) {
  RhsArgs A{n, Kw, Kc, mass_e, pos_e, vel_e, quat, t, tables, thrust, area, nozzle, um, up, uv, barC20, out};
  const unsigned grid = (n + 63) / 64;
  if (air)
    hipLaunchKernelGGL(rhs_vel_air_kernel, dim3(grid), dim3(64), table_lds_bytes(Kw, Kc), s, A);
  else
    hipLaunchKernelGGL(rhs_vel_noair_kernel, dim3(grid), dim3(64), 0, s, A);
  return hipGetLastError();
}

hipError_t launch_rhs_quat(int n, const double* quat, const double* u_e, double unit_u, double* out, hipStream_t s) {
  hipLaunchKernelGGL(rhs_quat_kernel, dim3((n + 63) / 64), dim3(64), 0, s, n, quat, u_e, unit_u, out);
  return hipGetLastError();
}

hipError_t launch_point(int kind, int n, const double* in, const double* aux, int aux_rows, double* out,
                        hipStream_t s) {
  const size_t lds = point_lds_bytes(aux_rows);
  hipLaunchKernelGGL(point_kernel, dim3((n + 63) / 64), dim3(64), lds, s, kind, n, in, aux, aux_rows, out);
  return hipGetLastError();
}

}  // namespace gel
