// gel_section_rhs.h -- the right-hand side F(sigma, X, U) that a phase's defect rows impose, at an arbitrary point of the section:
// what the collocation error estimate (gel_kernels_mesh.hip) integrates with the fine grid's matrix and what the explicit
// propagation (gel_kernels_prop.hip) integrates with RK4.  One device function, so that the two evaluate the same expression.
#pragma once
#include "gel_tables.h"

namespace gel {

// xt [11]: mass | position 3 | velocity 3 | quaternion 4 in x's normalised units; u0, u1: the controls (ignored by a hold phase);
// sig: the point in [-1, 1]; to, tf: the phase's normalised knot times; vp = unit_velocity / unit_position.
//   mass        mf_um with the engine on, else 0
//   position    X_vel vp
//   velocity    dynamics_velocity (reference_area != 0) at the normalised time sig (tf - to)/2 + (tf + to)/2, or _NoAir
//   quaternion  quat_rate, or 0 for a held attitude
// The caller keeps idle lanes out: wind_eci_or_calm takes a vote of the lanes that are here.  (All of F, the mass and position
// rows included, is therefore formed for active lanes only; the callers store and read F only there.)
// kDisp (gel_propagate_dispersed): the caller has already scaled ph.thrust, ph.mf_um and ph.area by its lane's factors (one product
// each, once per phase); fw scales the two wind components AFTER the interpolation -- the tables in LDS are the workgroup's --
// and before wind_eci_or_calm.  ph.air stays the handle's.  Without kDisp fw is not read: the code is what it was.
// kEns (gel_propagate_ensemble*, with kDisp): tb is the LANE's view of the tables (ens_lane_tables, gel_ensemble.h: its wind part
// lies in global memory) and wbr the lane's kept altitude interval of that table, carried by the caller across stages and steps:
// wind_ned2_cached gives wind_ned2's bits from it and searches again on a miss.  Without kEns wbr is not read.
template <bool kDisp = false, bool kEns = false>
GEL_DEV void section_rhs(const ProblemDev& P, const PhaseDev& ph, const Tables& tb, double vp, double sig, double to, double tf,
                         const double xt[11], double u0, double u1, double F[11], double fw = 1.0, Bracket2* wbr = nullptr) {
  F[0] = ph.engine_on ? ph.mf_um : 0.0;   // mass: the m[1:] - m[0] form when the engine is off
#pragma unroll
  for (int c = 0; c < 3; c++) F[1 + c] = xt[4 + c] * vp;
  const double m = xt[0] * P.um;
  const double r[3] = {xt[1] * P.up, xt[2] * P.up, xt[3] * P.up};
  const double q[4] = {xt[7], xt[8], xt[9], xt[10]};
  double dir[3], f[3];
  thrust_dir(q, dir);
  if (ph.air) {
    // dynamics_velocity at the normalised time of the point (PSparams.time_nodes, as the defect kernels take it)
    const double v3[3] = {xt[4] * P.uv, xt[5] * P.uv, xt[6] * P.uv};
    const PosPart pp = pos_part(r, tb, P.barC20, kEns ? wbr : nullptr);
    const EarthAngle ea = earth_angle(sig * (tf - to) / 2 + (tf + to) / 2);
    double w[3], Fa[3];
    if constexpr (kDisp) {
      const double wn = pp.wn * fw, we = pp.we * fw;
      wind_eci_or_calm(r, ea, pp.sl, pp.cl, pp.inv_p, wn, we, w);
    } else {
      wind_eci_or_calm(r, ea, pp.sl, pp.cl, pp.inv_p, pp.wn, pp.we, w);
    }
    aero_force(r, v3, pp.rho, pp.inv_a, w, ph.area, tb, Fa);
    const double T = ph.thrust - ph.nozzle * pp.P;
    const double Td[3] = {T * dir[0], T * dir[1], T * dir[2]};
    accel(Td, Fa, 1.0 / m, pp.g, P.inv_uv, f);
  } else {
    double g[3];
    gravity_eci(r, P.barC20, g);
    const double Td[3] = {ph.thrust * dir[0], ph.thrust * dir[1], ph.thrust * dir[2]};
    accel_noair(Td, 1.0 / m, g, P.inv_uv, f);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) F[4 + c] = f[c];
  double dq[4] = {0.0, 0.0, 0.0, 0.0};
  if (!ph.hold) quat_rate(q, u0, u1, P.uu, dq);
#pragma unroll
  for (int c = 0; c < 4; c++) F[7 + c] = dq[c];
}

}  // namespace gel
