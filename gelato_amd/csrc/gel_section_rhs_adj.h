// gel_section_rhs_adj.h -- the right-hand side F of gel_section_rhs.h together with the TRANSPOSE of its tangent (gel_section_rhs_tan.h)
// applied to one multiplier lF [11], for the adjoint flight (gel_kernels_propadj.hip).
//
// Values: the lines of section_rhs_tangent, on the same arguments in the same order, so F has section_rhs<true>'s bits.  Partials:
// the ones section_rhs_tangent reads -- the air branch's from the same linearise_air (gel_section_rhs_lin.h), then dg, the quadratic
// thrust direction and the bilinear quaternion rate; every line of the tangent is transposed where it stands, the 3 x 3 blocks
// contracted from the other side (over the component instead of over the position direction).  aero_force_tangent() is linear in (da, drho, dinv_a): its
// transpose is WRITTEN OUT here (not probed with unit inputs), term by term:
//   dF_i = -(dk a_i + kk da_i)                 ->  l_dk = -<lFa, a>;  l_da_i = -kk lFa_i
//   dk   = area / 2 (drho ca s + rho cas dM s + rho ca ds)   (0 where |a| = 0)
//                                              ->  l_drho = h ca s;  l_dM = h rho cas s;  l_ds = h rho ca,   h = area / 2 l_dk
//   dM   = ds inv_a + s dinv_a                 ->  l_ds += inv_a l_dM;  l_dinv_a = s l_dM
//   ds   = <a, da> / s                         ->  l_da_i += (a_i / s) l_ds
// The time has no adjoint here: the tangent of F along the time is taken as zero (gel_section_rhs_tan.h).
//
// Out: lxt [11] = J^T lF in the units of the value call's state, and in RhsAdjoint the multipliers of the controls and of
// ph.thrust, ph.mf_um, ph.area AS THE VALUE CALL HOLDS THEM (the caller multiplies by the handle's unscaled values, as the tangent
// forms d.dthrust from them) and of the wind factor.
//
// kWind (gel_propagate_adjoint_wind*): also out, in gwd, the multipliers (fw lwn, fw lwe) of the seed the tangent's
// kWind lines look up, with the rows and the weight of that lookup (gel_wind_rows.h); the caller splits them between the rows.
// Not written in an air-less phase.  kWind = false forms none of this and is the function it was.
#pragma once
#include "gel_section_rhs_lin.h"
#include "gel_wind_rows.h"

namespace gel {

struct RhsAdjoint {
  double u0, u1;
  double thrust, mf, area, fw;
};
struct RhsWindAdjoint {
  WindRows rows;
  double wn, we;
};

template <bool kWind = false>
GEL_DEV void section_rhs_adjoint(const ProblemDev& P, const PhaseDev& ph, const Tables& tb, double vp, double sig, double to,
                                 double tf, const double xt[11], double u0, double u1, double fw, const double lF[11],
                                 double F[11], double lxt[11], RhsAdjoint& g, RhsWindAdjoint* gwd = nullptr) {
  F[0] = ph.engine_on ? ph.mf_um : 0.0;
  g.mf = ph.engine_on ? lF[0] : 0.0;
#pragma unroll
  for (int c = 0; c < 3; c++) F[1 + c] = xt[4 + c] * vp;
  const double m = xt[0] * P.um;
  const double r[3] = {xt[1] * P.up, xt[2] * P.up, xt[3] * P.up};
  const double q[4] = {xt[7], xt[8], xt[9], xt[10]};
  double dir[3], f[3];
  thrust_dir(q, dir);
  const double inv_m = 1.0 / m;
  double dg[3][3];
  gravity_tangent(r, P.barC20, dg);
  // df_c = (X_c / m - (tm_c / m) dm + dg_c) / uv:  mu = the bracket's multiplier, nu = X's
  const double mu[3] = {lF[4] * P.inv_uv, lF[5] * P.inv_uv, lF[6] * P.inv_uv};
  const double nu[3] = {mu[0] * inv_m, mu[1] * inv_m, mu[2] * inv_m};
  double ldr[3], ldir[3], lv[3] = {0.0, 0.0, 0.0}, ldm;
#pragma unroll
  for (int k = 0; k < 3; k++) ldr[k] = dg[k][0] * mu[0] + dg[k][1] * mu[1] + dg[k][2] * mu[2];
  g.area = 0.0;
  g.fw = 0.0;
  if (ph.air) {
    AirLinearisation L;
    linearise_air(P, ph, tb, sig, to, tf, xt, r, dir, inv_m, fw, L, f);
    // ---- the transpose ----
    // df_c: -(tm_c / m) dm
    ldm = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) ldm -= (((L.Td[c] + L.Fa[c]) * inv_m) * inv_m) * mu[c];
    // X_c = (dT dir_c + T ddir_c) + (dFa_c - dka a_c)
    const double lT = nu[0] * dir[0] + nu[1] * dir[1] + nu[2] * dir[2];
    const double na = nu[0] * L.a[0] + nu[1] * L.a[1] + nu[2] * L.a[2];
#pragma unroll
    for (int c = 0; c < 3; c++) ldir[c] = L.T * nu[c];
    // dka = rho darea ca s / 2;  dT = dthrust - nozzle dP dhd
    g.area = (L.s2 > 0.0) ? (0.5 * L.pp.rho * L.ca * L.s) * (-na) : 0.0;
    g.thrust = lT;
    double lhd = -(ph.nozzle * L.at.dP) * lT;
    // aero_force_tangent transposed (the head of this file); lFa = nu
    double lda[3] = {-L.kk * nu[0], -L.kk * nu[1], -L.kk * nu[2]};
    if (L.s2 > 0.0) {
      const double h = 0.5 * ph.area * (-na);
      const double lrho = h * (L.ca * L.s), lM = h * (L.pp.rho * L.cas * L.s);
      const double ls = h * (L.pp.rho * L.ca) + L.pp.inv_a * lM;
      const double linv_a = L.s * lM;
#pragma unroll
      for (int i = 0; i < 3; i++) lda[i] += (L.a[i] / L.s) * ls;
      // drho = at.drho dhd, dinv_a = at.dinv_a dhd
      lhd += L.at.drho * lrho + L.at.dinv_a * linv_a;
    }
    // da = (dv uv + Omega x dr) - dw
#pragma unroll
    for (int i = 0; i < 3; i++) lv[i] = P.uv * lda[i];
    ldr[1] += kOmega * lda[0];
    ldr[0] -= kOmega * lda[1];
    const double ldw[3] = {-lda[0], -lda[1], -lda[2]};
    // dw_i = sum_k dw3[k][i] dr_k + (dwn N_i + dwe E_i);  dhd = <dh, dr>
#pragma unroll
    for (int k = 0; k < 3; k++) ldr[k] += (L.dw3[k][0] * ldw[0] + L.dw3[k][1] * ldw[1] + L.dw3[k][2] * ldw[2]) + L.dh[k] * lhd;
    const double lwn = (-L.pc.sl * L.clon) * ldw[0] + (-L.pc.sl * L.slon) * ldw[1] + L.pc.cl * ldw[2];
    const double lwe = (-L.slon) * ldw[0] + L.clon * ldw[1];
    // dwn = wn dfw, dwe = we dfw with the interpolated (unscaled) wind
    g.fw = L.pp.wn * lwn + L.pp.we * lwe;
    if constexpr (kWind) {
      gwd->rows = wind_rows(L.tail.h, L.tail.piece, tb.wind, tb.Kw);
      gwd->wn = fw * lwn;
      gwd->we = fw * lwe;
    }
  } else {
    double gv[3];
    gravity_eci(r, P.barC20, gv);
    const double Td[3] = {ph.thrust * dir[0], ph.thrust * dir[1], ph.thrust * dir[2]};
    accel_noair(Td, inv_m, gv, P.inv_uv, f);
    ldm = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) ldm -= ((Td[c] * inv_m) * inv_m) * mu[c];
    g.thrust = nu[0] * dir[0] + nu[1] * dir[1] + nu[2] * dir[2];
#pragma unroll
    for (int c = 0; c < 3; c++) ldir[c] = ph.thrust * nu[c];
  }
#pragma unroll
  for (int c = 0; c < 3; c++) F[4 + c] = f[c];
  lxt[0] = ldm * P.um;
#pragma unroll
  for (int k = 0; k < 3; k++) lxt[1 + k] = ldr[k] * P.up;
#pragma unroll
  for (int c = 0; c < 3; c++) lxt[4 + c] = lF[1 + c] * vp + lv[c];
  // the thrust direction's quadratic form, transposed (ddir of section_rhs_tangent read by columns)
  double lq[4] = {2.0 * (q[0] * ldir[0] + q[3] * ldir[1] - q[2] * ldir[2]), 2.0 * (q[1] * ldir[0] + q[2] * ldir[1] + q[3] * ldir[2]),
                  2.0 * (q[1] * ldir[1] - q[2] * ldir[0] - q[0] * ldir[2]), 2.0 * (q[0] * ldir[1] - q[3] * ldir[0] + q[1] * ldir[2])};
  double fq[4] = {0.0, 0.0, 0.0, 0.0};
  g.u0 = g.u1 = 0.0;
  if (!ph.hold) {
    quat_rate(q, u0, u1, P.uu, fq);
    // bilinear in (q, u) (quat_rate()): the rate of dq under u read by columns, then the rate of q under du
    const double d2r = 0.017453292519943295769;
    const double oy = (u0 * P.uu) * d2r, oz = (u1 * P.uu) * d2r;
    const double l0 = lF[7], l1 = lF[8], l2 = lF[9], l3 = lF[10];
    lq[0] += 0.5 * (oy * l2 + oz * l3);
    lq[1] += 0.5 * (oy * l3 - oz * l2);
    lq[2] += 0.5 * (oz * l1 - oy * l0);
    lq[3] += 0.5 * (-oz * l0 - oy * l1);
    const double loy = 0.5 * (((q[0] * l2 + q[1] * l3) - q[2] * l0) - q[3] * l1);
    const double loz = 0.5 * (((q[0] * l3 + q[2] * l1) - q[1] * l2) - q[3] * l0);
    g.u0 = (loy * d2r) * P.uu;
    g.u1 = (loz * d2r) * P.uu;
  }
#pragma unroll
  for (int c = 0; c < 4; c++) { F[7 + c] = fq[c]; lxt[7 + c] = lq[c]; }
}

}  // namespace gel
