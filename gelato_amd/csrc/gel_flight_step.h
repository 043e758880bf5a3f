// gel_flight_step.h -- what the flight kernels share on the device (prop_kernel, proptan_kernel, propadj_kernel; DESIGN.md 3.14,
// 3.20 - 3.23), each written once: the small helpers, a phase's set-up and dispersion factors, a stage's
// coefficients and control samples.  THE STEP of gel_prop.h is written out in each kernel on these pieces.
#pragma once
#include "gel_physics.h"
#include "gel_prop.h"

namespace gel {

GEL_DEV bool nonfinite(double v) { return !(__builtin_fabs(v) <= 1.79769313486231570815e308); }
// running maximum that keeps a NaN once it has seen one (fmax would drop it)
GEL_DEV double nan_max(double acc, double v) { return (v > acc || v != v) ? v : acc; }
// component c of state row xi of a packed vector (x, or y: the same layout)
GEL_DEV size_t state_index(int M, int xi, int c) {
  return (c == 0) ? (size_t)xi : (c < 4) ? (size_t)M + 3 * (size_t)xi + (c - 1) : (c < 7) ? 4 * (size_t)M + 3 * (size_t)xi + (c - 4)
                                                                                      : 7 * (size_t)M + 4 * (size_t)xi + (c - 7);
}
// the first and the last argument of a kernel's trailing pack (an EnsDev, then the wind seed or gradient)
template <typename A, typename... R>
GEL_DEV const A& pack_first(const A& a, const R&...) { return a; }
template <typename A>
GEL_DEV const A& pack_last(const A& a) { return a; }
template <typename A, typename B, typename... R>
GEL_DEV const auto& pack_last(const A&, const B& b, const R&... r) { return pack_last(b, r...); }

// One phase as a lane flies it (xb: the lane's decision vector).  n, k, sampled and the offsets are wave-uniform (load_const).
struct FlightPhase {
  PhaseDev ph;
  int n, k, sampled;        // collocation nodes, RK4 steps per node interval, the phase has control samples
  const double *sig, *hs;   // the stage points [2 k n + 1]; the step of every node interval [n]
  size_t pt0;               // first stage point of the phase in the workspace's rows
  double to, tf, S, fw;     // the knot times, S = (tf - to) * unit_t / 2.0, the wind factor: 1.0 until apply_factors()
};
GEL_DEV FlightPhase load_flight_phase(const ProblemDev& P, const PropDev& Pd, int s, const double* xb) {
  FlightPhase f;
  f.ph = load_phase(P.phases + s);
  f.n = load_const(&Pd.ph[s].n);
  f.k = load_const(&Pd.ph[s].k);
  f.sampled = load_const(&Pd.ph[s].sampled);
  f.sig = Pd.mat + load_const(&Pd.ph[s].sg);
  f.hs = Pd.mat + load_const(&Pd.ph[s].hs);
  f.pt0 = (size_t)load_const(&Pd.ph[s].pt0);
  f.to = xb[11 * P.M + 2 * P.N + s];
  f.tf = xb[11 * P.M + 2 * P.N + s + 1];
  f.S = (f.tf - f.to) * P.ut / 2.0;
  f.fw = 1.0;
  return f;
}

// The factors fac [kPropNDisp] of the lane's (vector, phase): thrust, mass flow and reference area scale the record, one product
// each; the fourth becomes fw.  Until this runs the record holds the handle's unscaled values, which the tangent reads first.
GEL_DEV void apply_factors(FlightPhase& f, const double* fac) {
  const double f_thrust = fac[0], f_mf = fac[1], f_area = fac[2];
  f.fw = fac[3];
  f.ph.thrust = f.ph.thrust * f_thrust;
  f.ph.mf_um = f.ph.mf_um * f_mf;
  f.ph.area = f.ph.area * f_area;
}

// Stage st = 0 .. 3 of the step whose first stage point is p: its stage point (p, p + 1, p + 1, p + 2), the a of
// yt = fma(a, F_prev, y) and the weight w of acc = fma(w, F, acc)
struct Stage { int pp; double a, w; };
GEL_DEV Stage rk4_stage(int p, int st, double Sh, double Sh2) { return {p + ((st + 1) >> 1), (st == 3) ? Sh : Sh2, (st == 3) ? 1.0 : 2.0}; }

// The control samples of stage point pp (us: the lane's column of the phase's workspace rows [stage point][2][ld]); zero without
GEL_DEV void stage_controls(const double* us, size_t ld, int sampled, int pp, double& u0, double& u1) {
  u0 = u1 = 0.0;
  if (sampled) {
    u0 = us[(size_t)pp * 2 * ld];
    u1 = us[((size_t)pp * 2 + 1) * ld];
  }
}

}  // namespace gel
