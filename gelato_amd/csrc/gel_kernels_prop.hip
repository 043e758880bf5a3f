// gel_kernels_prop.hip -- batched explicit propagation of the sections with classical RK4 (gel_propagate*): take
// the controls the optimiser found, integrate the equations of motion from a section's first state (or from every collocated
// node: GEL_PROP_RESTART_NODE) and see whether the trajectory arrives where the collocated states say.  Independent of D and I.
//
// Three kernels per call, the first two once per slab of vectors:
//   prop_sample_kernel   the control polynomial at every stage point of the free-attitude phases, in interp_kernel's register-
//                        blocked style (a lane owns one stage point of kPropSampleVB vectors whose U lies in LDS; the matrix is
//                        stored transposed: one coalesced load per column), into the plan's workspace [stage point][2][vector]
//   prop_kernel          one lane = one (vector, segment); a wavefront = 64 consecutive vectors of ONE segment, so the phase and
//                        the step count are wave-uniform and the two control samples of a stage are one coalesced load each.
//                        The step is written down in gel_prop.h; its pieces are gel_flight_step.h's.  The loop lengths n and k come from the plan's tables, which
//                        creation bounds (k n <= 2^20): a launch always ends.
//                        Template parameters: kChain (GEL_PROP_CHAIN) one lane = one vector through ALL phases, the state carried
//                        across the knots; kDisp (gel_propagate_dispersed*) per (vector, phase) factors of thrust, mass flow,
//                        reference area and wind.  <false, false> is the kernel as it was before the template.  kEns = 1
//                        (gel_propagate_ensemble*): every lane's wind table is the one its vector is assigned.
//   prop_err_kernel      err [B][S][4] from x and y: one lane = one (vector, phase), nodes in ascending order
// fp64 throughout; the right-hand side is section_rhs (gel_section_rhs.h), the one mesh_kernel evaluates.
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_section_rhs.h"
#include "gel_flight_step.h"

namespace gel {

__global__ __launch_bounds__(kPropSampleThreads) void prop_sample_kernel(ProblemDev P, PropDev Pd, int nb, const double* __restrict__ x,
                                                                         double* __restrict__ ws, long long ld) {
  extern __shared__ double lds[];
  constexpr int VB = kPropSampleVB;
  // workgroup -> (phase, group of vectors, point tile): the sampled phases' workgroups one after the other
  const long long ng = ((long long)nb + VB - 1) / VB;
  int s = 0;
  long long wg = blockIdx.x;
  for (; s < Pd.S; s++) {
    const long long c = ng * Pd.ph[s].ntile;
    if (wg < c) break;
    wg -= c;
  }
  if (s >= Pd.S) return;   // (never: the grid is the sum over phases)
  const PropPhaseDev q = Pd.ph[s];
  const PhaseDev ph = load_phase(P.phases + s);
  const long long grp = wg / q.ntile;
  const int tile = (int)(wg - grp * q.ntile);
  const int n = q.n, t = threadIdx.x;
  const long long Pp = 2LL * q.k * n + 1;
  const double* xv[VB];
#pragma unroll
  for (int v = 0; v < VB; v++) {
    const long long b = grp * VB + v;
    xv[v] = x + (size_t)(b < nb ? b : nb - 1) * P.nvars + 11 * (size_t)P.M + 2 * (size_t)ph.ua;   // (a tail group reads its last vector again)
  }
  for (int r = t; r < 2 * n; r += kPropSampleThreads) {
#pragma unroll
    for (int v = 0; v < VB; v++) lds[(size_t)r * VB + v] = xv[v][r];   // U [n][2][VB]
  }
  __syncthreads();
  const long long l = (long long)tile * kPropSampleThreads + t;
  if (l >= Pp) return;
  double u[2][VB];
#pragma unroll
  for (int v = 0; v < VB; v++) u[0][v] = u[1][v] = 0.0;
  const double* W = Pd.mat + q.wu + l;
  for (int j = 0; j < n; j++) {
    const double w = W[(size_t)j * Pp];
    const double* Uj = lds + (size_t)j * 2 * VB;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int v = 0; v < VB; v++) u[c][v] = __builtin_fma(w, Uj[c * VB + v], u[c][v]);
  }
  const int cu = Pd.cp[q.cu + l];
  if (cu >= 0) {
    const double* Uj = lds + (size_t)cu * 2 * VB;
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int v = 0; v < VB; v++) u[c][v] = Uj[c * VB + v];
  }
  double* o = ws + (size_t)(q.pt0 + l) * 2 * (size_t)ld + (size_t)grp * VB;
#pragma unroll
  for (int v = 0; v < VB; v++) {
    if (grp * VB + v >= nb) continue;
    o[v] = u[0][v];
    o[(size_t)ld + v] = u[1][v];
  }
}

// kDisp (gel_propagate_dispersed*): disp [nb][S][kPropNDisp]; the lane's four factors of a phase scale the phase record once (thrust,
// mass flow, reference area: one product each) and the interpolated wind inside section_rhs.
// kChain (GEL_PROP_CHAIN): one lane = one vector, which walks the phases in order and carries its state across the knots; a
// workgroup = kPropThreads consecutive vectors, so the phase stays wave-uniform.  Without either the code is the one-segment body.
// kEns = 1 (gel_propagate_ensemble*; with kDisp only, the other instantiations do not read Ens): the lane looks the wind up in the
// table its vector is assigned (ens_lane_tables: global memory) and keeps that table's altitude interval across stages, steps and
// phases.  disp may then be null: factors of one.  An int, not a branch on Ens.tables inside the dispersed instantiations: with both
// right-hand sides in one kernel the dispersed instantiations took 194 / 202 VGPRs (2 waves/SIMD) instead of 148 / 154.
template <bool kDisp, bool kChain, int kEns = 0>
__global__ __launch_bounds__(kPropThreads) void prop_kernel(ProblemDev P, PropDev Pd, int nb, const double* __restrict__ x,
                                                            double* __restrict__ y, const double* __restrict__ ws, long long ld,
                                                            const double* __restrict__ disp, EnsDev Ens) {
  extern __shared__ double lds[];
  // workgroup -> (segment, group of kPropThreads vectors); chain mode: the group alone
  const int ngrp = (nb + kPropThreads - 1) / kPropThreads;
  const int seg = kChain ? 0 : blockIdx.x / ngrp, grp = blockIdx.x - seg * ngrp;
  const Tables tb = stage_tables(P, lds);
  const int v = grp * kPropThreads + (int)threadIdx.x;
  if (seg >= Pd.nseg || v >= nb) return;   // (idle lanes leave: they stay out of the calm-air vote of wind_eci_or_calm; no barrier follows)
  bool bad = false;
  double yv[11];
  // under an ensemble: the lane's view of the tables (its wind part in global memory) and its kept altitude interval
  Tables tbe = tb;
  Bracket2 wbr = no_bracket2();
  if constexpr (kEns) tbe = ens_lane_tables(P, tb, Ens, Ens.member[v]);
  int s = kChain ? 0 : load_const(&Pd.seg_phase[seg]);
  do {
    const int M = P.M;
    const double* const xb = x + (size_t)v * P.nvars;
    double* const yb = y + (size_t)v * 11 * (size_t)M;
    FlightPhase f = load_flight_phase(P, Pd, s, xb);
    const PhaseDev& ph = f.ph;
    const int j0 = (!kChain && Pd.restart) ? seg - load_const(&Pd.ph[s].seg0) : 0, j1 = (!kChain && Pd.restart) ? j0 + 1 : f.n;
    const double* const us = ws + f.pt0 * 2 * (size_t)ld + v;
    if (kDisp && (!kEns || disp)) apply_factors(f, disp + ((size_t)v * Pd.S + s) * kPropNDisp);   // (null only under an ensemble: factors of one)

    if (kChain && s > 0) {
      // across the knot the collocated jump x(first node of s) - x(last node of s - 1) is added to the carried state; a zero jump
      // carries the bits (y + 0 would turn a -0 into +0)
#pragma unroll
      for (int c = 0; c < 11; c++) {
        const double jump = xb[state_index(M, ph.xa, c)] - xb[state_index(M, ph.xa - 1, c)];
        yv[c] = (jump == 0.0) ? yv[c] : yv[c] + jump;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 11; c++) yv[c] = xb[state_index(M, ph.xa + j0, c)];
    }
    if (j0 == 0) {   // node xa: X_0 bit for bit (chain mode beyond phase 0: the carried state)
#pragma unroll
      for (int c = 0; c < 11; c++) { yb[state_index(M, ph.xa, c)] = yv[c]; bad |= nonfinite(yv[c]); }
    }
    for (int j = j0; j < j1; j++) {
      const double Sh = f.S * f.hs[j], Sh2 = Sh * 0.5, Sh6 = Sh / 6.0;
      for (int i = 0; i < f.k; i++) {
        const int p = 2 * (f.k * j + i);
        double acc[11], F[11];
#pragma unroll
        for (int c = 0; c < 11; c++) acc[c] = F[c] = 0.0;
#pragma nounroll
        for (int st = 0; st < 4; st++) {
          const Stage g = rk4_stage(p, st, Sh, Sh2);
          double yt[11];
#pragma unroll
          for (int c = 0; c < 11; c++) yt[c] = st ? __builtin_fma(g.a, F[c], yv[c]) : yv[c];
          double u0, u1;
          stage_controls(us, (size_t)ld, f.sampled, g.pp, u0, u1);
          if constexpr (kEns) section_rhs<true, true>(P, ph, tbe, Pd.vp, f.sig[g.pp], f.to, f.tf, yt, u0, u1, F, f.fw, &wbr);
          else if constexpr (kDisp) section_rhs<true>(P, ph, tb, Pd.vp, f.sig[g.pp], f.to, f.tf, yt, u0, u1, F, f.fw);
          else section_rhs(P, ph, tb, Pd.vp, f.sig[g.pp], f.to, f.tf, yt, u0, u1, F);
#pragma unroll
          for (int c = 0; c < 11; c++) acc[c] = st ? __builtin_fma(g.w, F[c], acc[c]) : F[c];
        }
#pragma unroll
        for (int c = 0; c < 11; c++) yv[c] = __builtin_fma(Sh6, acc[c], yv[c]);
      }
#pragma unroll
      for (int c = 0; c < 11; c++) { yb[state_index(M, ph.xa + j + 1, c)] = yv[c]; bad |= nonfinite(yv[c]); }
    }
  } while (kChain && ++s < Pd.S);
  if (bad) *(volatile int32_t*)P.flag = 1;
}

__global__ __launch_bounds__(256) void prop_err_kernel(ProblemDev P, PropDev Pd, int B, const double* __restrict__ x,
                                                       const double* __restrict__ y, double* __restrict__ err) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)B * Pd.S) return;
  const long long b = t / Pd.S;
  const int s = (int)(t - b * Pd.S);
  const int n = P.phases[s].n, xa = P.phases[s].xa, M = P.M;
  const double* xb = x + (size_t)b * P.nvars;
  const double* yb = y + (size_t)b * 11 * (size_t)M;
  double d[11], mx[11];
#pragma unroll
  for (int c = 0; c < 11; c++) { d[c] = 0.0; mx[c] = nan_max(0.0, fabs(xb[state_index(M, xa, c)])); }
  for (int i = 1; i <= n; i++) {
#pragma unroll
    for (int c = 0; c < 11; c++) {
      const size_t k = state_index(M, xa + i, c);
      const double xv = xb[k];
      d[c] = nan_max(d[c], fabs(yb[k] - xv));
      mx[c] = nan_max(mx[c], fabs(xv));
    }
  }
#pragma unroll
  for (int c = 0; c < 11; c++) d[c] = d[c] / (1.0 + mx[c]);   // max_i (|d_i| / den) = (max_i |d_i|) / den: the rounded quotient is monotone
  bool bad = false;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int c0 = (g == 0) ? 0 : 3 * g - 2, c1 = (g == 0) ? 1 : (g == 3) ? 11 : 3 * g + 1;   // [0,1) [1,4) [4,7) [7,11)
    double e = 0.0;
#pragma unroll
    for (int c = c0; c < c1; c++) e = nan_max(e, d[c]);
    err[(size_t)t * 4 + g] = e;
    bad |= nonfinite(e);
  }
  if (bad) *(volatile int32_t*)P.flag = 1;
}

hipError_t launch_prop_slab(const ProblemDev& P, const PropDev& Pd, const PropPhaseDev* host_ph, int n_max_sampled, int nb,
                            const double* d_x, double* d_y, double* d_ws, int64_t ld, const double* d_disp, const EnsDev& ens,
                            hipStream_t s) {
  if (nb <= 0) return hipSuccess;
  if (ld < nb) return hipErrorInvalidValue;
  const long long ng = ((long long)nb + kPropSampleVB - 1) / kPropSampleVB;
  long long grid = 0;
  for (int i = 0; i < Pd.S; i++) grid += ng * host_ph[i].ntile;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (grid > 0) {
    const size_t lds = prop_sample_lds_bytes(n_max_sampled);
    if (lds > kPropMaxLds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prop_sample_kernel, dim3((unsigned)grid), dim3(kPropSampleThreads), lds, s, P, Pd, nb, d_x, d_ws, (long long)ld);
    if (const hipError_t e = hipGetLastError()) return e;
  }
  const long long ngrp = ((long long)nb + kPropThreads - 1) / kPropThreads;
  grid = Pd.chain ? ngrp : ngrp * Pd.nseg;
  if (grid <= 0) return hipSuccess;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds = table_lds_bytes(P.Kw, P.Kc);
  auto* const kern = ens.tables ? (Pd.chain ? prop_kernel<true, true, 1> : prop_kernel<true, false, 1>)
                     : Pd.chain ? (d_disp ? prop_kernel<true, true> : prop_kernel<false, true>)
                                : (d_disp ? prop_kernel<true, false> : prop_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropThreads), lds, s, P, Pd, nb, d_x, d_y, d_ws, (long long)ld, d_disp, ens);
  return hipGetLastError();
}

hipError_t launch_prop_err(const ProblemDev& P, const PropDev& Pd, int B, const double* d_x, const double* d_y, double* d_err,
                           hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const long long grid = ((long long)B * Pd.S + 255) / 256;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prop_err_kernel, dim3((unsigned)grid), dim3(256), 0, s, P, Pd, B, d_x, d_y, d_err);
  return hipGetLastError();
}

}  // namespace gel
