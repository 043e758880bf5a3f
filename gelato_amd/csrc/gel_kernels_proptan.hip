// gel_kernels_proptan.hip -- the tangent-linear propagation (gel_propagate_tangent*): the flight of
// gel_propagate_dispersed* together with the derivative of that discrete RK4 map along P seed directions per vector.
//
//   proptan_kernel<kChain>   one lane = one (vector, direction, segment): lane l of a slab is direction l % P of vector l / P, so
//                            dy [B][P][11 M] is lane-major.  A workgroup = kPropThreads consecutive lanes of ONE segment: the phase,
//                            n and k are wave-uniform.  The atmosphere, wind and CA tables are read where the handle keeps
//                            them, in global memory (the layout the other kernels copy into LDS: the same entries, hence
//                            the same bits): the rows a lookup compares against are the same addresses in every lane, and the
//                            kernel has no staging pass whose length depends on the tables' row counts.  Every lane recomputes its
//                            vector's value trajectory -- direction p's bits do not depend on P, and the extra lanes are the
//                            wavefronts a chain call lacks -- and direction 0 stores it: y has
//                            gel_propagate_dispersed*'s bits (the factors are applied as prop_kernel<true, .> applies them; a
//                            factor of one changes no bit).
// The control directions are sampled by prop_sample_kernel (gel_kernels_prop.hip), which is linear in the controls, pointed at dx.
// Loop lengths come from the plan's tables (k n <= 2^20): a launch always ends.  The right-hand side and its tangent are
// section_rhs_tangent (gel_section_rhs_tan.h).
//
// THE STEP'S TANGENT, in this order (value lines: gel_prop.h, on gel_flight_step.h's pieces; F, dF: the previous stage's):
//   dS   = (dtf - dto) * unit_t / 2.0;  dSh = dS * hs[j];  dSh2 = dSh * 0.5;  dSh6 = dSh / 6.0
//   dyt  = fma(da, F, fma(a, dF, dy))          a = Sh2, Sh2, Sh and da = dSh2, dSh2, dSh for stages 2, 3, 4; stage 1: dyt = dy
//   dacc = fma(w, dF, dacc)                    w = 2, 2, 1; stage 1: dacc = dF
//   dy   = fma(dSh6, acc, fma(Sh6, dacc, dy))  with acc of the value line, before y is updated
// Knot (chain): djump = dx(first node of s + 1) - dx(last node of s); dy where djump == 0, else dy + djump.
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_section_rhs_tan.h"
#include "gel_flight_step.h"
#include "gel_proptan.h"

namespace gel {

// kEns = 1 (gel_propagate_tangent_ensemble*): the kernel takes an EnsDev behind its arguments -- the pack Ens holds
// exactly that one argument, and none with kEns = 0, whose instantiations keep their argument list -- and the lane looks the wind
// up in the table its vector is assigned (ens_lane_tables; -1: the handle's own).  The view replaces tb in the ONE call that reads
// the wind, so the value, the slope of the interval the value lookup took (dw3) and the clamps all come from the member's rows.
// Every lookup searches (wind_ned2_centre): the interval is that of the member's handle, and so are the bits.
//
// kEns & 2 (gel_propagate_tangent_wind*): a WindSeedDev is the pack's LAST argument (behind the EnsDev where kEns = 3),
// and the lane's direction also moves the values of the wind table its flight reads, by its seed dwind [Kg][2] in global memory
// (per lane, or per direction with shared seeds).  The seed is read at the rows of the piece the value lookup took, which lie below
// the LANE's Kw (the handle's, or its member's): rows of the seed at or beyond that are not read.  kEns = 0 and 1 are the
// instantiations they were: the same argument lists, the same code.
template <bool kChain, int kEns = 0, typename... Ens>
__global__ __launch_bounds__(kPropThreads) void proptan_kernel(ProblemDev P, PropDev Pd, PropTanArgs A, Ens... ens) {
  static_assert(sizeof...(Ens) == (kEns & 1) + ((kEns >> 1) & 1), "an EnsDev with kEns & 1, then a WindSeedDev with kEns & 2, nothing else");
  const long long nl = (long long)A.nb * A.P;
  const long long ngrp = (nl + kPropThreads - 1) / kPropThreads;
  const int seg = kChain ? 0 : (int)(blockIdx.x / ngrp);
  const long long grp = blockIdx.x - seg * ngrp;
  const Tables tb = table_view(P.tables, P.Kw, P.Kc);   // the handle's tables where they lie (global memory): no LDS copy
  const long long l = grp * kPropThreads + (long long)threadIdx.x;
  if (seg >= Pd.nseg || l >= nl) return;   // (idle lanes leave: they stay out of the calm-air vote of wind_eci_or_calm; no barrier follows)
  const int v = (int)(l / A.P), p = (int)(l - (long long)v * A.P);
  Tables tbe = tb;   // under an ensemble: the lane's view (the wind part of its vector's member)
  if constexpr ((kEns & 1) != 0) tbe = ens_lane_view(P, tb, v, pack_first(ens...));
  const size_t ls = A.shared ? (size_t)p : (size_t)l;   // the lane's seed set
  const double* dwl = nullptr;   // the lane's wind seed [Kg][2]
  if constexpr ((kEns & 2) != 0) {
    const WindSeedDev& wd = pack_last(ens...);
    dwl = wd.dwind + ls * 2 * (size_t)wd.Kg;
  }
  bool bad = false;
  double yv[11], dyv[11];
  const int M = P.M, N = P.N;
  const double* const xb = A.x + (size_t)v * P.nvars;
  const double* const dxb = A.dx ? A.dx + ls * P.nvars : nullptr;
  double* const yb = A.y + (size_t)v * 11 * (size_t)M;
  double* const dyb = A.dy + (size_t)l * 11 * (size_t)M;
  int s = kChain ? 0 : load_const(&Pd.seg_phase[seg]);
  do {
    FlightPhase f = load_flight_phase(P, Pd, s, xb);
    const PhaseDev& ph = f.ph;
    const int j0 = (!kChain && Pd.restart) ? seg - load_const(&Pd.ph[s].seg0) : 0, j1 = (!kChain && Pd.restart) ? j0 + 1 : f.n;
    const double* const us = A.ws + f.pt0 * 2 * (size_t)A.ld + v;
    const double* const dus = A.dws + f.pt0 * 2 * (size_t)A.dld + ls;
    double dS = 0.0;
    if (dxb) dS = (dxb[11 * M + 2 * N + s + 1] - dxb[11 * M + 2 * N + s]) * P.ut / 2.0;
    RhsDirection d;
    d.du0 = d.du1 = d.dthrust = d.dmf = d.darea = d.dfw = 0.0;
    if (A.ddisp) {   // (before the factors scale the record: the tangents of thrust f0, mf_um f1 and area f2 along df)
      const double* const df = A.ddisp + (ls * Pd.S + s) * kPropNDisp;
      d.dthrust = ph.thrust * df[0];
      d.dmf = ph.mf_um * df[1];
      d.darea = ph.area * df[2];
      d.dfw = df[3];
    }
    if (A.disp) apply_factors(f, A.disp + ((size_t)v * Pd.S + s) * kPropNDisp);

    if (kChain && s > 0) {
#pragma unroll
      for (int c = 0; c < 11; c++) {
        const size_t i1 = state_index(M, ph.xa, c), i0 = state_index(M, ph.xa - 1, c);
        const double jump = xb[i1] - xb[i0];
        yv[c] = (jump == 0.0) ? yv[c] : yv[c] + jump;
        const double djump = dxb ? dxb[i1] - dxb[i0] : 0.0;
        dyv[c] = (djump == 0.0) ? dyv[c] : dyv[c] + djump;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 11; c++) {
        const size_t i = state_index(M, ph.xa + j0, c);
        yv[c] = xb[i];
        dyv[c] = dxb ? dxb[i] : 0.0;
      }
    }
    if (j0 == 0) {
#pragma unroll
      for (int c = 0; c < 11; c++) {
        const size_t i = state_index(M, ph.xa, c);
        if (p == 0) yb[i] = yv[c];
        dyb[i] = dyv[c];
        bad |= nonfinite(yv[c]);
        bad |= nonfinite(dyv[c]);
      }
    }
    for (int j = j0; j < j1; j++) {
      const double Sh = f.S * f.hs[j], Sh2 = Sh * 0.5, Sh6 = Sh / 6.0;
      const double dSh = dS * f.hs[j], dSh2 = dSh * 0.5, dSh6 = dSh / 6.0;
      for (int i = 0; i < f.k; i++) {
        const int pb = 2 * (f.k * j + i);
        double acc[11], F[11], dacc[11], dF[11];
#pragma unroll
        for (int c = 0; c < 11; c++) acc[c] = F[c] = dacc[c] = dF[c] = 0.0;
#pragma nounroll
        for (int st = 0; st < 4; st++) {
          const Stage g = rk4_stage(pb, st, Sh, Sh2);
          const double da = (st == 3) ? dSh : dSh2;
          double yt[11], dyt[11];
#pragma unroll
          for (int c = 0; c < 11; c++) {
            yt[c] = st ? __builtin_fma(g.a, F[c], yv[c]) : yv[c];
            dyt[c] = st ? __builtin_fma(da, F[c], __builtin_fma(g.a, dF[c], dyv[c])) : dyv[c];
          }
          double u0 = 0.0, u1 = 0.0;
          d.du0 = d.du1 = 0.0;
          if (f.sampled) {   // (stage_controls' reads with the seed's nested inside; two calls in a row compile to a section-mode tangent 2 - 4 % slower)
            u0 = us[(size_t)g.pp * 2 * (size_t)A.ld];
            u1 = us[((size_t)g.pp * 2 + 1) * (size_t)A.ld];
            if (dxb) {
              d.du0 = dus[(size_t)g.pp * 2 * (size_t)A.dld];
              d.du1 = dus[((size_t)g.pp * 2 + 1) * (size_t)A.dld];
            }
          }
          section_rhs_tangent<(kEns & 2) != 0>(P, ph, (kEns & 1) ? tbe : tb, Pd.vp, f.sig[g.pp], f.to, f.tf, yt, u0, u1, f.fw, dyt, d, F, dF, dwl);
#pragma unroll
          for (int c = 0; c < 11; c++) {
            acc[c] = st ? __builtin_fma(g.w, F[c], acc[c]) : F[c];
            dacc[c] = st ? __builtin_fma(g.w, dF[c], dacc[c]) : dF[c];
          }
        }
#pragma unroll
        for (int c = 0; c < 11; c++) {
          dyv[c] = __builtin_fma(dSh6, acc[c], __builtin_fma(Sh6, dacc[c], dyv[c]));
          yv[c] = __builtin_fma(Sh6, acc[c], yv[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < 11; c++) {
        const size_t i = state_index(M, ph.xa + j + 1, c);
        if (p == 0) yb[i] = yv[c];
        dyb[i] = dyv[c];
        bad |= nonfinite(yv[c]);
        bad |= nonfinite(dyv[c]);
      }
    }
  } while (kChain && ++s < Pd.S);
  if (bad) *(volatile int32_t*)P.flag = 1;
}

hipError_t launch_proptan_slab(const ProblemDev& P, const PropDev& Pd, const PropTanArgs& A, const EnsDev& ens, const WindSeedDev& wd,
                               hipStream_t s) {
  if (A.nb <= 0 || A.P <= 0) return hipSuccess;
  const long long nl = (long long)A.nb * A.P;
  if (A.ld < A.nb || (A.dx && A.dld < (A.shared ? (long long)A.P : nl))) return hipErrorInvalidValue;
  const long long ngrp = (nl + kPropThreads - 1) / kPropThreads;
  const long long grid = Pd.chain ? ngrp : ngrp * Pd.nseg;
  if (grid <= 0) return hipSuccess;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (wd.dwind) {
    // the seed's rows must cover every table a lane may read: the handle's (no ensemble, or member -1) and the members'
    if (wd.Kg < P.Kw || (ens.tables && wd.Kg < ens.Kw)) return hipErrorInvalidValue;
    if (ens.tables) {
      auto* const kern = Pd.chain ? proptan_kernel<true, 3, EnsDev, WindSeedDev> : proptan_kernel<false, 3, EnsDev, WindSeedDev>;
      hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropThreads), 0, s, P, Pd, A, ens, wd);
    } else {
      auto* const kern = Pd.chain ? proptan_kernel<true, 2, WindSeedDev> : proptan_kernel<false, 2, WindSeedDev>;
      hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropThreads), 0, s, P, Pd, A, wd);
    }
  } else if (ens.tables) {
    auto* const kern = Pd.chain ? proptan_kernel<true, 1, EnsDev> : proptan_kernel<false, 1, EnsDev>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropThreads), 0, s, P, Pd, A, ens);
  } else {
    auto* const kern = Pd.chain ? proptan_kernel<true> : proptan_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropThreads), 0, s, P, Pd, A);
  }
  return hipGetLastError();
}

}  // namespace gel
