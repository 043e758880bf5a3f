// gel_kernels_propadj.hip -- the adjoint flight (gel_propagate_adjoint*): the TRANSPOSE of the linear map
// gel_propagate_tangent* applies (gel_kernels_proptan.hip), applied to Q multipliers lam on y per vector.  The value flight itself is
// prop_kernel's (launch_prop_slab runs before these kernels); its y is both the call's output and the checkpoint set: y(node j) is the
// start of node interval j.
//
//   propadj_kernel<kChain>   one lane = one (vector, functional): lane l of a slab is functional l % Q of vector l / Q.  A
//                            workgroup = kPropAdjThreads = 64 consecutive lanes, all in the same phase: n and k are wave-uniform.
//                            In section mode too the lane walks ALL phases, one after the other, with lm starting at zero in each:
//                            the inner checkpoints [k_max - 1][11] are the lane's, and one thread per (lane, phase) would have S
//                            threads write and read the same cells at once.
//                            The tables are read where the handle keeps them, in global memory, as proptan_kernel reads them.  The
//                            lane walks BACKWARDS: phases S - 1 .. 0 (chain), intervals n - 1 .. 0, steps k - 1 .. 0.  No atomics:
//                            every output cell has one writer.
//   prop_sample_t_kernel     the transposed control sampler and the knot times' finishing step: one lane = one (lane of the slab,
//                            control node), plus one row of lanes for the S + 1 times.
//
// ONE STEP, REVERSED (value lines: gel_prop.h, on gel_flight_step.h's stage helpers; lm = the multiplier of the step's END state on entry, of its START state on exit):
//   restart   per interval, once: from y(node j) the k - 1 value steps to the starts of steps 1 .. k - 1, kept per lane in the
//             workspace (inner checkpoints); per step: F1 .. F3 with the value's own fma lines (kept in LDS): yt has the bits the
//             flight had
//   lacc = Sh6 lm
//   stage 4:  lF = lacc;                     (lyt4, lu, lfac) = section_rhs_adjoint(yt4, lF)
//   stage 3:  lF = fma(Sh,  lyt4, 2 lacc);   ... lyt3
//   stage 2:  lF = fma(Sh2, lyt3, 2 lacc);   ... lyt2
//   stage 1:  lF = fma(Sh2, lyt2,   lacc);   ... lyt1
//   lm  += ((lyt4 + lyt3) + lyt2) + lyt1
//   gS   = fma(hs[j], <lm_in, acc> / 6 + <lyt4, F3> + <lyt3, F2> / 2 + <lyt2, F1> / 2, gS)     (every <,> one fma chain, c ascending)
//   factors' multipliers: summed over the stages in walk order, per phase
// STAGE POINTS' CONTROL MULTIPLIERS gws [stage point][2][lanes], every cell stored once: the step's end point gets stage 4's plus the
// stage-1 pair of the step walked before (the next one in time), which the lane carries in registers; the midpoint gets
// stage 2's + stage 3's; the phase's first point gets the last carried pair.
// NODES: lam's rows of a node are added to lm where the walk passes the node.  A segment's start row: g = lm.  Chain knot into
// phase s: g[first node of s] = lm, g[last node of s - 1] = 0 - lm, and lm carries on.  Every other state row: +0.0.
// FACTORS: gdisp[s] = (handle's thrust, mf_um, area, 1) * (the phase's summed multipliers), as the tangent forms d.dthrust.
// TIMES (prop_sample_t_kernel): dS_s = (dt_{s+1} - dt_s) unit_t / 2, so gt[s] = ((gS[s-1] - gS[s]) * unit_t) / 2.0 with gS[-1] = gS[S] = 0.
// CONTROLS (prop_sample_t_kernel): gu[node j][c] = fma chain over ascending p of WuT[j][p] gws[p][c], skipping the stage points that
// ARE a collocation node (copy_u[p] >= 0: the value call bypasses Wu there); their cells are summed (ascending p) and added to the
// chain's result of node copy_u[p].  Hold-type phases: +0.0.
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_section_rhs_adj.h"
#include "gel_flight_step.h"
#include "gel_propadj.h"

namespace gel {

// kEns = 1 (gel_propagate_adjoint_ensemble*): as proptan_kernel's -- an EnsDev behind the arguments (the pack Ens
// holds exactly that one; none with kEns = 0, whose instantiations keep their argument list), and the lane's view of the tables
// (ens_lane_tables) in every call that reads the wind: the inner checkpoints' value steps, F1 .. F3 and the four reversed stages.
//
// kEns & 2 (gel_propagate_adjoint_wind*): a WindGradDev is the pack's LAST argument (behind the EnsDev where kEns = 3).
// WIND ROWS: the lane owns column l of gww [Kg][2][gld] (lane-major like gws: the functionals of one vector sit on the same piece, so
// their cells are neighbours), zeroed on the stream before the walk.  Every reversed air stage adds its (fw lwn, fw lwe) to the
// cells of the piece's two rows (gel_wind_rows.h) by read-add-write, in walk order, by this lane alone: one writer, no atomics --
// in section mode too, where the one lane walks every phase.  The rows lie below the LANE's Kw <= Kg.  After the walk the lane
// copies its column out as gwind [lane][Kg][2]: every element is written, an untouched row is the +0.0 it was zeroed to.
// kEns = 0 and 1 are the instantiations they were: the same argument lists, the same code.
template <bool kChain, int kEns = 0, typename... Ens>
__global__ __launch_bounds__(kPropAdjThreads) void propadj_kernel(ProblemDev P, PropDev Pd, PropAdjArgs A, Ens... ens) {
  static_assert(sizeof...(Ens) == (kEns & 1) + ((kEns >> 1) & 1), "an EnsDev with kEns & 1, then a WindGradDev with kEns & 2, nothing else");
  constexpr bool kWind = (kEns & 2) != 0;
  constexpr int T = kPropAdjThreads;
  __shared__ double Fs[3 * 11 * T];   // F1 .. F3 of the step in hand: [stage][component][lane]
  const long long nl = (long long)A.nb * A.Q;
  const Tables tb = table_view(P.tables, P.Kw, P.Kc);   // the handle's tables where they lie (global memory): no LDS copy
  const long long l = (long long)blockIdx.x * T + (long long)threadIdx.x;
  if (l >= nl) return;   // (idle lanes leave: they stay out of the calm-air vote of wind_eci_or_calm; no barrier follows)
  double* const Fl = Fs + threadIdx.x;     // the lane's column: no other lane reads or writes it
  const int v = (int)(l / A.Q), qf = (int)(l - (long long)v * A.Q);
  Tables tbe = tb;   // under an ensemble: the lane's view (the wind part of its vector's member)
  if constexpr ((kEns & 1) != 0) tbe = ens_lane_view(P, tb, v, pack_first(ens...));
  double* gwl = nullptr;   // the lane's column of gww
  if constexpr (kWind) gwl = pack_last(ens...).gww + (size_t)l;
  const int M = P.M, N = P.N;
  const double* const xb = A.x + (size_t)v * P.nvars;
  const double* const yb = A.y + (size_t)v * 11 * (size_t)M;
  const double* const lamb = A.lam + (A.shared ? (size_t)qf : (size_t)l) * 11 * (size_t)M;
  double* const gxb = A.gx + (size_t)l * P.nvars;
  double* const ckl = A.ck + (size_t)l;   // the lane's inner checkpoints [k - 1][11]: written and read by this lane alone
  bool bad = false;
  double lm[11];
#pragma unroll
  for (int c = 0; c < 11; c++) lm[c] = 0.0;
  int s = Pd.S - 1;
  do {
    if (!kChain) {   // every phase is a segment of its own: nothing is carried across the knot
#pragma unroll
      for (int c = 0; c < 11; c++) lm[c] = 0.0;
    }
    PhaseDev ph = load_phase(P.phases + s);
    const int n = load_const(&Pd.ph[s].n), k = load_const(&Pd.ph[s].k), sampled = load_const(&Pd.ph[s].sampled);
    const double* const sig = Pd.mat + load_const(&Pd.ph[s].sg);
    const double* const hs = Pd.mat + load_const(&Pd.ph[s].hs);
    const size_t pt0 = (size_t)load_const(&Pd.ph[s].pt0);
    const double* const us = A.ws + pt0 * 2 * (size_t)A.ld + v;
    double* const gus = A.gws + pt0 * 2 * (size_t)A.gld + (size_t)l;
    const double to = xb[11 * M + 2 * N + s], tf = xb[11 * M + 2 * N + s + 1];
    const double S = (tf - to) * P.ut / 2.0;
    const double thrust0 = ph.thrust, mf0 = ph.mf_um, area0 = ph.area;   // the handle's, before the factors scale the record
    double fw = 1.0;
    if (A.disp) {
      const double* const fac = A.disp + ((size_t)v * Pd.S + s) * kPropNDisp;
      const double f_thrust = fac[0], f_mf = fac[1], f_area = fac[2];
      fw = fac[3];
      ph.thrust = ph.thrust * f_thrust;
      ph.mf_um = ph.mf_um * f_mf;
      ph.area = ph.area * f_area;
    }
    // the phase's last node: its lam rows; its row of gx is the next phase's to write across a chain knot, else +0.0
#pragma unroll
    for (int c = 0; c < 11; c++) {
      const size_t i = state_index(M, ph.xa + n, c);
      lm[c] += lamb[i];
      if (!kChain || s == Pd.S - 1) gxb[i] = 0.0;
    }
    double gfac[4] = {0.0, 0.0, 0.0, 0.0}, gSv = 0.0, cu0 = 0.0, cu1 = 0.0;
    for (int j = n - 1; j >= 0; j--) {
      const double Sh = S * hs[j], Sh2 = Sh * 0.5, Sh6 = Sh / 6.0;
      // the interval's inner checkpoints: the starts of steps 1 .. k - 1, integrated once with the value step from the node's
      // checkpoint (k - 1 steps per interval; nothing at k = 1) into the lane's column of the workspace
      if (k > 1) {
        double yv[11];
#pragma unroll
        for (int c = 0; c < 11; c++) yv[c] = yb[state_index(M, ph.xa + j, c)];
        for (int ii = 0; ii < k - 1; ii++) {
          const int pf = 2 * (k * j + ii);
          double acc[11], F[11];
#pragma unroll
          for (int c = 0; c < 11; c++) acc[c] = F[c] = 0.0;
#pragma nounroll
          for (int st = 0; st < 4; st++) {
            const Stage g = rk4_stage(pf, st, Sh, Sh2);
            double yt[11];
#pragma unroll
            for (int c = 0; c < 11; c++) yt[c] = st ? __builtin_fma(g.a, F[c], yv[c]) : yv[c];
            double u0, u1;
            stage_controls(us, (size_t)A.ld, sampled, g.pp, u0, u1);
            section_rhs<true>(P, ph, (kEns & 1) ? tbe : tb, Pd.vp, sig[g.pp], to, tf, yt, u0, u1, F, fw);
#pragma unroll
            for (int c = 0; c < 11; c++) acc[c] = st ? __builtin_fma(g.w, F[c], acc[c]) : F[c];
          }
#pragma unroll
          for (int c = 0; c < 11; c++) {
            yv[c] = __builtin_fma(Sh6, acc[c], yv[c]);
            ckl[((size_t)ii * 11 + c) * (size_t)A.gld] = yv[c];
          }
        }
      }
      for (int i = k - 1; i >= 0; i--) {
        // ---- forward: the step's start (the node's checkpoint, or the interval's inner checkpoint), then F1 .. F3 ----
        const int pb = 2 * (k * j + i);
        double yv[11];
#pragma unroll
        for (int c = 0; c < 11; c++) yv[c] = i ? ckl[((size_t)(i - 1) * 11 + c) * (size_t)A.gld] : yb[state_index(M, ph.xa + j, c)];
        {
          double F[11];
#pragma unroll
          for (int c = 0; c < 11; c++) F[c] = 0.0;
#pragma nounroll
          for (int st = 0; st < 3; st++) {
            const Stage g = rk4_stage(pb, st, Sh, Sh2);
            double yt[11];
#pragma unroll
            for (int c = 0; c < 11; c++) yt[c] = st ? __builtin_fma(g.a, F[c], yv[c]) : yv[c];
            double u0, u1;
            stage_controls(us, (size_t)A.ld, sampled, g.pp, u0, u1);
            section_rhs<true>(P, ph, (kEns & 1) ? tbe : tb, Pd.vp, sig[g.pp], to, tf, yt, u0, u1, F, fw);
#pragma unroll
            for (int c = 0; c < 11; c++) Fl[(st * 11 + c) * T] = F[c];
          }
        }
        // ---- the four stages, reversed ----
        double lacc[11], lsum[11], lyt[11], gstep = 0.0, mid0 = 0.0, mid1 = 0.0;
#pragma unroll
        for (int c = 0; c < 11; c++) { lacc[c] = Sh6 * lm[c]; lsum[c] = 0.0; lyt[c] = 0.0; }
#pragma nounroll
        for (int st = 3; st >= 0; st--) {
          const Stage sg = rk4_stage(pb, st, Sh, Sh2);          // its point, and a of yt = y + a F_prev; the weight is the reversed walk's own
          const int pp = sg.pp;
          const double an = (st == 2) ? Sh : Sh2;   // the next stage's a: what its lyt brings to this stage's lF
          const double w = (st == 0) ? 1.0 : 2.0;
          double yt[11], lF[11];
#pragma unroll
          for (int c = 0; c < 11; c++) {
            const double Fp = st ? Fl[((st - 1) * 11 + c) * T] : 0.0;
            yt[c] = st ? __builtin_fma(sg.a, Fp, yv[c]) : yv[c];
            lF[c] = (st == 3) ? lacc[c] : __builtin_fma(an, lyt[c], w * lacc[c]);
          }
          double u0, u1;
          stage_controls(us, (size_t)A.ld, sampled, pp, u0, u1);
          double F[11], lx[11];
          RhsAdjoint g;
          if constexpr (kWind) {
            RhsWindAdjoint gw;
            section_rhs_adjoint<true>(P, ph, (kEns & 1) ? tbe : tb, Pd.vp, sig[pp], to, tf, yt, u0, u1, fw, lF, F, lx, g, &gw);
            if (ph.air) {   // (an air-less phase has no wind: gw is not written)
              const size_t g1 = (size_t)A.gld;
              double* const c0 = gwl + 2 * (size_t)gw.rows.i0 * g1;
              if (gw.rows.i1 != gw.rows.i0) {
                double* const c1 = gwl + 2 * (size_t)gw.rows.i1 * g1;
                const double t1 = gw.rows.th, t0 = 1.0 - t1;
                c0[0] = __builtin_fma(t0, gw.wn, c0[0]);
                c0[g1] = __builtin_fma(t0, gw.we, c0[g1]);
                c1[0] = __builtin_fma(t1, gw.wn, c1[0]);
                c1[g1] = __builtin_fma(t1, gw.we, c1[g1]);
              } else {
                c0[0] = c0[0] + gw.wn;
                c0[g1] = c0[g1] + gw.we;
              }
            }
          } else {
            section_rhs_adjoint(P, ph, kEns ? tbe : tb, Pd.vp, sig[pp], to, tf, yt, u0, u1, fw, lF, F, lx, g);
          }
          if (st == 3) {   // <lm, acc> / 6 with acc of the value lines
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < 11; c++) {
              double acc = __builtin_fma(2.0, Fl[(1 * 11 + c) * T], Fl[c * T]);
              acc = __builtin_fma(2.0, Fl[(2 * 11 + c) * T], acc);
              acc = __builtin_fma(1.0, F[c], acc);
              d = __builtin_fma(lm[c], acc, d);
            }
            gstep = d / 6.0;
          }
          if (st) {
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < 11; c++) d = __builtin_fma(lx[c], Fl[((st - 1) * 11 + c) * T], d);
            gstep += (st == 3) ? d : d * 0.5;
          }
#pragma unroll
          for (int c = 0; c < 11; c++) { lsum[c] += lx[c]; lyt[c] = lx[c]; }
          gfac[0] += g.thrust;
          gfac[1] += g.mf;
          gfac[2] += g.area;
          gfac[3] += g.fw;
          if (sampled) {
            if (st == 3) {
              gus[(size_t)(pb + 2) * 2 * (size_t)A.gld] = g.u0 + cu0;
              gus[((size_t)(pb + 2) * 2 + 1) * (size_t)A.gld] = g.u1 + cu1;
            } else if (st == 2) {
              mid0 = g.u0;
              mid1 = g.u1;
            } else if (st == 1) {
              gus[(size_t)(pb + 1) * 2 * (size_t)A.gld] = mid0 + g.u0;
              gus[((size_t)(pb + 1) * 2 + 1) * (size_t)A.gld] = mid1 + g.u1;
            } else {
              cu0 = g.u0;
              cu1 = g.u1;
            }
          }
        }
#pragma unroll
        for (int c = 0; c < 11; c++) lm[c] += lsum[c];
        gSv = __builtin_fma(hs[j], gstep, gSv);
      }
      // the walk passes node xa + j: its lam rows; an inner node's row of gx is +0.0 (the value call does not read it)
#pragma unroll
      for (int c = 0; c < 11; c++) {
        const size_t i = state_index(M, ph.xa + j, c);
        lm[c] += lamb[i];
        if (j > 0) gxb[i] = 0.0;
      }
    }
    // the segment's start
#pragma unroll
    for (int c = 0; c < 11; c++) {
      gxb[state_index(M, ph.xa, c)] = lm[c];
      if (kChain && s > 0) gxb[state_index(M, ph.xa - 1, c)] = 0.0 - lm[c];
      bad |= nonfinite(lm[c]);
    }
    if (sampled) {
      gus[0] = cu0;
      gus[(size_t)A.gld] = cu1;
    }
    A.gS[(size_t)s * (size_t)A.gld + (size_t)l] = gSv;
    bad |= nonfinite(gSv);
    if (A.gdisp) {
      double* const gd = A.gdisp + ((size_t)l * Pd.S + s) * kPropNDisp;
      const double g0 = thrust0 * gfac[0], g1 = mf0 * gfac[1], g2 = area0 * gfac[2], g3 = gfac[3];
      gd[0] = g0; gd[1] = g1; gd[2] = g2; gd[3] = g3;
      bad |= nonfinite(g0);
      bad |= nonfinite(g1);
      bad |= nonfinite(g2);
      bad |= nonfinite(g3);
    }
  } while (--s >= 0);
  if constexpr (kWind) {
    const WindGradDev& wg = pack_last(ens...);
    double* const out = wg.gwind + (size_t)l * 2 * (size_t)wg.Kg;
    for (int i = 0; i < 2 * wg.Kg; i++) {
      const double gv = gwl[(size_t)i * (size_t)A.gld];
      out[i] = gv;
      bad |= nonfinite(gv);
    }
  }
  if (bad) *(volatile int32_t*)P.flag = 1;
}

// workgroup -> (row, group of lanes): row < N: control node `row`; row == N: the knot times.  gx [nl][nvars] lane-major.
__global__ __launch_bounds__(kPropAdjSampleThreads) void prop_sample_t_kernel(ProblemDev P, PropDev Pd, long long nl,
                                                                             const double* __restrict__ gws, const double* __restrict__ gS,
                                                                             long long gld, double* __restrict__ gx) {
  const long long ngrp = (nl + kPropAdjSampleThreads - 1) / kPropAdjSampleThreads;
  const int row = (int)(blockIdx.x / ngrp), M = P.M, N = P.N;
  const long long l = (blockIdx.x - row * ngrp) * kPropAdjSampleThreads + threadIdx.x;
  if (l >= nl) return;
  double* const gxb = gx + (size_t)l * P.nvars + 11 * (size_t)M;
  bool bad = false;
  if (row < N) {
    int s = 0, ua = 0;
    for (; s < Pd.S - 1; s++) {
      const int n = Pd.ph[s].n;
      if (row < ua + n) break;
      ua += n;
    }
    const PropPhaseDev q = Pd.ph[s];
    const int j = row - ua;
    double g0 = 0.0, g1 = 0.0, e0 = 0.0, e1 = 0.0;
    if (q.sampled) {
      const long long Pp = 2LL * q.k * q.n + 1;
      const double* const W = Pd.mat + q.wu + (size_t)j * (size_t)Pp;
      const int32_t* const cp = Pd.cp + q.cu;
      const double* const cell = gws + (size_t)q.pt0 * 2 * (size_t)gld + (size_t)l;
      for (long long p = 0; p < Pp; p++) {
        const int cu = cp[p];
        if (cu >= 0 && cu != j) continue;   // another node's own point: the value call reads only that node there
        const double c0 = cell[(size_t)p * 2 * (size_t)gld], c1 = cell[((size_t)p * 2 + 1) * (size_t)gld];
        if (cu >= 0) {
          e0 += c0;
          e1 += c1;
        } else {
          const double w = W[p];
          g0 = __builtin_fma(w, c0, g0);
          g1 = __builtin_fma(w, c1, g1);
        }
      }
    }
    const double r0 = g0 + e0, r1 = g1 + e1;
    gxb[2 * (size_t)row] = r0;
    gxb[2 * (size_t)row + 1] = r1;
    bad = nonfinite(r0) || nonfinite(r1);
  } else {
    for (int s = 0; s <= Pd.S; s++) {
      const double a = (s > 0) ? gS[(size_t)(s - 1) * (size_t)gld + (size_t)l] : 0.0;
      const double b = (s < Pd.S) ? gS[(size_t)s * (size_t)gld + (size_t)l] : 0.0;
      const double gt = ((a - b) * P.ut) / 2.0;
      gxb[2 * (size_t)N + s] = gt;
      bad |= nonfinite(gt);
    }
  }
  if (bad) *(volatile int32_t*)P.flag = 1;
}

hipError_t launch_propadj_slab(const ProblemDev& P, const PropDev& Pd, const PropAdjArgs& A, const EnsDev& ens, const WindGradDev& wg,
                               hipStream_t s) {
  if (A.nb <= 0 || A.Q <= 0) return hipSuccess;
  if (Pd.restart) return hipErrorInvalidValue;
  const long long nl = (long long)A.nb * A.Q;
  if (A.ld < A.nb || A.gld < nl || !A.ck) return hipErrorInvalidValue;
  const long long grid = (nl + kPropAdjThreads - 1) / kPropAdjThreads;   // one lane per (vector, functional) in either mode
  const long long sgrid = (nl + kPropAdjSampleThreads - 1) / kPropAdjSampleThreads * ((long long)P.N + 1);
  if (grid <= 0) return hipSuccess;
  if (grid > 0x7fffffffLL || sgrid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (wg.gwind) {
    // the rows must cover every table a lane may read: the handle's (no ensemble, or member -1) and the members'
    if (!wg.gww || wg.Kg < P.Kw || (ens.tables && wg.Kg < ens.Kw)) return hipErrorInvalidValue;
    if (const hipError_t e = hipMemsetAsync(wg.gww, 0, (size_t)wg.Kg * 2 * (size_t)A.gld * sizeof(double), s)) return e;
    if (ens.tables) {
      auto* const kern = Pd.chain ? propadj_kernel<true, 3, EnsDev, WindGradDev> : propadj_kernel<false, 3, EnsDev, WindGradDev>;
      hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropAdjThreads), 0, s, P, Pd, A, ens, wg);
    } else {
      auto* const kern = Pd.chain ? propadj_kernel<true, 2, WindGradDev> : propadj_kernel<false, 2, WindGradDev>;
      hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropAdjThreads), 0, s, P, Pd, A, wg);
    }
  } else if (ens.tables) {
    auto* const kern = Pd.chain ? propadj_kernel<true, 1, EnsDev> : propadj_kernel<false, 1, EnsDev>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropAdjThreads), 0, s, P, Pd, A, ens);
  } else {
    auto* const kern = Pd.chain ? propadj_kernel<true> : propadj_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kPropAdjThreads), 0, s, P, Pd, A);
  }
  if (const hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(prop_sample_t_kernel, dim3((unsigned)sgrid), dim3(kPropAdjSampleThreads), 0, s, P, Pd, nl,
                     (const double*)A.gws, (const double*)A.gS, A.gld, A.gx);
  return hipGetLastError();
}

}  // namespace gel
