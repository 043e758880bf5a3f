// gel_prop.h -- batched explicit propagation of the sections with classical RK4 (gel_kernels_prop.hip): the
// shooting check.  The tables travel in a struct of their own (PropDev), as MeshDev and InterpDev do, so that ProblemDev keeps its
// layout.
//
// Phase s of n nodes, support tau_x = [-1, tau_1 .. tau_n], k = steps[s]: every node interval [tau_x_j, tau_x_{j+1}] is cut into
// k equal steps, and the phase has Pp = 2 k n + 1 STAGE POINTS: point 2 (k j + i) + m, m = 0, 1, 2, is the start, the middle and
// the end of step i of interval j.
//
// THE STEP, in this order and with these roundings (every product / sum below is one fp64 operation, fma where written):
//   h    = hs[j] = (tau_x_{j+1} - tau_x_j) / k          (formed once on the host: one subtraction, one division)
//   S    = (tf - to) * unit_t / 2.0                     (mesh_kernel's expression)
//   Sh   = S * h;  Sh2 = Sh * 0.5;  Sh6 = Sh / 6.0
//   k1 = F(p,     y,                 U(p))              p = 2 (k j + i): the step's first stage point
//   k2 = F(p + 1, fma(Sh2, k1, y),   U(p + 1))
//   k3 = F(p + 1, fma(Sh2, k2, y),   U(p + 1))
//   k4 = F(p + 2, fma(Sh,  k3, y),   U(p + 2))
//   a  = fma(2, k2, k1);  a = fma(2, k3, a);  a = fma(1, k4, a)        (2 k exact: each line rounds once)
//   y  = fma(Sh6, a, y)
// F = section_rhs (gel_section_rhs.h) at the stage point's sigma; U(p) = the control samples of the plan's workspace.  Quaternions
// are never renormalised.
//
// THE CHAIN (GEL_PROP_CHAIN): phase 0 starts at its X_0; into phase s + 1, per component, jump = x(first node of s + 1) - x(last node
// of s) (one subtraction) and the start value is y itself where jump == 0, else y + jump (one addition).  The step is the one above.
// THE FACTORS (gel_propagate_dispersed*): thrust f0, mf_um f1, area f2 -- one product each, once per (vector, phase) -- and wn f3,
// we f3 on the interpolated wind inside F; a factor of 1.0 changes no bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gel_device.h"
#include "gel_ensemble.h"

namespace gel {

struct PropPhaseDev {
  int32_t n, k;          // collocation nodes, RK4 steps per node interval
  int32_t sampled;       // the phase has control samples (free attitude); a hold-type phase has none
  int32_t ntile;         // sample kernel: point tiles of kPropSampleThreads lanes, ceil(Pp / kPropSampleThreads); 0 if not sampled
  int32_t seg0;          // restart mode: first segment (node interval) of the phase; section mode: s
  int32_t pad;
  int64_t pt0;           // first stage point of the phase in the workspace's rows (counted over the sampled phases only)
  int64_t sg;            // offset (doubles) in PropDev::mat of sig [Pp]: the stage points
  int64_t hs;            // offset of hs [n]: the step of every node interval
  int64_t wu;            // offset of WuT [n][Pp]: WuT[j Pp + p] = Wu[p][j], the Lagrange basis on tau_1 .. tau_n at stage point p
  int64_t cu;            // offset (int32) in PropDev::cp of copy_u [Pp]: the collocation node a stage point IS, else -1
};

struct PropDev {
  int32_t S, restart;    // phases; 0: one segment = one phase, 1 (GEL_PROP_RESTART_NODE): one segment = one node interval
  int32_t nseg;          // S, or N in restart mode
  int32_t chain;         // 1 (GEL_PROP_CHAIN): one lane = one vector through all phases; nseg = S, every phase its own segment
  const PropPhaseDev* ph;
  const int32_t* seg_phase;   // [nseg] phase of every segment
  const double* mat;
  const int32_t* cp;
  double vp;             // unit_velocity / unit_position
};

constexpr int kPropThreads = 256;         // prop_kernel: 4 wavefronts, each 64 consecutive vectors of ONE segment
constexpr int kPropSampleThreads = 256;   // prop_sample_kernel: one lane per stage point of a tile
constexpr int kPropSampleVB = 4;          // prop_sample_kernel: decision vectors per workgroup
constexpr size_t kPropMaxLds = 64 * 1024;
constexpr int64_t kPropMaxLaneSteps = 1 << 20;   // steps[s] n_s (chain mode: their sum over the phases) may not exceed this: no lane runs longer
constexpr int kPropNDisp = 4;             // dispersion factors per (vector, phase): thrust, mass flow, reference area, wind (GEL_PROP_NDISP)

// bytes of LDS the sample kernel takes for a phase of n nodes: U [n][2][kPropSampleVB]
inline size_t prop_sample_lds_bytes(int n) { return (size_t)16 * n * kPropSampleVB; }

// One slab of nb vectors (x, y: the slab's first vector; ws: [stage point][2][ld] with ld >= nb):
// control samples into ws, then y [nb][11 M] from x [nb][nvars].  n_max_sampled sizes the sample kernel's LDS.  d_disp: the slab's
// factors [nb][S][kPropNDisp], or null (the undispersed instantiation).  ens: the wind ensemble with the SLAB's part of the
// assignment (ens.member = the entry of the slab's first vector), or ens.tables == null; with an ensemble the kernel's kEns
// instantiation runs, with factors of one where d_disp is null.
hipError_t launch_prop_slab(const ProblemDev& P, const PropDev& Pd, const PropPhaseDev* host_ph, int n_max_sampled, int nb,
                            const double* d_x, double* d_y, double* d_ws, int64_t ld, const double* d_disp, const EnsDev& ens,
                            hipStream_t s);
// err [B][S][4] from x and y (all B vectors in one launch)
hipError_t launch_prop_err(const ProblemDev& P, const PropDev& Pd, int B, const double* d_x, const double* d_y, double* d_err,
                           hipStream_t s);

}  // namespace gel
