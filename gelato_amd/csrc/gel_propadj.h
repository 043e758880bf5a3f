// gel_propadj.h -- the adjoint flight (gel_kernels_propadj.hip): one slab's launches.  The plan's tables are
// gel_prop.h's PropDev; the reversed step and the order of every accumulation are written down in gel_kernels_propadj.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gel_prop.h"

namespace gel {

constexpr int kPropAdjThreads = 64;       // propadj_kernel: one wavefront, F1 .. F3 of its lanes in LDS (3 x 11 x 64 doubles)
constexpr int kPropAdjSampleThreads = 256;   // prop_sample_t_kernel: consecutive lanes of one control node (or of the knot times)

// One slab of nb vectors with Q functionals each (every pointer: the slab's first vector / first lane); lane l = functional l % Q of
// vector l / Q.
struct PropAdjArgs {
  int32_t nb, Q, shared, pad;
  const double* x;       // [nb][nvars]
  const double* disp;    // [nb][S][kPropNDisp] or null: factors of one
  const double* lam;     // [nb][Q][11 M], shared: [Q][11 M]
  const double* y;       // [nb][11 M]: the value flight's result = the checkpoints
  double* gx;            // [nb][Q][nvars]
  double* gdisp;         // [nb][Q][S][kPropNDisp] or null
  const double* ws;      // the control samples [stage point][2][ld], ld >= nb
  double* gws;           // the stage points' control adjoints [stage point][2][gld], gld >= nb Q: every cell stored once
  double* gS;            // the adjoint of S h's factor S of every (phase, lane): [S][gld]
  double* ck;            // inner checkpoints, the starts of steps 1 .. k - 1 of the interval in hand: [k_max - 1][11][gld] (never null);
                         // a lane's column has ONE user: the lane's thread, which walks all its phases (section mode too)
  long long ld, gld;
};

// The wind rows' gradient of a slab: gww [Kg][2][gld] the lanes' columns (workspace, zeroed by the launch), gwind
// [nb][Q][Kg][2] the result (the slab's first lane), or gwind == null: not wanted.  Kg >= the row count of every table a lane of the
// launch may read.
struct WindGradDev {
  double* gww;
  double* gwind;
  int32_t Kg, pad;
};

// propadj_kernel (state rows of gx, gdisp, gws, gS), then prop_sample_t_kernel (control and time entries of gx).  ens: the wind
// ensemble with the SLAB's part of the assignment (a lane's vector is lane / Q), or ens.tables == null: the instantiations without
// an ensemble, launched as before.  With an ensemble A.y must be the ensemble flight's (prop_kernel<*, *, 1> under
// the same assignment): the checkpoints.  wg.gwind == null: the instantiations without the wind rows, launched as before
hipError_t launch_propadj_slab(const ProblemDev& P, const PropDev& Pd, const PropAdjArgs& A, const EnsDev& ens, const WindGradDev& wg,
                               hipStream_t s);

}  // namespace gel
