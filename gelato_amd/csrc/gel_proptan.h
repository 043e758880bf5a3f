// gel_proptan.h -- the tangent-linear propagation (gel_kernels_proptan.hip): one slab's launch.  The plan's tables
// are gel_prop.h's PropDev; the step and the order of its tangent are written down in gel_kernels_proptan.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gel_prop.h"

namespace gel {

// One slab of nb vectors with P directions each (every pointer: the slab's first vector / first lane).
struct PropTanArgs {
  int32_t nb, P, shared, pad;
  const double* x;       // [nb][nvars]
  const double* disp;    // [nb][S][kPropNDisp] or null: factors of one
  const double* dx;      // [nb][P][nvars], shared: [P][nvars]; or null: zero
  const double* ddisp;   // [nb][P][S][kPropNDisp], shared: [P][S][kPropNDisp]; or null: zero
  double* y;             // [nb][11 M]
  double* dy;            // [nb][P][11 M]
  const double* ws;      // the control samples [stage point][2][ld], ld >= nb
  const double* dws;     // the control directions' samples [stage point][2][dld], dld >= nb P (shared: P); not read where dx is null
  long long ld, dld;
};

// The wind seeds of a slab: dwind [nb][P][Kg][2], shared: [P][Kg][2] (the slab's first lane, like dx), or
// dwind == null: no wind seed.  Kg >= the row count of every table a lane of the launch may read.
struct WindSeedDev {
  const double* dwind;
  int32_t Kg, pad;
};

// ens: the wind ensemble with the SLAB's part of the assignment (ens.member = the entry of the slab's first vector; a lane's vector
// is lane / P), or ens.tables == null: the instantiations without an ensemble, launched as before
hipError_t launch_proptan_slab(const ProblemDev& P, const PropDev& Pd, const PropTanArgs& A, const EnsDev& ens, const WindSeedDev& wd,
                               hipStream_t s);

}  // namespace gel
