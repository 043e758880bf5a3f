// gel_ensemble.h -- the wind ensemble of a Monte-Carlo batch (gel_wind_ensemble*): what host and kernels share.
// E member tables of Kw rows each lie in DEVICE memory, every member staged like a handle's own wind table (its rows [Kw][3]
// followed by its slopes [Kw - 1][2]: append_rows_and_slopes, 5 Kw - 2 doubles), and one int32 per vector of the batch selects the
// member its flight and its table rows look the wind up in: -1 the handle's own table, else 0 .. E - 1.  The host validates the
// assignment before it uploads it, so no kernel forms an address from an unchecked index.
// The struct travels as a kernel argument of its own behind the existing ones (ProblemDev keeps its layout); tables == nullptr
// is a launch without an ensemble.
#pragma once
#include <stdint.h>

namespace gel {

struct EnsDev {
  const double* tables;    // [E][stride], or null: no ensemble
  const int32_t* member;   // the assignment, from the launch's first vector on
  int32_t E, Kw;
  int64_t stride;          // doubles per member: 5 Kw - 2
};

constexpr int64_t kEnsMaxDoubles = 1LL << 27;   // E (5 Kw - 2) at the most: 1 GB
constexpr int32_t kEnsMaxRows = 1 << 20;        // Kw at the most: a bisection of 20 steps

#ifdef GEL_DEV   // the kernels' translation units (gel_tables.h comes first there)
// The lane's view of the tables under an ensemble: atmosphere and CA stay the workgroup's LDS copies, the wind part points into
// GLOBAL memory for every lane -- the member's block, or for -1 the handle's own global copy P.tables, of which the LDS image is a
// memcpy: the same bits -- so that no lane mixes address spaces in one load.  m: the vector's entry of the assignment.
GEL_DEV Tables ens_lane_tables(const ProblemDev& P, const Tables& tb, const EnsDev& E, int m) {
  const bool own = m < 0;
  const double* const w = own ? P.tables + kAtmDoubles : E.tables + (size_t)m * (size_t)E.stride;
  Tables t = tb;
  t.Kw = own ? P.Kw : E.Kw;
  t.wind = w;
  t.winds = w + (own ? 3 * P.Kw + 2 * P.Kc : 3 * E.Kw);
  return t;
}
// The same view for the lane of vector v of the launch (v counts from the slab's first vector, as member does): what the tangent
// and the adjoint flight take.  Their tb already lies in global memory, atmosphere and CA included; only the wind
// part changes.
GEL_DEV Tables ens_lane_view(const ProblemDev& P, const Tables& tb, int v, const EnsDev& E) {
  return ens_lane_tables(P, tb, E, E.member[v]);
}
#endif

}  // namespace gel
