// gel_mesh.h -- the LGR collocation error estimate per section (gel_kernels_mesh.hip): its tables and its launcher.  The tables
// travel in a struct of their own (MeshDev), so that ProblemDev -- which every other kernel takes by value -- keeps its layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gel_device.h"
#include "gel_launch.h"

namespace gel {

// One phase of n collocation nodes: P = n + 1 test points, the flipped LGR points sigma_1 .. sigma_P of n + 1 (sigma_P = +1).
// The phase's matrices lie in MeshDev::mat TRANSPOSED, point index fastest, so that the lanes of one vector (one test point
// each) read a matrix column with one coalesced load:
//   LxT [(n+1) support nodes][P]   LxT[i P + l] = Lx[l][i]   Lagrange basis on tau_x = [-1, tau_1 .. tau_n] at sigma_{l+1}
//   LuT [n collocation nodes][P]   LuT[j P + l] = Lu[l][j]   Lagrange basis on tau_1 .. tau_n at sigma_{l+1}
//   IT  [P][P]                     IT[k P + l]  = I[l][k]    Radau integration matrix of the fine grid, (D^[:, 1:])^-1
//   sig [P]                        sigma_1 .. sigma_P
struct MeshPhaseDev {
  int32_t n, vpb;        // collocation nodes; decision vectors per workgroup (mesh_vectors_per_group: kMeshMaxThreads / P, or what fits the LDS)
  int32_t pt0;           // first test point of the phase in the [npts] rows of the optional differences
  int32_t pad;
  int64_t lx, lu, it, sg;  // offsets (doubles) of LxT, LuT, IT and sigma in MeshDev::mat
  int64_t lds;           // bytes of LDS a workgroup of this phase takes (tables included)
};

struct MeshDev {
  int32_t S, npts;       // phases; sum over phases of n + 1
  const MeshPhaseDev* ph;
  const double* mat;
  double vp;             // unit_velocity / unit_position: the position rows' right-hand side per unit of normalised velocity
};

constexpr int kMeshMaxThreads = 512;   // workgroup size of mesh_kernel: phases of up to 511 nodes
// LDS of a phase of n nodes: the padded tables, then per vector X [11][n+1] | U [2][n] and the 11 per-component maxima.  A workgroup
// takes as many decision vectors as it has lanes for (kMeshMaxThreads / (n + 1)) and as fit kLaunchMaxLds beside the tables
// (MeshPhaseDev::vpb, ::lds; a short phase is bound by the LDS: 170 vectors of n = 2 alone take 65 280 bytes), at least one: a
// phase whose single vector does not fit is refused by the host (gel_mesh_error*)
inline size_t mesh_vector_doubles(int n) { return 11 * (size_t)(n + 1) + 2 * (size_t)n + 11; }
inline int mesh_vectors_that_fit(int Kw, int Kc, int n) {   // beside the tables, under kLaunchMaxLds; 1 if not even one does
  const size_t cap = kLaunchMaxLds / sizeof(double), tab = padded_table_doubles(Kw, Kc);
  const size_t fit = tab < cap ? (cap - tab) / mesh_vector_doubles(n) : 0;
  return (int)(fit > 0 ? (fit < (size_t)kMeshMaxThreads ? fit : (size_t)kMeshMaxThreads) : 1);
}
inline int mesh_vectors_per_group(int Kw, int Kc, int n) {
  const int lanes = kMeshMaxThreads / (n + 1), fit = mesh_vectors_that_fit(Kw, Kc, n);
  return fit < lanes ? fit : lanes;
}
inline size_t mesh_lds_bytes(int Kw, int Kc, int n) {
  return sizeof(double) * (padded_table_doubles(Kw, Kc) + (size_t)mesh_vectors_per_group(Kw, Kc, n) * mesh_vector_doubles(n));
}

// err [B][S][4] (mass, position, velocity, quaternion); diff [B][npts][11] or null.  The non-finite flag is P.flag.
hipError_t launch_mesh(const ProblemDev& P, const MeshDev& Md, const MeshPhaseDev* host_ph, int B, const double* d_x, double* d_err,
                       double* d_diff, hipStream_t s);

}  // namespace gel
