// gel_interp.h -- batched spectral interpolation of the collocation solution (gel_kernels_interp.hip): dense
// output at any points inside the sections, and transfer of decision vectors to another mesh.  The tables travel in a struct of
// their own (InterpDev), as MeshDev and JprodDev do, so that ProblemDev keeps its layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gel {

// One phase of n source nodes, evaluated at P state points and Pu control points (table mode: P = Pu = the phase's points;
// transfer mode: P = n_d + 1 at [-1, tau^d], Pu = n_d at tau^d).  The phase's matrices lie in InterpDev::mat TRANSPOSED, point
// index fastest, so that the lanes of a wavefront (one point each) read a matrix column with one coalesced load:
//   WxT [(n+1) support nodes][P]    WxT[i P + l]  = Wx[l][i]   Lagrange basis on [-1, tau_1 .. tau_n] at point l
//   WuT [n collocation nodes][Pu]   WuT[j Pu + l] = Wu[l][j]   Lagrange basis on tau_1 .. tau_n at point l
//   sig [P]                         the points (table mode only: the time column)
// and in InterpDev::cp: copy_x [P], copy_u [Pu] -- the support index of a point that IS a support node (its value is copied,
// not multiplied), else -1.
struct InterpPhaseDev {
  int32_t n, xa, ua;     // source: collocation nodes, first state row, first control row
  int32_t P, Pu;         // state points, control points
  int32_t ntile;         // point tiles of kInterpThreads lanes: ceil(max(P, Pu) / kInterpThreads); 0 for a phase without points
  int32_t xd, ud;        // table mode: xd = first row of the phase in the [npts] rows; transfer mode: first state / control row of
                         // the phase in the destination's packed vector
  int64_t wx, wu, sg;    // offsets (doubles) of WxT, WuT and sig in InterpDev::mat
  int64_t cx, cu;        // offsets (int32) of copy_x and copy_u in InterpDev::cp
};

struct InterpDev {
  int32_t S, mode;       // phases; 0 table, 1 transfer
  int32_t unit_quat;     // GEL_INTERP_UNIT_QUAT: rows that are not copies get q / sqrt(q . q)
  int32_t nvars;         // source: doubles per decision vector
  int32_t M, N;          // source: state rows, control rows
  int32_t Md, Nd;        // transfer mode: the destination's
  int64_t ostride;       // doubles per output vector: 14 npts (table) or the destination's num_vars (transfer)
  const InterpPhaseDev* ph;
  const double* mat;
  const int32_t* cp;
};

constexpr int kInterpThreads = 256;           // workgroup size of interp_kernel: one lane per output point of a tile
constexpr size_t kInterpMaxLds = 64 * 1024;   // LDS a workgroup may take (the default limit of a launch without attributes)
constexpr int kInterpCols = 14;               // table mode: time | mass, position 3, velocity 3, quaternion 4 | u 2

// doubles of one vector's staged slice of a phase of n nodes: X [n+1][11] | U [n][2]
inline __host__ __device__ int interp_slice_doubles(int n) { return 13 * n + 11; }
// bytes of LDS a workgroup of vb vectors takes for a phase of n nodes
inline size_t interp_lds_bytes(int n, int vb) { return 8 * (size_t)interp_slice_doubles(n) * vb; }
// vectors per workgroup (4, 2 or 1): the most whose staged slice of the longest phase fits; 0: none does
inline int interp_vectors_per_group(int n_max) {
  for (int vb = 4; vb >= 1; vb >>= 1)
    if (interp_lds_bytes(n_max, vb) <= kInterpMaxLds) return vb;
  return 0;
}

// The normalised time of point sigma in a phase [to, tf]: mesh_kernel's expression, kept from contraction so that the host and
// the device round it alike.
inline __host__ __device__ double interp_time(double sigma, double to, double tf) {
#pragma clang fp contract(off)
  return sigma * (tf - to) / 2 + (tf + to) / 2;
}
// q . q as one fma chain over components 0 .. 3 from +0.0
inline __host__ __device__ double interp_quat_dot(const double* q) {
  double d = 0.0;
  for (int k = 0; k < 4; k++) d = __builtin_fma(q[k], q[k], d);
  return d;
}

// out [B][ostride] from x [B][nvars]; n_max: the longest source phase that has points (sizes the LDS); vb: vectors per workgroup
// (1, 2 or 4; a vector's results do not depend on it).  Rows behind B are not written.  The non-finite flag is *flag.
hipError_t launch_interp(const InterpDev& Id, const InterpPhaseDev* host_ph, int n_max, int B, const double* d_x, double* d_out,
                         int32_t* flag, int vb, hipStream_t s);

}  // namespace gel
