// gel_kernels_mesh.hip -- the LGR collocation error estimate per section (gel_mesh_error*).
//
// For one phase of n nodes and one decision vector: interpolate the state (support tau_x = [-1, tau]) and the control (support
// tau) onto the flipped LGR points sigma_1 .. sigma_{n+1} of n + 1, evaluate the right-hand side the phase's defect rows impose
// there, integrate it with the fine grid's Radau integration matrix I from X_0, and compare:
//   e_{j,c} = |X^_c(sigma_j) - X~_c(sigma_j)| / (1 + max_{l=0..n+1} |X~_c(sigma_l)|),   X^ = X_0 + S I F,  S = (tf - to) unit_t / 2
// Output: max_j e over the components of each group (mass, position, velocity, quaternion), and on request X^ - X~ per point.
//
// One lane = one (decision vector, test point) pair of one phase; a workgroup of kMeshMaxThreads lanes carries vpb = 512 / (n + 1)
// vectors of the same phase (3 at n = 128, 7 at n = 64) -- fewer where that many do not fit 64 KB of LDS beside the tables
// (gel_mesh.h mesh_vectors_per_group: 167 instead of 170 at n = 2 with the example's tables); lanes with v >= vpb stay idle.  Each vector's state (11 (n+1)) and control (2 n) are
// staged in LDS; the interpolation reads them as broadcasts and the matrices (transposed on the host: one coalesced load per
// column) through the cache.  The same LDS region then holds |X~| for the per-component maxima, the right-hand sides F for the
// product with I, and |X^ - X~| for the maxima over the points.  Nothing per point reaches HBM unless diff is asked for.
// fp64 throughout; the right-hand side is section_rhs (gel_section_rhs.h), built from the value functions of gel_rhs_parts.h /
// gel_physics.h.
#include <hip/hip_runtime.h>

#include "gel_tables.h"
#include "gel_section_rhs.h"
#include "gel_mesh.h"
#include "gel_flight_step.h"   // nan_max

namespace gel {

__global__ __launch_bounds__(kMeshMaxThreads) void mesh_kernel(ProblemDev P, MeshDev Md, int B, const double* __restrict__ x,
                                                               double* __restrict__ err, double* __restrict__ diff) {
  extern __shared__ double lds[];
  // workgroup -> (phase, group of vectors): the phases' workgroups one after the other
  int s = 0, grp = blockIdx.x;
  for (; s < Md.S; s++) {
    const int vpb_s = load_const(&Md.ph[s].vpb);
    const int ng = (B + vpb_s - 1) / vpb_s;
    if (grp < ng) break;
    grp -= ng;
  }
  if (s >= Md.S) return;   // (never: the grid is the sum over phases)
  const Tables tb = stage_tables(P, lds, false);
  const int n = load_const(&Md.ph[s].n), vpb = load_const(&Md.ph[s].vpb), pt0 = load_const(&Md.ph[s].pt0);
  const int np = n + 1;                       // test points
  const int sx = 11 * np + 2 * n;             // doubles per vector: X [11][n+1] | U [2][n]; later |X~|, F, |d| in its first 11 np
  double* const base = lds + ((table_doubles(P.Kw, P.Kc) + 1) & ~1);
  double* const Ex = base + (size_t)vpb * sx;   // [vpb][11] per-component maxima of |X~|, then e
  const int t = threadIdx.x, v = t / np, l = t - v * np;
  const long long b = (long long)grp * vpb + v;
  const bool act = v < vpb && b < B;
  const PhaseDev ph = load_phase(P.phases + s);
  const int M = P.M, N = P.N;

  // ---- stage X (support nodes xa .. xa + n) and U (collocation nodes ua .. ua + n - 1) of every vector of the group ----
  for (int k = t; k < vpb * sx; k += blockDim.x) {
    const int vv = k / sx, r = k - vv * sx;
    const long long bb = (long long)grp * vpb + vv;
    double val = 0.0;
    if (bb < B) {
      const double* xb = x + (size_t)bb * P.nvars;
      if (r < 11 * np) {
        const int c = r / np, i = r - c * np, xi = ph.xa + i;
        val = (c == 0) ? xb[xi] : (c < 4) ? xb[M + 3 * xi + (c - 1)] : (c < 7) ? xb[4 * M + 3 * xi + (c - 4)] : xb[7 * M + 4 * xi + (c - 7)];
      } else {
        const int r2 = r - 11 * np, c = r2 / n, j = r2 - c * n;
        val = xb[11 * M + 2 * (ph.ua + j) + c];
      }
    }
    base[(size_t)vv * sx + r] = val;
  }
  __syncthreads();
  double* const Xs = base + (size_t)(act ? v : 0) * sx;
  const double* const Us = Xs + 11 * np;

  // ---- interpolated state and control at sigma_{l+1} ----
  const double* const LxT = Md.mat + load_const(&Md.ph[s].lx);
  const double* const LuT = Md.mat + load_const(&Md.ph[s].lu);
  const double* const IT = Md.mat + load_const(&Md.ph[s].it);
  const double sig = act ? Md.mat[load_const(&Md.ph[s].sg) + l] : 0.0;
  double xt[11], x0[11];
#pragma unroll
  for (int c = 0; c < 11; c++) { xt[c] = 0.0; x0[c] = Xs[c * np]; }
  double u0 = 0.0, u1 = 0.0;
  if (act) {
    for (int i = 0; i <= n; i++) {
      const double w = LxT[(size_t)i * np + l];
#pragma unroll
      for (int c = 0; c < 11; c++) xt[c] = __builtin_fma(w, Xs[c * np + i], xt[c]);
    }
    if (!ph.hold)
      for (int j = 0; j < n; j++) {
        const double w = LuT[(size_t)j * np + l];
        u0 = __builtin_fma(w, Us[j], u0);
        u1 = __builtin_fma(w, Us[n + j], u1);
      }
  }
  __syncthreads();   // X and U are read: the region takes |X~| now

  // ---- per-component maxima of |X~| over sigma_0 .. sigma_{n+1} (X~(sigma_0) = X_0) ----
  if (act) {
#pragma unroll
    for (int c = 0; c < 11; c++) Xs[c * np + l] = (l == 0) ? nan_max(fabs(xt[c]), fabs(x0[c])) : fabs(xt[c]);
  }
  __syncthreads();
  if (act)
    for (int c = l; c < 11; c += np) {   // lane l reduces components l, l + np, ... (a phase of n = 2 has 3 lanes per vector)
      double mx = 0.0;
      for (int k = 0; k < np; k++) mx = nan_max(mx, Xs[c * np + k]);
      Ex[v * 11 + c] = mx;
    }
  __syncthreads();

  // ---- right-hand side of the phase's defect rows at the test point ----
  const double* xb = x + (size_t)(act ? b : 0) * P.nvars;
  const double to = xb[11 * M + 2 * N + s], tf = xb[11 * M + 2 * N + s + 1];
  const double S = (tf - to) * P.ut / 2.0;
  double F[11];
  if (act) {   // (idle lanes stay out of the calm-air vote of wind_eci_or_calm)
    section_rhs(P, ph, tb, Md.vp, sig, to, tf, xt, u0, u1, F);
#pragma unroll
    for (int c = 0; c < 11; c++) Xs[c * np + l] = F[c];
  }
  __syncthreads();

  // ---- X^(sigma_{l+1}) = X_0 + S sum_k I[l][k] F_k; the difference to X~ ----
  double d[11];
#pragma unroll
  for (int c = 0; c < 11; c++) d[c] = 0.0;
  if (act) {
    for (int k = 0; k < np; k++) {
      const double w = IT[(size_t)k * np + l];
#pragma unroll
      for (int c = 0; c < 11; c++) d[c] = __builtin_fma(w, Xs[c * np + k], d[c]);
    }
#pragma unroll
    for (int c = 0; c < 11; c++) d[c] = __builtin_fma(S, d[c], x0[c]) - xt[c];
    if (diff) {
      double* o = diff + ((size_t)b * Md.npts + pt0 + l) * 11;
#pragma unroll
      for (int c = 0; c < 11; c++) o[c] = d[c];
    }
  }
  __syncthreads();   // F is read: the region takes |X^ - X~|
  if (act) {
#pragma unroll
    for (int c = 0; c < 11; c++) Xs[c * np + l] = fabs(d[c]);
  }
  __syncthreads();
  if (act)
    for (int c = l; c < 11; c += np) {
      double md = 0.0;
      for (int k = 0; k < np; k++) md = nan_max(md, Xs[c * np + k]);
      Ex[v * 11 + c] = md / (1.0 + Ex[v * 11 + c]);   // max_j (|d_j| / den) = (max_j |d_j|) / den: the rounded quotient is monotone
    }
  __syncthreads();
  if (act)
    for (int g = l; g < 4; g += np) {
      const int c0 = (g == 0) ? 0 : 3 * g - 2, c1 = (g == 0) ? 1 : (g == 3) ? 11 : 3 * g + 1;   // [0,1) [1,4) [4,7) [7,11)
      double e = 0.0;
      for (int c = c0; c < c1; c++) e = nan_max(e, Ex[v * 11 + c]);
      err[((size_t)b * Md.S + s) * 4 + g] = e;
      if (!(e <= 1.79769313486231570815e308)) *(volatile int32_t*)P.flag = 1;
    }
}

hipError_t launch_mesh(const ProblemDev& P, const MeshDev& Md, const MeshPhaseDev* host_ph, int B, const double* d_x, double* d_err,
                       double* d_diff, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  long long grid = 0;
  size_t lds = 0;
  for (int i = 0; i < Md.S; i++) {
    grid += (B + host_ph[i].vpb - 1) / host_ph[i].vpb;
    if ((size_t)host_ph[i].lds > lds) lds = (size_t)host_ph[i].lds;
  }
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mesh_kernel, dim3((unsigned)grid), dim3(kMeshMaxThreads), lds, s, P, Md, B, d_x, d_err, d_diff);
  return hipGetLastError();
}

}  // namespace gel
