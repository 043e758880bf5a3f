// gel_kernels_interp.hip -- batched spectral interpolation of the collocation solution (gel_interp*).
//
// Per phase the solution is a polynomial: degree n in the 11 state components on the support [-1, tau_1 .. tau_n], degree n - 1 in
// the 2 controls on tau_1 .. tau_n.  The kernel evaluates it at the plan's points: out = Wx X and Wu U, every output ONE fma chain
// over the support index in ascending order from +0.0 (the host form gel_interp_host runs the same chain: same bits), and a
// point that is a support node copies the node's value instead.
//
// A workgroup of kInterpThreads lanes = (a group of VB decision vectors, one phase, one tile of kInterpThreads points).  The
// phase's slice of the VB vectors is staged in LDS as [support node][component][VB]; one lane owns one point of ALL VB vectors:
// it loads a matrix element once (the matrices are stored transposed: one coalesced load per column and wavefront) and feeds the
// 11 VB state FMAs (2 VB control FMAs) with it from registers, the VB inputs of a (node, component) arriving as one LDS broadcast.
// Which vectors share a workgroup changes no bit of any of them.
#include <hip/hip_runtime.h>

#include "gel_interp.h"
#include "gel_flight_step.h"   // nonfinite

namespace gel {

template <int VB>
__global__ __launch_bounds__(kInterpThreads) void interp_kernel(InterpDev Id, int B, const double* __restrict__ x,
                                                                double* __restrict__ out, int32_t* flag) {
  extern __shared__ double lds[];
  // workgroup -> (phase, group of vectors, point tile): the phases' workgroups one after the other, the tiles of a group side by side
  const long long ng = ((long long)B + VB - 1) / VB;
  int s = 0;
  long long wg = blockIdx.x;
  for (; s < Id.S; s++) {
    const long long c = ng * Id.ph[s].ntile;
    if (wg < c) break;
    wg -= c;
  }
  if (s >= Id.S) return;   // (never: the grid is the sum over phases)
  const InterpPhaseDev ph = Id.ph[s];
  const long long grp = wg / ph.ntile;
  const int tile = (int)(wg - grp * ph.ntile);
  const int n = ph.n, np = n + 1, sx = interp_slice_doubles(n);
  const int M = Id.M, N = Id.N;
  const int t = threadIdx.x;

  // ---- stage X (state rows xa .. xa + n) and U (control rows ua .. ua + n - 1) of the group's vectors: five contiguous runs of
  //      x per vector; a tail group reads its last vector again ----
  const double* xv[VB];
#pragma unroll
  for (int v = 0; v < VB; v++) {
    const long long b = grp * VB + v;
    xv[v] = x + (size_t)(b < B ? b : B - 1) * Id.nvars;
  }
  for (int r = t; r < sx; r += kInterpThreads) {
    int g, k;
    if (r < np) { g = ph.xa + r; k = r * 11; }
    else if (r < 4 * np) { const int q = r - np; g = M + 3 * ph.xa + q; k = (q / 3) * 11 + 1 + q % 3; }
    else if (r < 7 * np) { const int q = r - 4 * np; g = 4 * M + 3 * ph.xa + q; k = (q / 3) * 11 + 4 + q % 3; }
    else if (r < 11 * np) { const int q = r - 7 * np; g = 7 * M + 4 * ph.xa + q; k = (q >> 2) * 11 + 7 + (q & 3); }
    else { const int q = r - 11 * np; g = 11 * M + 2 * ph.ua + q; k = 11 * np + q; }
#pragma unroll
    for (int v = 0; v < VB; v++) lds[(size_t)k * VB + v] = xv[v][g];
  }
  __syncthreads();

  const int l = tile * kInterpThreads + t;
  const double* const Us = lds + (size_t)11 * np * VB;
  bool bad = false;

  // ---- states at point l ----
  if (l < ph.P) {
    double a[11][VB];
#pragma unroll
    for (int c = 0; c < 11; c++)
#pragma unroll
      for (int v = 0; v < VB; v++) a[c][v] = 0.0;
    const double* W = Id.mat + ph.wx + l;
    for (int i = 0; i <= n; i++) {
      const double w = W[(size_t)i * ph.P];
      const double* Xi = lds + (size_t)i * 11 * VB;
#pragma unroll
      for (int c = 0; c < 11; c++)
#pragma unroll
        for (int v = 0; v < VB; v++) a[c][v] = __builtin_fma(w, Xi[c * VB + v], a[c][v]);
    }
    const int cx = Id.cp[ph.cx + l];
    if (cx >= 0) {
      const double* Xi = lds + (size_t)cx * 11 * VB;
#pragma unroll
      for (int c = 0; c < 11; c++)
#pragma unroll
        for (int v = 0; v < VB; v++) a[c][v] = Xi[c * VB + v];
    } else if (Id.unit_quat) {
#pragma unroll
      for (int v = 0; v < VB; v++) {
        const double q[4] = {a[7][v], a[8][v], a[9][v], a[10][v]};
        const double nrm = __builtin_sqrt(interp_quat_dot(q));
#pragma unroll
        for (int k = 0; k < 4; k++) a[7 + k][v] = q[k] / nrm;
      }
    }
    const double sig = Id.mode == 0 ? Id.mat[ph.sg + l] : 0.0;
#pragma unroll
    for (int v = 0; v < VB; v++) {
      const long long b = grp * VB + v;
      if (b >= B) continue;
#pragma unroll
      for (int c = 0; c < 11; c++) bad |= nonfinite(a[c][v]);
      if (Id.mode == 0) {
        double* o = out + (size_t)b * Id.ostride + (size_t)(ph.xd + l) * kInterpCols;
        const double tm = interp_time(sig, xv[v][11 * M + 2 * N + s], xv[v][11 * M + 2 * N + s + 1]);
        bad |= nonfinite(tm);
        o[0] = tm;
#pragma unroll
        for (int c = 0; c < 11; c++) o[1 + c] = a[c][v];
      } else {
        double* o = out + (size_t)b * Id.ostride;
        const int xi = ph.xd + l, Md = Id.Md;
        o[xi] = a[0][v];
#pragma unroll
        for (int c = 0; c < 3; c++) o[Md + 3 * xi + c] = a[1 + c][v];
#pragma unroll
        for (int c = 0; c < 3; c++) o[4 * Md + 3 * xi + c] = a[4 + c][v];
#pragma unroll
        for (int c = 0; c < 4; c++) o[7 * Md + 4 * xi + c] = a[7 + c][v];
      }
    }
  }

  // ---- controls at point l ----
  if (l < ph.Pu) {
    double u[2][VB];
#pragma unroll
    for (int v = 0; v < VB; v++) u[0][v] = u[1][v] = 0.0;
    const double* W = Id.mat + ph.wu + l;
    for (int j = 0; j < n; j++) {
      const double w = W[(size_t)j * ph.Pu];
      const double* Uj = Us + (size_t)j * 2 * VB;
#pragma unroll
      for (int c = 0; c < 2; c++)
#pragma unroll
        for (int v = 0; v < VB; v++) u[c][v] = __builtin_fma(w, Uj[c * VB + v], u[c][v]);
    }
    const int cu = Id.cp[ph.cu + l];
    if (cu >= 0) {
      const double* Uj = Us + (size_t)cu * 2 * VB;
#pragma unroll
      for (int c = 0; c < 2; c++)
#pragma unroll
        for (int v = 0; v < VB; v++) u[c][v] = Uj[c * VB + v];
    }
#pragma unroll
    for (int v = 0; v < VB; v++) {
      const long long b = grp * VB + v;
      if (b >= B) continue;
      bad |= nonfinite(u[0][v]) || nonfinite(u[1][v]);
      double* o = out + (size_t)b * Id.ostride;
      if (Id.mode == 0) o += (size_t)(ph.xd + l) * kInterpCols + 12;
      else o += 11 * Id.Md + 2 * (ph.ud + l);
      o[0] = u[0][v];
      o[1] = u[1][v];
    }
  }

  // ---- transfer mode: the knot times are copied; phase s carries t_s, the last phase t_S as well ----
  if (Id.mode == 1 && tile == 0 && t < VB) {
    const long long b = grp * VB + t;
    if (b < B) {
      const double* ti = x + (size_t)b * Id.nvars + 11 * M + 2 * N;
      double* to = out + (size_t)b * Id.ostride + 11 * Id.Md + 2 * Id.Nd;
      to[s] = ti[s];
      bad |= nonfinite(ti[s]);
      if (s == Id.S - 1) { to[s + 1] = ti[s + 1]; bad |= nonfinite(ti[s + 1]); }
    }
  }
  if (bad) *(volatile int32_t*)flag = 1;
}

hipError_t launch_interp(const InterpDev& Id, const InterpPhaseDev* host_ph, int n_max, int B, const double* d_x, double* d_out,
                         int32_t* flag, int vb, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const long long ng = ((long long)B + vb - 1) / vb;
  long long grid = 0;
  for (int i = 0; i < Id.S; i++) grid += ng * host_ph[i].ntile;
  if (grid == 0) return hipSuccess;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds = interp_lds_bytes(n_max, vb);
  if (lds > kInterpMaxLds) return hipErrorInvalidValue;
  const dim3 g((unsigned)grid), blk(kInterpThreads);
  if (vb == 4) hipLaunchKernelGGL(interp_kernel<4>, g, blk, lds, s, Id, B, d_x, d_out, flag);
  else if (vb == 2) hipLaunchKernelGGL(interp_kernel<2>, g, blk, lds, s, Id, B, d_x, d_out, flag);
  else if (vb == 1) hipLaunchKernelGGL(interp_kernel<1>, g, blk, lds, s, Id, B, d_x, d_out, flag);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace gel
