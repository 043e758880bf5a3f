// gel_kernels_exact_rows.hip -- the exact Jacobian of the node-function rows of the row table (GEL_FLAG_EXACT_ROWS_JAC): every
// jfn entry as s (df / dx_c) / p[0] (s = -1 with mode & 8), the derivative of the row's function with respect to the normalised
// column c (position xyz, velocity xyz of the row's node, its knot time), formed in fp64 forward mode (gel_exact_rows.h).  The row
// values are not formed here: the host launches rows_kernel without a jfn output first, so they stay bit-identical to a handle
// without the flag.
//
// rows_body's layout: eight lanes per (decision vector, node-function row), lane 1 + c carries direction c as a scalar dual
// (value, tangent) seeded with (c == k) ? unit : 0; lane 0 has nothing to do.  The value parts of a row's lanes are the same, so
// its lanes take the same branches and leave Vincenty's loop together.  Columns the function does not read are exact zeros
// without evaluating it: the knot time of fn 0 .. 8 and of rows with tcol < 0, the velocity of fn 9 .. 11, 14 and 15.
#include <hip/hip_runtime.h>

#include "gel_launch.h"
#include "gel_exact_rows.h"

namespace gel {

constexpr int kExactRowsBlock = 256;

__global__ __launch_bounds__(kExactRowsBlock) void exact_rows_kernel(ProblemDev P, int nfn, const FnRowDev* __restrict__ fr, int B,
                                                                      const double* __restrict__ x, double* __restrict__ jfn) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long grp = t >> 3;
  const int c = (int)(t & 7) - 1;                   // -1 idle, 0..2 position xyz, 3..5 velocity xyz, 6 knot time
  if (c < 0 || grp >= (long long)B * nfn) return;
  const int b = (int)(grp / nfn), row = (int)(grp - (long long)b * nfn);
  const FnRowDev F = fr[row];
  const bool vel_free = F.fn >= 9 && F.fn != 12 && F.fn != 13;
  const bool zero = (c == 6) ? (F.fn <= 8 || F.tcol < 0) : (c >= 3 && vel_free);
  double d = 0.0;
  if (!zero) {
    const double* xb = x + (size_t)b * P.nvars;
    Dual r[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      r[k] = Dual{xb[P.M + 3 * F.node + k] * P.up, (c == k) ? P.up : 0.0};
      v[k] = Dual{xb[4 * P.M + 3 * F.node + k] * P.uv, (c == 3 + k) ? P.uv : 0.0};
    }
    Dual tk = {0.0, 0.0};
    if (F.tcol >= 0) tk = Dual{xb[11 * P.M + 2 * P.N + F.tcol] * P.ut, (c == 6) ? P.ut : 0.0};
    d = node_fn_dual(F.fn, r, v, tk, F.p).d / F.p[0];
    if (F.mode & 8) d = -d;
  }
  jfn[((size_t)b * nfn + row) * 7 + c] = d;
  if (!(fabs(d) <= 1.79769313486231570815e308)) *(volatile int32_t*)P.flag = 1;  // every writer stores the same 1
}

hipError_t launch_rows_exact(const ProblemDev& P, int nfn, const FnRowDev* fr, int B, const double* d_x, double* d_jfn, hipStream_t s) {
  if (B <= 0 || nfn <= 0) return hipSuccess;
  const long long threads = (long long)B * nfn * 8;
  const unsigned grid = (unsigned)((threads + kExactRowsBlock - 1) / kExactRowsBlock);
  hipLaunchKernelGGL(exact_rows_kernel, dim3(grid), dim3(kExactRowsBlock), 0, s, P, nfn, fr, B, d_x, d_jfn);
  return hipGetLastError();
}

}  // namespace gel
