// gel_kernels_conprod.hip -- the batched products with K, the Jacobian of every row that is not a defect row (gel_con_matvec*,
// gel_con_rmatvec*).
//
//   y_b = K(x_b) v_b           y [B][R]          g_b = K(x_b)^T lambda_b       g [B][num_vars]
//
// K is never formed: its entries are read where the launches that produce them leave them -- jfn of gel_rows_eval_device, the
// dense gradient arrays of gel_eval_aero_all_device or the records of gel_eval_batch_aero_device -- through the tables of
// gel_conprod.h, built on the host from the row table and from the walk behind gel_aero_pattern / gel_aero_record_map.
//
// One lane = one output of one vector (a row of K v, a column of K^T lambda), lanes in output order inside a vector: the lanes
// that walk the nodes of an aero spec read neighbouring doubles of part A's [column][node] rows (whole lines), and the table
// elements of neighbouring outputs lie side by side.  An output is ONE fma chain from +0.0 over its table row: the order is the
// table's, which the handle's configuration alone decides -- not B, not the vector's place in the batch, not the source form, not
// a launch parameter.  The time columns of K^T lambda (the only long rows) are one lane each as well: no floating-point atomics,
// no workspace.  A lane loads everything (its input with accumulate included) before its single store.  64-bit addressing
// throughout: at mixed-6x64 and B = 65536 the record buffer is 6 GB.  fp64, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "gel_conprod.h"

namespace gel {
namespace {

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.79769313486231570815e308; }

constexpr int kConprodThreads = 256;

__global__ __launch_bounds__(kConprodThreads) void conprod_kernel(ConprodOpDev op, ConprodVals vals, long long total,
                                                                  const double* __restrict__ in, double* out, int accumulate,
                                                                  int32_t* flag) {
  const long long t = (long long)blockIdx.x * kConprodThreads + threadIdx.x;
  if (t >= total) return;
  const long long b = t / op.nout;
  const int o = (int)(t - b * op.nout);
  const double* const inb = in + (size_t)b * op.nin;
  const double* const jfn = vals.jfn + (size_t)b * vals.jfn_stride;
  const double* const a0 = vals.aero[0] + (size_t)b * vals.aero_stride[0];
  const double* const a1 = vals.aero[1] + (size_t)b * vals.aero_stride[1];
  const double* const a2 = vals.aero[2] + (size_t)b * vals.aero_stride[2];
  const int e0 = op.ptr[o], e1 = op.ptr[o + 1];
  double acc = 0.0;
  for (int e = e0; e < e1; e++) {
    const int sc = op.src[e];
    double a;
    if (sc == kConSrcConst) {
      a = op.cval[e];
    } else {
      const double* const base = (sc == kConSrcJfn) ? jfn : (sc == kConSrcAero0) ? a0 : (sc == kConSrcAero0 + 1) ? a1 : a2;
      a = base[op.off[e]];
    }
    acc = __builtin_fma(a, inb[op.idx[e]], acc);
  }
  if (accumulate) acc = out[t] + acc;
  out[t] = acc;
  if (!finite64(acc)) *(volatile int32_t*)flag = 1;
}

}  // namespace

hipError_t launch_conprod(const ConprodOpDev& op, const ConprodVals& vals, int B, const double* d_in, double* d_out,
                          int accumulate, int32_t* flag, hipStream_t s) {
  if (B <= 0 || op.nout <= 0) return hipSuccess;
  const long long total = (long long)B * op.nout;
  const long long grid = (total + kConprodThreads - 1) / kConprodThreads;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(conprod_kernel, dim3((unsigned)grid), dim3(kConprodThreads), 0, s, op, vals, total, d_in, d_out, accumulate,
                     flag);
  return hipGetLastError();
}

}  // namespace gel
