// gel_kernels_rows.hip -- the row table (rows_kernel: rows_body of gel_rows_body.h, launch_rows) and the post-processing table
// (output_kernel: output_row of gel_output_row.h, launch_output).
#include "gel_rows_body.h"

namespace gel {

__global__ void rows_kernel(ProblemDev P, int nlin, const LinRowDev* __restrict__ lin, int nfn,
                            const FnRowDev* __restrict__ fr, int B, int lin_blocks, const double* __restrict__ x,
                            double* __restrict__ con, double* __restrict__ jfn) {
  rows_body(P, nlin, lin, nfn, fr, B, lin_blocks, x, con, jfn, blockIdx.x);
}

hipError_t launch_rows(const ProblemDev& P, int nlin, const LinRowDev* lin, int nfn, const FnRowDev* fr, int B,
                       const double* d_x, double* d_con, double* d_jfn, hipStream_t s) {
  if (B <= 0 || nlin + nfn <= 0) return hipSuccess;
  const int lb = (int)(((long long)B * nlin + 255) / 256), fb = (int)(((long long)B * nfn * 8 + 255) / 256);
  hipLaunchKernelGGL(rows_kernel, dim3((unsigned)(lb + fb)), dim3(256), 0, s, P, nlin, lin, nfn, fr, B, lb, d_x, d_con, d_jfn);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Post-processing table (output_result.py:37-263): one thread per state node, kOutputCols values
// per node in the order of include/gelato_amd.h GEL_OUTPUT_*.  Runs once after the optimiser has finished: written for
// agreement with the reference's formulas (same operation order, libm calls where the reference has them), not speed.
// The row itself is output_row (gel_output_row.h), which the batched table (gel_kernels_outbatch.hip) shares.
// ---------------------------------------------------------------------------
constexpr int kOutputCols = kOutputColumns;
__global__ void output_kernel(ProblemDev P, int M, const double* __restrict__ x, const double* __restrict__ tx,
                              const int32_t* __restrict__ node_sec, double lat0, double lon0, double* __restrict__ out) {
  extern __shared__ double lds[];
  const Tables tb = stage_tables(P, lds);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const PhaseDev ph = P.phases[node_sec[i]];
  output_row<false>(P, tb, ph, M, i, x, tx[i], lat0, lon0, out + (size_t)i * kOutputCols, kRowAll, 1.0);
}

hipError_t launch_output(const ProblemDev& P, int M, const double* d_x, const double* d_tx, const int32_t* d_node_sec,
                         double lat0, double lon0, double* d_out, hipStream_t s) {
  hipLaunchKernelGGL(output_kernel, dim3((M + 63) / 64), dim3(64), table_lds_bytes(P.Kw, P.Kc), s, P, M, d_x, d_tx, d_node_sec,
                     lat0, lon0, d_out);
  return hipGetLastError();
}

}  // namespace gel
